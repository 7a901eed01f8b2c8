"""Record the ``cnn_module_kernel`` fixture of tests/test_gpu_conv_kernel.py from the REAL reference modules (imported unmodified
through oracle/shims) on CPU: ``python -m tools.make_conv_kernel_golden``.  Where the reference checkout is absent, ``record()``
goes through the oracle instead (as tools/make_wide_golden.py does), so that the CPU test can recompute the file on either machine.

Synthetic weights: ``synthetic.conformer_state_dict(0, 50, num_blocks=2, kernel=K)`` and
``synthetic.squeezeformer_state_dict(0, 50, num_blocks=4, kernel=K, streaming=...)`` with reduce_idx 1 / recover_idx 3; the inputs
are those of tools/make_wide_golden.py.  Every record is a function of seeds.  ``conv_kernel_v50.npz`` holds probabilities only,
plus the final caches of one chunk run per family (the smallest ones: the file stays under 1 MiB).  Keys, with ``<b>`` = ``s`` /
``n`` for streaming: True / False:
  ``c<K><b>_b3``, ``c<K><b>_67``, ``c<K><b>_403``      Conformer 256 / 4: get_encoder_out of the ragged B = 3 batch, of one utterance
                                                    of 67 frames and of one of 403 frames
  ``cbn<K><b>_b3``                                   the same batch with cnn_module_norm: batch_norm
  ``c<K>_chunk_<r>``                                 three 67-frame get_encoder_out_chunk steps (stride 64), required_cache_size r
  ``c8_chunk_att_16``, ``c8_chunk_cnn_16``           the final caches of the K = 8, r = 16 run
  ``w31<b>_b3``, ``w31<b>_67``, ``w31_chunk_-1``     Conformer 512 / 8 at K = 31
  ``q<K><b>_b3``, ``q<K><b>_67``, ``q<K><b>_403``      Squeezeformer
  ``q<K>_chunk_-1``, ``q8_chunk_cnn_-1``             its chunk steps, and the final cnn cache of the K = 8 run
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import shims                   # noqa: E402
from masr_amd.utils import synthetic      # noqa: E402
from tools.make_wide_golden import CHUNKS, ragged_inputs, single_inputs      # noqa: E402,F401

OUT = os.path.join(ROOT, 'tests', 'golden', 'conv_kernel_v50.npz')
V = 50
LIMIT = 1 << 20
SQZ_IDX = {'reduce_idx': 1, 'recover_idx': 3}
# (K, streaming) of the full-context records
CONFORMER = [(31, True), (31, False), (9, True), (9, False), (8, True), (3, True)]
CONFORMER_BN = [(31, False), (9, True)]
CONFORMER_CHUNK = [(31, -1), (31, 16), (8, -1), (8, 16)]
WIDE = [(31, True), (31, False)]
SQUEEZEFORMER = [(15, True), (15, False), (8, True), (7, False)]
SQUEEZEFORMER_CHUNK = [15, 8]


def conformer_sd(K, norm='layer_norm', wide=False):
    more = {'d': 512, 'heads': 8} if wide else {}
    return synthetic.conformer_state_dict(0, V, num_blocks=2, kernel=K, cnn_module_norm=norm, **more)


def squeezeformer_sd(K, streaming):
    return synthetic.squeezeformer_state_dict(0, V, num_blocks=4, kernel=K, streaming=streaming)


def _live(family, sd, streaming, tmp, **conf):
    """the live reference model with the synthetic weights, in eval mode"""
    shims.install()
    if family == 'conformer':
        from masr.model_utils.conformer.model import ConformerModel as M
    else:
        from masr.model_utils.squeezeformer.model import SqueezeformerModel as M
    cfg = yaml.safe_load(open(os.path.join(shims.REFERENCE_ROOT, 'configs', family + '.yml'), encoding='utf-8'))
    cfg['encoder_conf'].update(conf)
    p = os.path.join(tmp, 'mean_istd.json')
    json.dump({'mean': sd['encoder.global_cmvn.mean'].tolist(), 'istd': sd['encoder.global_cmvn.istd'].tolist(),
               'feature_method': 'fbank'}, open(p, 'w'))
    torch.manual_seed(0)
    m = M(input_dim=80, vocab_size=V, mean_istd_path=p, streaming=streaming, encoder_conf=cfg['encoder_conf'],
          decoder_conf=cfg['decoder_conf'], **cfg['model_conf'])
    missing, unexpected = m.load_state_dict(sd, strict=False)
    # (the attention decoder is not part of the synthetic weights and not of get_encoder_out*)
    missing = [k for k in missing if not k.startswith('decoder.') and 'concat_linear' not in k]
    assert not unexpected and not missing, (missing, unexpected)
    return m.eval()


class Oracle:
    """the reference's two entry points through the oracle (where the reference checkout is absent)"""

    def __init__(self, family, sd, streaming, K, heads=4):
        from oracle import conformer, squeezeformer
        self.sd, self.K = sd, K
        if family == 'conformer':
            self.m, self.full, self.chunk = conformer, {'heads': heads, 'kernel': K, 'streaming': streaming}, {'heads': heads, 'kernel': K}
        else:
            self.m, self.full, self.chunk = squeezeformer, dict(SQZ_IDX, kernel=K, causal=streaming), dict(SQZ_IDX, kernel=K)

    def get_encoder_out(self, feats, lens):
        return self.m.get_encoder_out(self.sd, feats, lens, **self.full)

    def get_encoder_out_chunk(self, x, off, rcs, att, cnn):
        return self.m.get_encoder_out_chunk(self.sd, x, off, rcs, att, cnn, **self.chunk)


def conformer_model(K, streaming, tmp=None, norm='layer_norm', wide=False):
    sd = conformer_sd(K, norm, wide)
    if not tmp:
        return Oracle('conformer', sd, streaming, K, 8 if wide else 4)
    conf = dict(num_blocks=2, cnn_module_kernel=K, cnn_module_norm=norm)
    if wide:
        conf.update(output_size=512, attention_heads=8)
    return _live('conformer', sd, streaming, tmp, **conf)


def squeezeformer_model(K, streaming, tmp=None):
    sd = squeezeformer_sd(K, streaming)
    if not tmp:
        return Oracle('squeezeformer', sd, streaming, K)
    return _live('squeezeformer', sd, streaming, tmp, num_blocks=4, cnn_module_kernel=K, **SQZ_IDX)


def chunk_steps(m, rcs):
    """the three chunk steps of the 403-frame utterance -> (probabilities [3, 16, V], att cache, cnn cache)"""
    x = single_inputs()[403]
    att, cnn, off, chunks = torch.zeros(0, 0, 0, 0), torch.zeros(0, 0, 0, 0), 0, []
    for cur, n in CHUNKS:
        r, att, cnn = m.get_encoder_out_chunk(x[:1, cur:cur + n], off, rcs, att, cnn)
        off += r.shape[1]
        chunks.append(r[0].numpy())
    return np.stack(chunks), att.numpy(), cnn.numpy()


def _full(out, key, m, cases=('b3', 67, 403)):
    feats, lens = ragged_inputs()
    singles = single_inputs()
    for case in cases:
        if case == 'b3':
            out[f'{key}_b3'] = m.get_encoder_out(feats, lens).numpy()
        else:
            out[f'{key}_{case}'] = m.get_encoder_out(singles[case], torch.tensor([case])).numpy()


@torch.no_grad()
def record(tmp=None):
    """every record of the file: through the live reference when ``tmp`` (a scratch directory) is given, else through the oracle"""
    out = {}
    b = {True: 's', False: 'n'}
    for K, streaming in CONFORMER:
        _full(out, f'c{K}{b[streaming]}', conformer_model(K, streaming, tmp))
    for K, streaming in CONFORMER_BN:
        _full(out, f'cbn{K}{b[streaming]}', conformer_model(K, streaming, tmp, norm='batch_norm'), ('b3',))
    for K, rcs in CONFORMER_CHUNK:
        probs, att, cnn = chunk_steps(conformer_model(K, True, tmp), rcs)
        out[f'c{K}_chunk_{rcs}'] = probs
        if (K, rcs) == (8, 16):
            out['c8_chunk_att_16'], out['c8_chunk_cnn_16'] = att, cnn
    for K, streaming in WIDE:
        _full(out, f'w{K}{b[streaming]}', conformer_model(K, streaming, tmp, wide=True), ('b3', 67))
    out['w31_chunk_-1'] = chunk_steps(conformer_model(31, True, tmp, wide=True), -1)[0]
    for K, streaming in SQUEEZEFORMER:
        _full(out, f'q{K}{b[streaming]}', squeezeformer_model(K, streaming, tmp))
    for K in SQUEEZEFORMER_CHUNK:
        probs, _, cnn = chunk_steps(squeezeformer_model(K, True, tmp), -1)
        out[f'q{K}_chunk_-1'] = probs
        if K == 8:
            out['q8_chunk_cnn_-1'] = cnn
    return out


def main():
    assert shims.reference_available(), 'the reference checkout is needed'
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with tempfile.TemporaryDirectory() as tmp:
        np.savez_compressed(OUT, **record(tmp))
    print(OUT, os.path.getsize(OUT))
    assert os.path.getsize(OUT) <= LIMIT


if __name__ == '__main__':
    main()
