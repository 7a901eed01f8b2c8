"""Record the ``output_size: 512, attention_heads: 8`` Conformer fixture of tests/test_gpu_wide.py from the REAL reference modules
(imported unmodified through oracle/shims) on CPU.  Runs only where the reference checkout exists:
``python -m tools.make_wide_golden``.

Synthetic weights (masr_amd.utils.synthetic.conformer_state_dict(0, 50, d=512, heads=8, num_blocks=2)); every record is a function
of seeds, so that the CPU test can recompute it next to the committed file.  ``conformer_wide_v50.npz``, keys ``<s|n>_*`` for
streaming: True / False:
  ``*_b3_probs``, ``*_b3_enc``     get_encoder_out of the ragged B = 3 batch of ``ragged_inputs()`` (lens 131 / 99 / 67) and a probe of
                                   the encoder output (every 8th column)
  ``*_single_probs_<T>``           one utterance of T = 67 / 403 frames (``single_inputs()``)
  ``s_chunk_probs_<r>``, ``s_chunk_att_<r>``, ``s_chunk_cnn_<r>``    three 67-frame get_encoder_out_chunk steps (stride 64) of the
                                   403-frame utterance with required_cache_size r = -1 / 16: probabilities per chunk, final caches
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

OUT = os.path.join(ROOT, 'tests', 'golden', 'conformer_wide_v50.npz')
V, D, HEADS, BLOCKS = 50, 512, 8, 2
LENS = (131, 99, 67)
SINGLE_T = (67, 403)
CHUNKS = [(0, 67), (64, 67), (128, 67)]
CACHE_SIZES = (-1, 16)
PROBE = 8                                  # the encoder probe keeps every 8th column
LIMIT = 1 << 20


def state_dict(**kw):
    return synthetic.conformer_state_dict(0, V, d=D, heads=HEADS, num_blocks=BLOCKS, **kw)


def ragged_inputs():
    """-> feats [3, 131, 80] float32 (zero past each length), lens [3] int64"""
    rng = np.random.default_rng(11)
    feats = rng.standard_normal((len(LENS), max(LENS), 80)).astype(np.float32) * 3 + 13
    lens = np.array(LENS, np.int64)
    feats *= (np.arange(max(LENS))[None, :, None] < lens[:, None, None])
    return torch.from_numpy(feats), torch.from_numpy(lens)


def single_inputs():
    """{T: [1, T, 80] float32}, drawn in the order of SINGLE_T from one generator"""
    rng = np.random.default_rng(12)
    return {T: torch.from_numpy(rng.standard_normal((1, T, 80)).astype(np.float32) * 3 + 13) for T in SINGLE_T}


def model(streaming, tmp):
    """the live reference ConformerModel at 512 / 8 with the synthetic weights, in eval mode"""
    shims.install()
    from masr.model_utils.conformer.model import ConformerModel as M
    cfg = yaml.safe_load(open(os.path.join(shims.REFERENCE_ROOT, 'configs', 'conformer.yml'), encoding='utf-8'))
    cfg['encoder_conf'].update(output_size=D, attention_heads=HEADS, num_blocks=BLOCKS)
    sd = state_dict()
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


class OracleModel:
    """the same three entry points through oracle.conformer with heads = 8 (where the reference checkout is absent)"""

    def __init__(self, streaming):
        from oracle import conformer as oc
        self.oc, self.sd, self.streaming = oc, state_dict(), streaming

    def get_encoder_out(self, feats, lens):
        return self.oc.get_encoder_out(self.sd, feats, lens, heads=HEADS, streaming=self.streaming)

    def encoder_out(self, feats, lens):
        return self.oc.encoder_full(self.sd, feats, lens, -1, heads=HEADS, streaming=self.streaming)

    def get_encoder_out_chunk(self, x, off, rcs, att, cnn):
        return self.oc.get_encoder_out_chunk(self.sd, x, off, rcs, att, cnn, heads=HEADS)


def encoder_out(m, feats, lens):
    return m.encoder_out(feats, lens) if isinstance(m, OracleModel) else m.encoder(feats, lens, -1, -1)[0]


@torch.no_grad()
def record_of(m, streaming):
    """the records of one build (streaming True / False) from a model with the reference's entry points"""
    k = 's_' if streaming else 'n_'
    out = {}
    feats, lens = ragged_inputs()
    out[k + 'b3_probs'] = m.get_encoder_out(feats, lens).numpy()
    out[k + 'b3_enc'] = np.ascontiguousarray(encoder_out(m, feats, lens).numpy()[:, :, ::PROBE])
    singles = single_inputs()
    for T, x in singles.items():
        out[k + f'single_probs_{T}'] = m.get_encoder_out(x, torch.tensor([T])).numpy()
    if streaming:
        x = singles[403]
        for rcs in CACHE_SIZES:
            att, cnn, off, chunks = torch.zeros(0, 0, 0, 0), torch.zeros(0, 0, 0, 0), 0, []
            for cur, n in CHUNKS:
                r, att, cnn = m.get_encoder_out_chunk(x[:1, cur:cur + n], off, rcs, att, cnn)
                off += r.shape[1]
                chunks.append(r[0].numpy())
            out[f's_chunk_probs_{rcs}'] = np.stack(chunks)
            out[f's_chunk_att_{rcs}'] = att.numpy()
            out[f's_chunk_cnn_{rcs}'] = cnn.numpy()
    return out


def record(tmp=None):
    """every record of the file: through the live reference when ``tmp`` (a scratch directory) is given, else through the oracle"""
    out = {}
    for streaming in (True, False):
        out.update(record_of(model(streaming, tmp) if tmp else OracleModel(streaming), streaming))
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
