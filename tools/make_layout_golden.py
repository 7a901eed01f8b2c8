"""Record the layer-layout fixture of tests/test_gpu_layouts.py / tests/test_layouts_cpu.py from the REAL reference modules (imported
unmodified through oracle/shims) on CPU: ``python -m tools.make_layout_golden``.  Where the reference checkout is absent, ``record()``
goes through the oracle instead (as tools/make_conv_kernel_golden.py does), so that the CPU test can recompute the file on either
machine.

The layouts are the layer positions a checkpoint's YAML sets: the Squeezeformer's ``reduce_idx`` / ``recover_idx`` and the Efficient
Conformer's ``stride_layer_idx`` / leading ``group_layer_idx``, off the shipped ones.  Synthetic weights
(``synthetic.squeezeformer_state_dict(0, 50, num_blocks=L, streaming=...)``, ``synthetic.efficient_conformer_state_dict(0, 50,
num_blocks=L, stride_layer_idx=(s,), group_layer_idx=range(g))``), inputs from seeds.  ``layouts_v50.npz`` holds CTC probabilities
only, with ``<b>`` = ``s`` / ``n`` for streaming: True / False and ``<name>`` = ``name_of(layout)``:
  ``<name>_<b>_b3``       get_encoder_out of the ragged B = 3 batch of T = 139 feature frames
  ``<name>_s_chunks``     three 67-frame get_encoder_out_chunk steps (stride 64) of the 203-frame utterance, all history kept
  ``refused``             one line per layout that masr_create refuses: ``<name>|<what the reference does with it>``, where the
                          latter is ``error`` (its constructor or forward raises), ``frames <n>`` (it runs and gives n encoder frames
                          for the batch; the engine's contract is ``contract_frames``) -- see REFUSED below
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

OUT = os.path.join(ROOT, 'tests', 'golden', 'layouts_v50.npz')
V = 50
LIMIT = 1 << 20
T_BATCH = (139, 143)                       # T' = 34 / 35 behind conv2d: even and odd, T' mod 3 = 1 and 2
T_CHUNKED = 203
WINDOWS = [(0, 67), (64, 67), (128, 67), (192, 11)]
CHUNKS = WINDOWS[:3]                       # the fixture's chunk run (the GPU test adds the short last window)

# (family, L, a, b): squeezeformer a = reduce_idx, b = recover_idx (None = null); efficient_conformer a = stride layer, b = number of
# leading grouped layers
EFFICIENT = [('efficient_conformer', 4, 3, 4), ('efficient_conformer', 4, 0, 0), ('efficient_conformer', 4, 0, 1),
             ('efficient_conformer', 5, 2, 1), ('efficient_conformer', 5, 3, 2), ('efficient_conformer', 4, 2, 0)]
SQUEEZEFORMER = [('squeezeformer', 4, 0, 3), ('squeezeformer', 4, 1, 2), ('squeezeformer', 3, 1, 1), ('squeezeformer', 4, None, 3)]
LAYOUTS = EFFICIENT + SQUEEZEFORMER
# what masr_create refuses.  The first group fails in the reference itself or leaves it at a frame rate the engine's entry points
# exclude (the Efficient Conformer's output is at half the input layer's rate, the Squeezeformer's at the full one); the second group
# RUNS in the reference at the contract's rate -- an index that names no layer is ignored there, and grouped attention behind the
# stride layer is simply not implemented here -- and is refused all the same: the record says so, it is not hidden.
REFUSED = [('efficient_conformer', 4, -1, 0), ('efficient_conformer', 4, 4, 4), ('efficient_conformer', 4, 5, 0),
           ('squeezeformer', 4, -2, 3), ('squeezeformer', 4, 2, 1), ('squeezeformer', 4, 3, 0),
           ('squeezeformer', 4, 2, None), ('squeezeformer', 4, 2, 4)]
REFUSED_BUT_RUNS = [('efficient_conformer', 4, 1, 3), ('efficient_conformer', 4, 0, 2), ('squeezeformer', 4, 4, 5),
                    ('squeezeformer', 4, 7, 9)]


def name_of(layout):
    fam, L, a, b = layout
    n = (lambda v: 'null' if v is None else str(v))
    return f'q{L}_r{n(a)}_c{n(b)}' if fam == 'squeezeformer' else f'e{L}_s{n(a)}_g{n(b)}'


def state_dict(layout, streaming=True):
    fam, L, a, b = layout
    if fam == 'squeezeformer':
        return synthetic.squeezeformer_state_dict(0, V, num_blocks=L, streaming=streaming)
    # (a refused layout may name a layer that does not exist: the weights then are those of the layers that do)
    return synthetic.efficient_conformer_state_dict(0, V, num_blocks=L, stride_layer_idx=(a,), group_layer_idx=tuple(range(max(b, 0))))


def encoder_conf(layout):
    """the ``encoder_conf`` entries of the layout, as a YAML would hold them (HipEngine's argument)"""
    fam, L, a, b = layout
    if fam == 'squeezeformer':
        return {'encoder_dim': 256, 'attention_heads': 4, 'feed_forward_expansion_factor': 8, 'cnn_module_kernel': 31, 'num_blocks': L,
                'reduce_idx': a, 'recover_idx': b}
    return {'output_size': 256, 'attention_heads': 4, 'linear_units': 2048, 'cnn_module_kernel': 15, 'num_blocks': L,
            'efficient_conf': {'stride_layer_idx': [a], 'stride': [2], 'group_layer_idx': list(range(max(b, 0))), 'group_size': 3,
                               'stride_kernel': True}}


def oracle_kw(layout, streaming=None):
    """keywords of the oracle's ``get_encoder_out_chunk`` (``streaming=None``) or ``encoder_full`` / ``get_encoder_out``"""
    fam, L, a, b = layout
    if fam == 'squeezeformer':
        kw = {'reduce_idx': a, 'recover_idx': b}
        return kw if streaming is None else dict(kw, causal=streaming)
    kw = {'stride_layer_idx': (a,), 'group_layer_idx': tuple(range(max(b, 0)))}
    return kw if streaming is None else dict(kw, streaming=streaming)


def ragged_batch(T):
    """-> feats [3, T, 80] float32 (zero past each length), lens [3] int64; the longest utterance is full length"""
    rng = np.random.default_rng(1000 + T)
    lens = np.array([T, rng.integers(T // 2, T - 8), rng.integers(40, T // 2)], np.int64)
    feats = rng.standard_normal((3, T, 80)).astype(np.float32) * 3 + 13
    feats *= (np.arange(T)[None, :, None] < lens[:, None, None])
    return torch.from_numpy(feats), torch.from_numpy(lens)


def chunked_input():
    """-> [2, 203, 80] float32: the utterance of the chunk runs, and a second one for the stream that runs out of phase"""
    rng = np.random.default_rng(2000 + T_CHUNKED)
    return torch.from_numpy(rng.standard_normal((2, T_CHUNKED, 80)).astype(np.float32) * 3 + 13)


def contract_frames(layout, T=T_BATCH[0]):
    """encoder frames the engine's entry points give for T feature frames: conv2d's, halved with ceil for the Efficient Conformer"""
    t4 = ((T - 1) // 2 - 1) // 2
    return (t4 + 1) // 2 if layout[0] == 'efficient_conformer' else t4


def _live(layout, streaming, tmp):
    """the live reference model with the synthetic weights, in eval mode"""
    fam, L, a, b = layout
    shims.install()
    if fam == 'squeezeformer':
        from masr.model_utils.squeezeformer.model import SqueezeformerModel as M
    else:
        from masr.model_utils.efficient_conformer.model import EfficientConformerModel as M
    cfg = yaml.safe_load(open(os.path.join(shims.REFERENCE_ROOT, 'configs', fam + '.yml'), encoding='utf-8'))
    conf = cfg['encoder_conf']
    conf['num_blocks'] = L
    if fam == 'squeezeformer':
        conf.update(reduce_idx=a, recover_idx=b)
    else:           # (the nested efficient_conf is swallowed by **kwargs in the reference: its constructor takes the entries themselves)
        conf.pop('efficient_conf', None)
        conf.update(stride_layer_idx=[a], stride=[2], group_layer_idx=list(range(max(b, 0))), group_size=3, stride_kernel=True)
    sd = state_dict(layout, streaming)
    p = os.path.join(tmp, 'mean_istd.json')
    json.dump({'mean': sd['encoder.global_cmvn.mean'].tolist(), 'istd': sd['encoder.global_cmvn.istd'].tolist(),
               'feature_method': 'fbank'}, open(p, 'w'))
    torch.manual_seed(0)
    m = M(input_dim=80, vocab_size=V, mean_istd_path=p, streaming=streaming, encoder_conf=conf, decoder_conf=cfg['decoder_conf'],
          **cfg['model_conf'])
    missing, unexpected = m.load_state_dict(sd, strict=False)
    # (the attention decoder is not part of the synthetic weights and not of get_encoder_out*)
    missing = [k for k in missing if not k.startswith('decoder.') and 'concat_linear' not in k]
    assert not unexpected and not missing, (missing, unexpected)
    return m.eval()


class Oracle:
    """the reference's two entry points through the oracle (where the reference checkout is absent)"""

    def __init__(self, layout, streaming):
        from oracle import f64
        self.m, self.sd = f64.module_of(layout[0]), state_dict(layout, streaming)
        self.full, self.chunk = oracle_kw(layout, streaming), oracle_kw(layout)

    def get_encoder_out(self, feats, lens):
        return self.m.get_encoder_out(self.sd, feats, lens, **self.full)

    def get_encoder_out_chunk(self, x, off, rcs, att, cnn):
        return self.m.get_encoder_out_chunk(self.sd, x, off, rcs, att, cnn, **self.chunk)


def model(layout, streaming, tmp=None):
    return _live(layout, streaming, tmp) if tmp else Oracle(layout, streaming)


def chunk_steps(m, windows=CHUNKS, rcs=-1):
    """the chunk steps of the 203-frame utterance -> probabilities of all chunks concatenated [T', V]"""
    x = chunked_input()
    att, cnn, off, chunks = torch.zeros(0, 0, 0, 0), torch.zeros(0, 0, 0, 0), 0, []
    for cur, n in windows:
        r, att, cnn = m.get_encoder_out_chunk(x[:1, cur:cur + n], off, rcs, att, cnn)
        off += r.shape[1]
        chunks.append(r[0].numpy())
    return np.concatenate(chunks)


def outcome(layout, tmp=None):
    """what the reference does with a layout on the T = 139 batch: 'error' or 'frames <n>'"""
    feats, lens = ragged_batch(T_BATCH[0])
    try:
        return f'frames {model(layout, True, tmp).get_encoder_out(feats, lens).shape[1]}'
    except Exception:
        return 'error'


@torch.no_grad()
def record(tmp=None):
    """every record of the file: through the live reference when ``tmp`` (a scratch directory) is given, else through the oracle"""
    out = {}
    feats, lens = ragged_batch(T_BATCH[0])
    for layout in LAYOUTS:
        for streaming in (True, False):
            m = model(layout, streaming, tmp)
            out[f'{name_of(layout)}_{"s" if streaming else "n"}_b3'] = m.get_encoder_out(feats, lens).numpy()
            if streaming:
                out[f'{name_of(layout)}_s_chunks'] = chunk_steps(m)
    out['refused'] = np.array([f'{name_of(l)}|{outcome(l, tmp)}' for l in REFUSED + REFUSED_BUT_RUNS])
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
