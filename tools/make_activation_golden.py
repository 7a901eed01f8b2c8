"""Record the ``activation_type`` Conformer fixture of tests/test_gpu_activation.py from the REAL reference modules (imported
unmodified through oracle/shims) on CPU, built once per activation.  Runs only where the reference checkout exists:
``python -m tools.make_activation_golden``.

Synthetic weights (masr_amd.utils.synthetic.conformer_state_dict(0, 50, num_blocks=2): an activation has no weights, so every
activation reads the same checkpoint); every record is a function of seeds, so that the CPU test can recompute it next to the
committed file -- through the live reference, or through the restatement tests/activation_ref.py where the checkout is absent.

Like tools/make_abs_pos_golden.py the float64 record of a key is stored as its distance from the float32 one,

    ``<key>``       the float32 output
    ``<key>__d64``  float32(y64 - y32)            truth = float64(<key>) + float64(<key>__d64)

taken from the same live model after ``model.double()``.  Forty ragged-batch records in float32 alone are 0.75 MiB, so the
distances are kept where they pin the most for their bytes -- the probabilities of the ragged batch of the ten 256 / 4 builds and
of the 67-frame utterance; the GPU tests take their float64 truth from tests/activation_ref.py, which
tests/test_activation_cpu.py holds against these distances.

``conformer_activation_v50.npz``, keys ``<act>_<width>_<s|n>_*`` (act relu / gelu / tanh / hardtanh / selu, width 256 / 512,
streaming: True / False):
  ``*_b3_probs``, ``*_b3_enc``     get_encoder_out of the ragged B = 3 batch (lens 131 / 99 / 67) and a probe of the encoder output
                                   (every 8th column)
  ``*_256_s_single_probs_67``      one utterance of 67 frames (T' = 16)
  ``*_256_s_single_probs_403``     one utterance of 403 frames (T' = 100), relu and gelu
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

OUT = os.path.join(ROOT, 'tests', 'golden', 'conformer_activation_v50.npz')
V, BLOCKS = 50, 2
WIDTHS = {256: 4, 512: 8}                  # output_size -> attention_heads
ACTS = ('relu', 'gelu', 'tanh', 'hardtanh', 'selu')
LONG_ACTS = ('relu', 'gelu')               # the activations recorded on the 403-frame utterance
LENS = (131, 99, 67)
SINGLE_T = (67, 403)
PROBE = 8                                  # the encoder probe keeps every 8th column
LIMIT = 1 << 20
D64 = '__d64'


def builds():
    """(act, width, streaming) of every recorded build"""
    return [(a, w, s) for a in ACTS for w in WIDTHS for s in (True, False)]


def prefix(act, width, streaming):
    return f'{act}_{width}_{"s" if streaming else "n"}_'


def names_of(act, width, streaming):
    """(record names of a build, those that carry a float64 distance)"""
    names = ['b3_probs', 'b3_enc']
    d64 = ['b3_probs'] if width == 256 else []
    if width == 256 and streaming:
        names += ['single_probs_67'] + (['single_probs_403'] if act in LONG_ACTS else [])
        d64 += ['single_probs_67']
    return names, d64


def state_dict(width):
    return synthetic.conformer_state_dict(0, V, d=width, heads=WIDTHS[width], num_blocks=BLOCKS)


def encoder_conf(act, width):
    return {'output_size': width, 'attention_heads': WIDTHS[width], 'num_blocks': BLOCKS, 'activation_type': act}


def ragged_inputs():
    """-> feats [3, 131, 80] float32 (zero past each length), lens [3] int64"""
    rng = np.random.default_rng(21)
    feats = rng.standard_normal((len(LENS), max(LENS), 80)).astype(np.float32) * 3 + 13
    lens = np.array(LENS, np.int64)
    feats *= (np.arange(max(LENS))[None, :, None] < lens[:, None, None])
    return torch.from_numpy(feats), torch.from_numpy(lens)


def single_inputs():
    """{T: [1, T, 80] float32}, drawn in the order of SINGLE_T from one generator"""
    rng = np.random.default_rng(22)
    return {T: torch.from_numpy(rng.standard_normal((1, T, 80)).astype(np.float32) * 3 + 13) for T in SINGLE_T}


def model(act, width, streaming, tmp):
    """the live reference ConformerModel built with ``activation_type: act`` and the synthetic weights, in eval mode (float32)"""
    shims.install()
    from masr.model_utils.conformer.model import ConformerModel as M
    cfg = yaml.safe_load(open(os.path.join(shims.REFERENCE_ROOT, 'configs', 'conformer.yml'), encoding='utf-8'))
    cfg['encoder_conf'].update(encoder_conf(act, width))
    sd = state_dict(width)
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
    layer = m.encoder.encoders[0]
    want = {'relu': 'ReLU', 'gelu': 'GELU', 'tanh': 'Tanh', 'hardtanh': 'Hardtanh', 'selu': 'SELU', 'swish': 'Swish'}[act]
    for mod in (layer.feed_forward.activation, layer.feed_forward_macaron.activation, layer.conv_module.activation):
        assert type(mod).__name__ == want, (act, type(mod).__name__)
    return m.eval()


class RefModel:
    """the entry points the records need through tests/activation_ref.py (where the reference checkout is absent)"""

    def __init__(self, act, width, streaming):
        from oracle.f64 import cast_state_dict
        from tests import activation_ref as ar
        self.ar, self.cast, self.sd = ar, cast_state_dict, state_dict(width)
        self.kw = dict(act=act, heads=WIDTHS[width], streaming=streaming)

    def double(self):
        self.sd = self.cast(self.sd, torch.float64)
        return self

    def get_encoder_out(self, feats, lens):
        return self.ar.get_encoder_out(self.sd, feats, lens, **self.kw)

    def encoder_out(self, feats, lens):
        return self.ar.encoder_full(self.sd, feats, lens, **self.kw)


def encoder_out(m, feats, lens):
    return m.encoder_out(feats, lens) if isinstance(m, RefModel) else m.encoder(feats, lens, -1, -1)[0]


@torch.no_grad()
def record_of(m, act, width, streaming):
    """the records of one build from a model with the reference's entry points: float32, and the float64 distance where kept"""
    k = prefix(act, width, streaming)
    names, d64 = names_of(act, width, streaming)
    runs = {}
    for dt in (torch.float32, torch.float64):
        mm = m if dt == torch.float32 else m.double()          # (float32 first: .double() converts the model in place)
        if dt == torch.float64 and not isinstance(m, RefModel):
            # the positional table is a plain attribute (conformer/embedding.py:31), which .double() leaves alone: the float32
            # table cast to float64, the one oracle.conformer.positional_table hands out in float64
            pe = mm.encoder.embed.pos_enc
            pe.pe = pe.pe.double()
        want = names if dt == torch.float32 else d64
        r = {}
        feats, lens = ragged_inputs()
        feats = feats.to(dt)
        if 'b3_probs' in want:
            r['b3_probs'] = mm.get_encoder_out(feats, lens)
        if 'b3_enc' in want:
            r['b3_enc'] = encoder_out(mm, feats, lens)[:, :, ::PROBE]
        for T, x in single_inputs().items():
            if f'single_probs_{T}' in want:
                r[f'single_probs_{T}'] = mm.get_encoder_out(x.to(dt), torch.tensor([T]))
        runs[dt] = r
    out = {}
    for name, y32 in runs[torch.float32].items():
        assert y32.dtype == torch.float32, (name, y32.dtype)
        out[k + name] = np.ascontiguousarray(y32.numpy())
        if name in runs[torch.float64]:
            y64 = runs[torch.float64][name]
            assert y64.dtype == torch.float64 and y64.shape == y32.shape, (name, y64.dtype)
            out[k + name + D64] = np.ascontiguousarray((y64 - y32.double()).float().numpy())
    return out


def truth(z, key):
    """the float64 record of ``key`` from a loaded file or a record dict"""
    return np.asarray(z[key], np.float64) + np.asarray(z[key + D64], np.float64)


def record(tmp=None, only=None):
    """every record of the file (or of the builds ``only``): through the live reference when ``tmp`` (a scratch directory) is
    given, else through tests/activation_ref.py"""
    out = {}
    for act, width, streaming in builds():
        if only is None or (act, width, streaming) in only:
            m = model(act, width, streaming, tmp) if tmp else RefModel(act, width, streaming)
            out.update(record_of(m, act, width, streaming))
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
