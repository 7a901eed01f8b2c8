"""Record the ``pos_enc_layer_type: abs_pos`` / ``no_pos`` Conformer fixture of tests/test_gpu_abs_pos.py from the REAL reference
modules (imported unmodified through oracle/shims) on CPU.  Runs only where the reference checkout exists:
``python -m tools.make_abs_pos_golden``.

Synthetic weights (masr_amd.utils.synthetic.conformer_state_dict(0, 50, num_blocks=2, pos_enc_layer_type=...)); every record is a
function of seeds, so that the CPU test can recompute it next to the committed file.  There is no oracle restatement of these two
modes, so every record is taken TWICE from the same live model: in float32, and after ``model.double()`` on float64 inputs -- the
truth of the budget rule (tests/budget.py).  The float64 record is stored as its distance from the float32 one,

    ``<key>``       the float32 output
    ``<key>__d64``  float32(y64 - y32)            truth = float64(<key>) + float64(<key>__d64)

which keeps the truth to 2^-24 of the reference's own error (about 1e-14 absolute here) at half the bytes of a float64 array.

``conformer_abs_pos_v50.npz``, keys ``<mode>_<width>_<s|n>_*`` (mode abs / no, width 256 / 512, streaming: True / False):
  ``*_b3_probs``, ``*_b3_enc``     get_encoder_out of the ragged B = 3 batch (lens 131 / 99 / 67) and a probe of the encoder output
                                   (every 8th column)
  ``*_single_probs_<T>``           one utterance of T = 67 / 403 frames (width 256)
  ``*_s_chunk_probs_<r>``, ``*_s_chunk_att_<r>``, ``*_s_chunk_cnn_<r>``    three 67-frame get_encoder_out_chunk steps (stride 64) of the
                                   403-frame utterance with required_cache_size r = -1 / 16: probabilities per chunk in full; the
                                   final caches in float32 only, as probes (att: every 8th column of [L, H, t, 2 dk] -- key and
                                   value halves alike; cnn: every 4th channel of [L, 1, d, 14])
Width 512 / 8 carries abs_pos only: the ragged batch of both builds and the chunk steps.

``no_pos``: the reference's NoPositionalEncoding (conformer/embedding.py:104-117) never sets the ``d_model`` and ``dropout`` that
its ``forward`` reads (its ``__init__`` only calls ``nn.Module.__init__``), so the class as shipped raises AttributeError on its
first call.  ``model()`` sets those two attributes on the INSTANCE (``d_model`` = output_size, ``dropout`` = the identity in eval
mode); the class's own ``forward`` then runs as written: x unscaled, a zero ``pos_emb`` that plain attention ignores.
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

OUT = os.path.join(ROOT, 'tests', 'golden', 'conformer_abs_pos_v50.npz')
V, BLOCKS = 50, 2
WIDTHS = {256: 4, 512: 8}                  # output_size -> attention_heads
MODES = {'abs': 'abs_pos', 'no': 'no_pos'}
LENS = (131, 99, 67)
SINGLE_T = (67, 403)
CHUNKS = [(0, 67), (64, 67), (128, 67)]
CACHE_SIZES = (-1, 16)
PROBE = 8                                  # the encoder and att-cache probes keep every 8th column
CNN_PROBE = 4                              # the cnn-cache probe keeps every 4th channel
LIMIT = 1 << 20
D64 = '__d64'


def builds():
    """(mode, width, streaming) of every recorded build: both modes and both builds at 256 / 4, abs_pos alone at 512 / 8"""
    return [(m, 256, s) for m in MODES for s in (True, False)] + [('abs', 512, s) for s in (True, False)]


def prefix(mode, width, streaming):
    return f'{mode}_{width}_{"s" if streaming else "n"}_'


def state_dict(mode, width):
    return synthetic.conformer_state_dict(0, V, d=width, heads=WIDTHS[width], num_blocks=BLOCKS, pos_enc_layer_type=MODES[mode])


def encoder_conf(mode, width):
    return {'output_size': width, 'attention_heads': WIDTHS[width], 'num_blocks': BLOCKS, 'pos_enc_layer_type': MODES[mode]}


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


def model(mode, width, streaming, tmp):
    """the live reference ConformerModel with the synthetic weights, in eval mode (float32)"""
    shims.install()
    from masr.model_utils.conformer.model import ConformerModel as M
    cfg = yaml.safe_load(open(os.path.join(shims.REFERENCE_ROOT, 'configs', 'conformer.yml'), encoding='utf-8'))
    cfg['encoder_conf'].update(encoder_conf(mode, width))
    sd = state_dict(mode, width)
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
    assert not any('linear_pos' in k or 'pos_bias' in k for k in m.state_dict()), 'plain attention expected'
    if mode == 'no':            # what NoPositionalEncoding.__init__ leaves out (see the module docstring)
        pe = m.encoder.embed.pos_enc
        assert type(pe).__name__ == 'NoPositionalEncoding' and not hasattr(pe, 'd_model')
        pe.d_model = width
        pe.dropout = torch.nn.Identity()
    return m.eval()


@torch.no_grad()
def record_of(m, mode, width, streaming):
    """the records of one build from the live model, every output in float32 and as its float64 distance"""
    k = prefix(mode, width, streaming)
    runs = {}
    for dt in (torch.float32, torch.float64):
        mm = m if dt == torch.float32 else m.double()          # (float32 first: .double() converts the model in place)
        r = {}
        feats, lens = ragged_inputs()
        feats = feats.to(dt)
        r['b3_probs'] = mm.get_encoder_out(feats, lens)
        r['b3_enc'] = mm.encoder(feats, lens, -1, -1)[0][:, :, ::PROBE]
        singles = {T: x.to(dt) for T, x in single_inputs().items()}
        if width == 256:
            for T, x in singles.items():
                r[f'single_probs_{T}'] = mm.get_encoder_out(x, torch.tensor([T]))
        if streaming:
            x = singles[403]
            for rcs in CACHE_SIZES:
                att, cnn, off, chunks = torch.zeros(0, 0, 0, 0, dtype=dt), torch.zeros(0, 0, 0, 0, dtype=dt), 0, []
                for cur, n in CHUNKS:
                    o, att, cnn = mm.get_encoder_out_chunk(x[:1, cur:cur + n], off, rcs, att, cnn)
                    off += o.shape[1]
                    chunks.append(o[0])
                r[f'chunk_probs_{rcs}'] = torch.stack(chunks)
                if dt == torch.float32:
                    r[f'chunk_att_{rcs}'] = att[..., ::PROBE]
                    r[f'chunk_cnn_{rcs}'] = cnn[:, :, ::CNN_PROBE]
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


def record(tmp, only=None):
    """every record of the file (or of the builds ``only``) through the live reference; ``tmp``: a scratch directory"""
    out = {}
    for mode, width, streaming in builds():
        if only is None or (mode, width, streaming) in only:
            out.update(record_of(model(mode, width, streaming, tmp), mode, width, streaming))
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
