"""Record the conv2d6 / conv2d8 fixtures of tests/test_gpu_input_layers.py from the REAL reference modules (imported unmodified
through oracle/shims) on CPU.  Runs only where the reference checkout exists:  ``python -m tools.make_input_layer_golden``.

Synthetic weights (masr_amd.utils.synthetic, seed 0, V = 512) and seeded features; every record is a function of its inputs so
that the CPU test can recompute it next to the committed file.
* ``conformer_<il>_v512.npz``      ConformerModel (configs/conformer.yml, streaming: True, input_layer = il): get_encoder_out
                                   probs and encoder output of a ragged B = 3 batch (one utterance at the minimum frame count),
                                   the chunk-4 masked encoder output, and get_encoder_out_chunk over the facade's 67 / 64 windows.
* ``conformer_<il>_nonstreaming_v512.npz``  the same with streaming: False (probs and encoder output).
* ``efficient_conformer_conv2d8_v512.npz``   EfficientConformerModel (configs/efficient_conformer.yml, input_layer conv2d8):
                                   probs and encoder output of the ragged batch.
* ``predictor_conv2d8.npz``        reference MASRPredictor(use_gpu=False) on the TorchScript export of a conv2d8 Conformer
                                   (V = 4233, use_dB_normalization: False): predict and every predict_stream partial of
                                   dataset/test.wav.
"""
import json
import os
import sys
import tempfile
import wave

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import shims                   # noqa: E402
from masr_amd.utils import synthetic      # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
MIN_FRAMES = {'conv2d6': 11, 'conv2d8': 15}
T_IN = 331


def inputs(il):
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(3, T_IN, 80, generator=g) * 3 + 13
    lens = torch.tensor([T_IN, 200, MIN_FRAMES[il]])
    return feats * (torch.arange(T_IN)[None, :, None] < lens[:, None, None]), lens


def _mean_istd(sd, tmp):
    p = os.path.join(tmp, 'mean_istd.json')
    json.dump({'mean': sd['encoder.global_cmvn.mean'].tolist(), 'istd': sd['encoder.global_cmvn.istd'].tolist(),
               'feature_method': 'fbank'}, open(p, 'w'))
    return p


def _model(kind, il, vocab, streaming, tmp):
    shims.install()
    ref = shims.REFERENCE_ROOT
    if kind == 'conformer':
        from masr.model_utils.conformer.model import ConformerModel as M
        sd = synthetic.conformer_state_dict(0, vocab, input_layer=il)
    else:
        from masr.model_utils.efficient_conformer.model import EfficientConformerModel as M
        sd = synthetic.efficient_conformer_state_dict(0, vocab, input_layer=il)
    cfg = yaml.safe_load(open(os.path.join(ref, 'configs', kind + '.yml'), encoding='utf-8'))
    cfg['encoder_conf']['input_layer'] = il
    mean_istd = _mean_istd(sd, tmp)
    torch.manual_seed(0)
    m = M(input_dim=80, vocab_size=vocab, mean_istd_path=mean_istd, streaming=streaming, encoder_conf=cfg['encoder_conf'],
          decoder_conf=cfg['decoder_conf'], **cfg['model_conf'])
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith('decoder.') or 'concat_linear' in k for k in missing), (missing, unexpected)
    return m.eval(), cfg, mean_istd


def windows(T):
    """the facade's windows over T frames with is_end (predict.py:283-306): 67 frames every 64, the last at least 7"""
    return [(cur, min(cur + 67, T)) for cur in range(0, T - 7 + 1, 64)]


@torch.no_grad()
def conformer_record(il, streaming, tmp):
    m, _, _ = _model('conformer', il, 512, streaming, tmp)
    feats, lens = inputs(il)
    enc, _ = m.encoder(feats, lens, -1, -1)
    rec = {'feats': feats.numpy(), 'lens': lens.numpy().astype(np.int32), 'enc': enc.numpy(),
           'probs': m.get_encoder_out(feats, lens).numpy()}
    if streaming:
        rec['enc4'] = m.encoder(feats, lens, 4, -1)[0].numpy()
        att, cnn, off, probs, spans = torch.zeros(0, 0, 0, 0), torch.zeros(0, 0, 0, 0), 0, [], []
        from masr_amd.engine import subsampled_len
        for a, b in windows(T_IN):
            if subsampled_len(b - a, il) <= 0:          # the reference's conv refuses a window below the minimum
                continue
            r, att, cnn = m.get_encoder_out_chunk(feats[:1, a:b], off, -16, att, cnn)
            off += r.shape[1]
            probs.append(r[0].numpy())
            spans.append((a, b))
        rec['chunk_probs'] = np.concatenate(probs)
        rec['chunk_spans'] = np.array(spans, np.int32)
    return rec


@torch.no_grad()
def efficient_record(il, tmp):
    m, _, _ = _model('efficient_conformer', il, 512, True, tmp)
    feats, lens = inputs(il)
    enc, _ = m.encoder(feats, lens, -1, -1)
    return {'feats': feats.numpy(), 'lens': lens.numpy().astype(np.int32), 'enc': enc.numpy(),
            'probs': m.get_encoder_out(feats, lens).numpy()}


def test_pcm():
    w = wave.open(os.path.join(shims.REFERENCE_ROOT, 'dataset', 'test.wav'))
    return np.frombuffer(w.readframes(w.getnframes()), np.int16).copy()


def facade_record(tmp):
    from masr.predict import MASRPredictor
    from oracle.make_golden import record_facade
    m, cfg, mean_istd = _model('conformer', 'conv2d8', 4233, True, tmp)
    vpath = os.path.join(tmp, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(4233):
            f.write(f'{t}\t1\n')
    mdir = os.path.join(tmp, 'models', 'conformer_conv2d8')
    os.makedirs(mdir, exist_ok=True)
    torch.jit.save(m.export(), os.path.join(mdir, 'inference.pt'))
    cfg['dataset_conf']['dataset_vocab'] = vpath
    cfg['dataset_conf']['mean_istd_path'] = mean_istd
    cfg['decoder'] = 'ctc_greedy'
    cfg['preprocess_conf']['use_dB_normalization'] = False
    pred = MASRPredictor(configs=cfg, model_path=os.path.join(mdir, 'inference.pt'), use_gpu=False)
    return record_facade(pred, test_pcm())


def main():
    assert shims.reference_available(), 'the reference checkout is needed'
    with tempfile.TemporaryDirectory() as tmp:
        for il in ('conv2d6', 'conv2d8'):
            np.savez_compressed(os.path.join(OUT, f'conformer_{il}_v512.npz'), **conformer_record(il, True, tmp))
            np.savez_compressed(os.path.join(OUT, f'conformer_{il}_nonstreaming_v512.npz'), **conformer_record(il, False, tmp))
        np.savez_compressed(os.path.join(OUT, 'efficient_conformer_conv2d8_v512.npz'), **efficient_record('conv2d8', tmp))
        np.savez_compressed(os.path.join(OUT, 'predictor_conv2d8.npz'), **facade_record(tmp))
    for f in sorted(os.listdir(OUT)):
        if 'conv2d' in f:
            print(' ', f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == '__main__':
    main()
