"""Record the DeepSpeech2 ``rnn_size`` fixtures of tests/test_gpu_ds2_rnn_size.py from the REAL reference modules (imported
unmodified through oracle/shims) on CPU.  Runs only where the reference checkout exists:
``python -m tools.make_ds2_rnn_size_golden``.

Synthetic weights (masr_amd.utils.synthetic, seed 0) and the seeded ragged batch of ``oracle.make_golden.golden_inputs()``.
* ``deepspeech2_rnn_sizes.npz``         DeepSpeech2Model (configs/deepspeech2.yml with rnn_size / use_gru / num_rnn_layers replaced),
                                        V = 50, 2 layers, for (rnn_size 768, LSTM) and (rnn_size 2048, GRU): get_encoder_out of the
                                        bi-directional (streaming: False) and uni-directional (streaming: True) models on the ragged
                                        B = 3 batch, and a 5-chunk get_encoder_out_chunk run of the uni model with its final h / c.
                                        Keys are ``h<rnn_size>_<cell>_<record>``.
* ``predictor_deepspeech2_h512.npz``    reference MASRPredictor(use_gpu=False) on the TorchScript export of the rnn_size 512 LSTM
                                        models (5 layers, V = 4233): predict(test.wav) for bi and uni and every predict_stream partial.
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
CASES = ((768, False), (2048, True))       # (rnn_size, use_gru)


def _model(vocab, streaming, tmp, rnn_size, use_gru, layers):
    shims.install()
    from masr.model_utils.deepspeech2.model import DeepSpeech2Model
    sd = synthetic.deepspeech2_state_dict(0, vocab, rnn_size=rnn_size, num_rnn_layers=layers, bidirectional=not streaming,
                                          use_gru=use_gru)
    cfg = yaml.safe_load(open(os.path.join(shims.REFERENCE_ROOT, 'configs', 'deepspeech2.yml'), encoding='utf-8'))
    cfg['encoder_conf'].update(rnn_size=rnn_size, use_gru=use_gru, num_rnn_layers=layers)
    mean_istd = os.path.join(tmp, f'mean_istd_ds2_h{rnn_size}.json')
    json.dump({'mean': sd['encoder.global_cmvn.mean'].tolist(), 'istd': sd['encoder.global_cmvn.istd'].tolist(),
               'feature_method': 'fbank'}, open(mean_istd, 'w'))
    m = DeepSpeech2Model(input_dim=80, vocab_size=vocab, mean_istd_path=mean_istd, streaming=streaming,
                         encoder_conf=cfg['encoder_conf'], decoder_conf=cfg['decoder_conf'])
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    return m.eval(), cfg, mean_istd


@torch.no_grad()
def encoder_record(tmp):
    from oracle.make_golden import golden_inputs
    feats, lens = golden_inputs()
    out = {}
    for rnn_size, use_gru in CASES:
        k = f'h{rnn_size}_{"gru" if use_gru else "lstm"}_'
        m, _, _ = _model(50, False, tmp, rnn_size, use_gru, 2)
        out[k + 'bi_probs'] = m.get_encoder_out(feats, lens).numpy()
        m, _, _ = _model(50, True, tmp, rnn_size, use_gru, 2)
        out[k + 'uni_probs'] = m.get_encoder_out(feats, lens).numpy()
        h, c, chunks = torch.zeros(0, 0, 0, 0), torch.zeros(0, 0, 0, 0), []
        for cur in range(0, feats.shape[1] - 67 + 1, 64):
            x = feats[:1, cur:cur + 67]
            r, _, h, c = m.get_encoder_out_chunk(x, torch.tensor([x.shape[1]]), h, c)
            chunks.append(r[0].numpy())
        out[k + 'chunk_probs'] = np.stack(chunks)
        out[k + 'h'] = h.numpy()
        out[k + 'c'] = c.numpy()
    return out


def facade_record(tmp):
    from masr.predict import MASRPredictor
    w = wave.open(os.path.join(shims.REFERENCE_ROOT, 'dataset', 'test.wav'))
    pcm = np.frombuffer(w.readframes(w.getnframes()), np.int16).copy()
    vpath = os.path.join(tmp, 'vocabulary_ds2_h512.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(4233):
            f.write(f'{t}\t1\n')
    res = {}
    for streaming in (False, True):
        m, cfg, mean_istd = _model(4233, streaming, tmp, 512, False, 5)
        mdir = os.path.join(tmp, 'models', f'deepspeech2_h512_{streaming}')
        os.makedirs(mdir)
        torch.jit.save(m.export(), os.path.join(mdir, 'inference.pt'))
        cfg['dataset_conf']['dataset_vocab'] = vpath
        cfg['dataset_conf']['mean_istd_path'] = mean_istd
        cfg['decoder'] = 'ctc_greedy'
        cfg['streaming'] = streaming
        pred = MASRPredictor(configs=cfg, model_path=os.path.join(mdir, 'inference.pt'), use_gpu=False)
        r = pred.predict(audio_data=pcm.copy())
        key = 'uni' if streaming else 'bi'
        res[key + '_text'] = np.array(r['text'])
        res[key + '_score'] = np.array(r['score'], np.float64)
        if streaming:
            texts, scores, valid = [], [], []
            for s0 in range(0, len(pcm), 8000):
                q = pred.predict_stream(audio_data=pcm[s0:s0 + 8000].tobytes(), is_end=(s0 + 8000 >= len(pcm)))
                valid.append(q is not None and q['text'] is not None)
                texts.append('' if not valid[-1] else q['text'])
                scores.append(0.0 if not valid[-1] else float(q['score']))
            pred.reset_stream()
            res['stream_text'], res['stream_score'], res['stream_valid'] = np.array(texts), np.array(scores), np.array(valid)
    return res


def main():
    assert shims.reference_available(), 'the reference checkout is needed'
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with tempfile.TemporaryDirectory() as tmp:
        np.savez_compressed(os.path.join(OUT, 'deepspeech2_rnn_sizes.npz'), **encoder_record(tmp))
        res = facade_record(tmp)
        np.savez_compressed(os.path.join(OUT, 'predictor_deepspeech2_h512.npz'), **res)
        print('deepspeech2 h512 facade:', res['bi_text'], res['bi_score'], '| stream:', res['stream_text'][-1], res['stream_score'][-1])
    for f in ('deepspeech2_rnn_sizes.npz', 'predictor_deepspeech2_h512.npz'):
        print(' ', f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == '__main__':
    main()
