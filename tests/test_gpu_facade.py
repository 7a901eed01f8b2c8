"""GPU: the drop-in Python surface (MASRPredictor / InferencePredictor / AudioFeaturizer / greedy
decoders) against fixtures recorded from the REAL reference facade (oracle/make_golden.py ->
predictor.npz: MASRPredictor(use_gpu=False).predict / predict_stream on dataset/test.wav)."""
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')

CONFIG = """
encoder_conf: {output_size: 256, attention_heads: 4, linear_units: 2048, num_blocks: 12, dropout_rate: 0.1,
  positional_dropout_rate: 0.1, attention_dropout_rate: 0.1, input_layer: conv2d, normalize_before: True,
  cnn_module_kernel: 15, use_cnn_module: True, activation_type: swish, pos_enc_layer_type: rel_pos}
preprocess_conf: {feature_method: fbank, n_mels: 80, n_mfcc: 40, sample_rate: 16000, use_dB_normalization: True, target_dB: -20}
dataset_conf: {dataset_vocab: VOCAB}
use_model: conformer
streaming: True
decoder: ctc_greedy
metrics_type: cer
"""


@pytest.fixture(scope='module')
def predictor(tmp_path_factory):
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    d = tmp_path_factory.mktemp('facade')
    vpath = os.path.join(d, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(4233):
            f.write(f'{t}\t1\n')
    cfg = yaml.safe_load(CONFIG.replace('VOCAB', vpath))
    sd = synthetic.conformer_state_dict(0, 4233)
    # also exercise the artefact loader: model.pt (state_dict) on disk
    mpath = os.path.join(d, 'model.pt')
    torch.save(sd, mpath)
    return MASRPredictor(configs=cfg, model_path=mpath, use_gpu=True)


def _close(a, b):
    from oracle import decoders as od
    return od.cer(a, b)


def _gain_reproducible():
    """True when this host's numpy evaluates the normalisation gain of test.wav to the float32 the fixture host did
    (engine.reference_gains; numpy's float32 log10 / power are machine dependent).  Then every transcript recorded from the
    reference facade must be reproduced EXACTLY; otherwise +-1 LSB int16 differences may move single characters."""
    from masr_amd.engine import reference_gains
    tw = np.load(os.path.join(GOLDEN, 'testwav.npz'))
    return reference_gains(np.array([tw['mean_square']], np.float32), -20)[0] == tw['gain']


def _same(ref_text, text, ref_score, score, what):
    c = _close(ref_text, text)
    print(f'{what}: CER vs reference facade {c}, score {score:.4f} vs {ref_score:.4f}')
    if _gain_reproducible():
        assert text == ref_text, (what, text, ref_text)
        assert abs(score - ref_score) < 1e-3, (what, score, ref_score)
    else:
        assert c <= 0.1 and abs(score - ref_score) < 0.5, (what, text, ref_text)


def test_predict_offline_matches_reference_facade(predictor):
    z = np.load(os.path.join(GOLDEN, 'predictor.npz'))
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    res = predictor.predict(audio_data=pcm.copy())
    _same(str(z['offline_text']), res['text'], float(z['offline_score']), res['score'], 'conformer predict(test.wav)')


def test_predict_stream_matches_reference_facade(predictor):
    z = np.load(os.path.join(GOLDEN, 'predictor.npz'))
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    predictor.reset_stream()
    step, n = 8000, len(pcm)
    k = 0
    for s in range(0, n, step):
        r = predictor.predict_stream(audio_data=pcm[s:s + step].tobytes(), is_end=(s + step >= n))
        valid = r is not None and r['text'] is not None
        assert valid == bool(z['stream_valid'][k]), f'call {k}: validity differs'
        if valid:
            _same(str(z['stream_text'][k]), r['text'], float(z['stream_score'][k]), r['score'], f'conformer predict_stream call {k}')
        k += 1
    predictor.reset_stream()
    # after reset the first call behaves like a fresh stream
    r = predictor.predict_stream(audio_data=pcm[:8000].tobytes(), is_end=False)
    assert (r is not None) == bool(z['stream_valid'][0])
    predictor.reset_stream()


def test_predict_batch_equals_single(predictor):
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    # equal lengths: with padding the reference's pad mask keeps one extra (padding-contaminated)
    # attention key per utterance, so ragged batch != single by construction (see test_gpu_parity)
    a, b = pcm[:60000].copy(), pcm[70000:130000].copy()
    single = [predictor.predict(audio_data=x.copy()) for x in (a, b)]
    batch = predictor.predict_batch([a, b])
    for s, t in zip(single, batch):
        assert _close(s['text'], t['text']) <= 0.05
        assert abs(s['score'] - t['score']) < 0.2


def test_greedy_decoder_api_known_answer():
    from masr_amd.decoders.ctc_greedy_decoder import greedy_decoder, greedy_decoder_batch, greedy_decoder_chunk
    vocab = ['<blank>', '<unk>', 'a', 'b', '<space>', '<eos>']
    p = np.array([[.1, 0, .8, .1, 0, 0], [.1, 0, .7, .2, 0, 0], [.9, 0, .05, .05, 0, 0], [.1, 0, .6, .3, 0, 0],
                  [0, 0, .1, .2, .7, 0], [.2, 0, .1, .7, 0, 0]], np.float32)
    assert greedy_decoder(p, vocab) == (69.9999988079071, 'aa b')       # reference KAT, SURVEY.md 8(a-15)
    s, t, a, b = greedy_decoder_chunk(p[:3], vocab)
    assert (s, t) == (75.0, 'a')
    s, t, a, b = greedy_decoder_chunk(p[3:], vocab, a, b)
    assert (s, t) == (69.9999988079071, 'aa b')
    assert greedy_decoder_batch([p, p[:2]], vocab) == ['aa b', 'a']
    z = np.load(os.path.join(GOLDEN, 'greedy.npz'))
    s, t = greedy_decoder(z['probs'], vocab)
    assert s == float(z['score']) and t == str(z['text'])


def test_featurizer_api(predictor):
    from masr_amd.data_utils.audio import AudioSegment
    from masr_amd.data_utils.featurizer.audio_featurizer import AudioFeaturizer
    z = np.load(os.path.join(GOLDEN, 'testwav.npz'))
    seg = AudioSegment.from_ndarray(z['pcm'], 16000)
    before = seg.samples
    feat = AudioFeaturizer(feature_method='fbank', n_mels=80, sample_rate=16000, use_dB_normalization=True,
                           target_dB=-20).featurize(seg)
    assert feat.shape == (837, 80) and feat.dtype == np.float32
    err = np.abs(feat - z['fbank'])
    # gain is reproducible only to a few ulp (see test_gpu_parity.test_fbank_testwav...): frames that
    # contain a +-1 LSB sample may move by up to 0.1, everything else agrees to 1e-3
    assert err.max() < 0.1 and np.quantile(err.max(axis=1), 0.5) < 1e-3
    # the segment was normalised in place, like the reference (audio.py:304)
    ms = float(np.mean(seg.samples.astype(np.float64) ** 2))
    assert abs(10 * np.log10(ms) + 20.0) < 1e-3 and not np.allclose(before, seg.samples)


def _squeezeformer_beam_cfg(tmp_path, V, beam, lm_path):
    from masr_amd.utils import synthetic
    vocab = synthetic.synthetic_vocab(V)
    vpath = os.path.join(tmp_path, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in vocab:
            f.write(f'{t}\t1\n')
    cfg = {'encoder_conf': {'encoder_dim': 256, 'output_size': 256, 'attention_heads': 4, 'num_blocks': 12, 'reduce_idx': 5,
                            'recover_idx': 11, 'feed_forward_expansion_factor': 8, 'cnn_module_kernel': 31},
           'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'ctc_beam_search_decoder_conf': {'alpha': 2.2, 'beta': 4.3, 'beam_size': beam, 'num_processes': 10,
                                            'cutoff_prob': 0.99, 'cutoff_top_n': 40, 'language_model_path': lm_path},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'squeezeformer', 'streaming': False,
           'decoder': 'ctc_beam_search', 'metrics_type': 'cer'}
    return cfg, vocab


def test_squeezeformer_beam_search_facade(tmp_path):
    """BASELINE config 3 shape: squeezeformer.yml (streaming: False) + ctc_beam_search with the external scorer through the
    facade, checked against the oracle pipeline (fbank -> Squeezeformer -> the published decoder with its pruning rule and
    alpha 2.2 / beta 4.3): transcript identical, score to 1e-3.  A missing LM file is the reference's assertion."""
    from masr_amd.decoders.lm_scorer import write_synthetic_arpa
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    from oracle import beam_search as obs, fbank as ofb, squeezeformer as osq
    V = 300
    sd = synthetic.squeezeformer_state_dict(0, V)
    cfg, vocab = _squeezeformer_beam_cfg(tmp_path, V, 10, 'lm/absent.klm')
    with pytest.raises(AssertionError, match='语言模型不存在'):       # beam_search_decoder.py:28
        MASRPredictor(configs=cfg, use_gpu=True, state_dict=sd)
    lm_path = write_synthetic_arpa(os.path.join(tmp_path, 'lm3.arpa'), vocab, order=3, seed=3, n_higher=6000)
    cfg, vocab = _squeezeformer_beam_cfg(tmp_path, V, 10, lm_path)
    pred = MASRPredictor(configs=cfg, use_gpu=True, state_dict=sd)
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm'][:48000]
    res = pred.predict(audio_data=pcm.copy())
    feat, _ = ofb.featurize_pcm16(pcm)
    with torch.no_grad():
        probs = osq.get_encoder_out(sd, torch.from_numpy(feat)[None], torch.tensor([feat.shape[0]]))[0].numpy()
    sc = obs.Scorer(obs.ArpaLM(lm_path), vocab, 2.2, 4.3)
    s_ref, toks_ref, _ = obs.ctc_beam_search_decoder(probs, vocab, 10, 0.99, 40, sc, 0)
    t_ref = ''.join(vocab[t] for t in toks_ref).replace('<space>', ' ')
    assert res['text'] == t_ref, (res['text'], t_ref)
    assert abs(res['score'] - s_ref) < 1e-3 * max(1.0, abs(s_ref)), (res['score'], s_ref)
    batch = pred.predict_batch([pcm.copy(), pcm.copy()])
    assert batch[0]['text'] == batch[1]['text'] == res['text']
    with pytest.raises(Exception):
        pred.predict_stream(audio_data=pcm[:8000].tobytes())       # streaming: False (predict.py:253-255)


# ---------------------------------------------------------------------------------------------------
# BASELINE config 1: deepspeech2.yml, B=1 on dataset/test.wav, ctc_greedy (fixture: predictor_deepspeech2.npz)
# ---------------------------------------------------------------------------------------------------
DS2_CONFIG = """
encoder_conf: {num_rnn_layers: 5, rnn_size: 1024, use_gru: False}
preprocess_conf: {feature_method: fbank, n_mels: 80, n_mfcc: 40, sample_rate: 16000, use_dB_normalization: True, target_dB: -20}
dataset_conf: {dataset_vocab: VOCAB}
use_model: deepspeech2
streaming: STREAMING
decoder: ctc_greedy
metrics_type: cer
"""


def _ds2_predictor(d, streaming):
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    vpath = os.path.join(d, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(4233):
            f.write(f'{t}\t1\n')
    cfg = yaml.safe_load(DS2_CONFIG.replace('VOCAB', vpath).replace('STREAMING', str(streaming)))
    sd = synthetic.deepspeech2_state_dict(0, 4233, bidirectional=not streaming)
    mpath = os.path.join(d, f'model_{streaming}.pt')
    torch.save(sd, mpath)
    return MASRPredictor(configs=cfg, model_path=mpath, use_gpu=True)


def test_deepspeech2_config1_matches_reference_facade(tmp_path):
    z = np.load(os.path.join(GOLDEN, 'predictor_deepspeech2.npz'))
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    p = _ds2_predictor(str(tmp_path), False)
    res = p.predict(audio_data=pcm.copy())
    _same(str(z['bi_text']), res['text'], float(z['bi_score']), res['score'], 'deepspeech2 (bi) predict(test.wav): BASELINE configs[0]')
    with pytest.raises(Exception):
        p.predict_stream(audio_data=pcm[:8000].tobytes())       # non-streaming model: predict.py:262-263


def test_deepspeech2_stream_matches_reference_facade(tmp_path):
    z = np.load(os.path.join(GOLDEN, 'predictor_deepspeech2.npz'))
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    p = _ds2_predictor(str(tmp_path), True)
    res = p.predict(audio_data=pcm.copy())
    _same(str(z['uni_text']), res['text'], float(z['uni_score']), res['score'], 'deepspeech2 (uni) predict(test.wav)')
    p.reset_stream()
    k = 0
    for s in range(0, len(pcm), 8000):
        r = p.predict_stream(audio_data=pcm[s:s + 8000].tobytes(), is_end=(s + 8000 >= len(pcm)))
        valid = r is not None and r['text'] is not None
        assert valid == bool(z['stream_valid'][k]), f'call {k}: validity differs'
        if valid:
            _same(str(z['stream_text'][k]), r['text'], float(z['stream_score'][k]), r['score'], f'deepspeech2 predict_stream call {k}')
        k += 1
    p.reset_stream()


def test_evaluate_manifest_matches_per_utterance_cer(predictor, tmp_path):
    """batched evaluation over a reference-format manifest == per-utterance predict + CER"""
    import json
    import wave
    from masr_amd.utils.metrics import cer
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    pieces = [pcm[:32000], pcm[20000:68000], pcm[40000:56000], pcm[60000:124000]]
    labels = ['丁丂七丄', '丅丆万丈三上下', '丌不', '与丏丐丑丒专且丕世']
    man = os.path.join(tmp_path, 'manifest.test')
    with open(man, 'w', encoding='utf-8') as f:
        for i, (p, t) in enumerate(zip(pieces, labels)):
            path = os.path.join(tmp_path, f'u{i}.wav')
            with wave.open(path, 'wb') as w:
                w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
                w.writeframes(p.astype('<i2').tobytes())
            f.write(json.dumps({'audio_filepath': path, 'text': t, 'duration': len(p) / 16000}, ensure_ascii=False) + '\n')
    loss, err = predictor.evaluate(man, batch_size=3, display_result=True)
    assert loss == -1
    # same batches by hand: sorted by duration -> [u2, u0, u1], [u3]
    paths = [os.path.join(tmp_path, f'u{i}.wav') for i in range(4)]
    r1 = predictor.predict_batch([paths[2], paths[0], paths[1]])
    r2 = predictor.predict_batch([paths[3]])
    want = np.mean([cer(r1[0]['text'], labels[2]), cer(r1[1]['text'], labels[0]), cer(r1[2]['text'], labels[1]),
                    cer(r2[0]['text'], labels[3])])
    assert err == pytest.approx(float(want))
    # a batch of one is the single-utterance path
    assert r2[0]['text'] == predictor.predict(audio_data=paths[3])['text']
    # and against the ORACLE (not the product itself): the reference's CPU arithmetic on the same padded batches --
    # features of each utterance, zero-padded batch, get_encoder_out, greedy decode over each utterance's own frames
    from masr_amd.utils import synthetic
    from oracle import conformer as oc, decoders as od, fbank as ofb
    sd, vocab = synthetic.conformer_state_dict(0, 4233), synthetic.synthetic_vocab(4233)
    errs = []
    for batch in ([2, 0, 1], [3]):
        fl = [ofb.featurize_pcm16(pieces[i])[0] for i in batch]
        T = max(f.shape[0] for f in fl)
        feats = np.zeros((len(batch), T, 80), np.float32)
        for j, f in enumerate(fl):
            feats[j, :f.shape[0]] = f
        with torch.no_grad():
            probs = oc.get_encoder_out(sd, torch.from_numpy(feats), torch.tensor([f.shape[0] for f in fl])).numpy()
        for j, i in enumerate(batch):
            _, text = od.greedy_decoder(probs[j, :oc.subsampled_len(fl[j].shape[0])], vocab)
            errs.append(cer(text, labels[i]))
    print(f'evaluate(): CER {err} vs oracle pipeline {np.mean(errs)}')
    assert err == pytest.approx(float(np.mean(errs)), abs=1e-9 if _gain_reproducible() else 0.05)


def test_predict_long_batches_vad_segments(predictor):
    """predict_long = VAD segments -> batched recognition -> texts joined like predict.py:222-233"""
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    long_pcm = np.concatenate([pcm, np.zeros(8000, np.int16), pcm[::-1], np.zeros(4000, np.int16), pcm[:70000]])

    class FixedVAD:                      # the reference VADPredictor's interface (vad_predictor.py:105-168)
        def get_speech_timestamps(self, audio, sampling_rate):
            assert audio.dtype == np.float32 and sampling_rate == 16000
            n = len(pcm)
            return [{'start': 0, 'end': n}, {'start': n + 8000, 'end': 2 * n + 8000},
                    {'start': 2 * n + 12000, 'end': 2 * n + 12000 + 70000}]

    seg = [long_pcm[0:len(pcm)], long_pcm[len(pcm) + 8000:2 * len(pcm) + 8000], long_pcm[2 * len(pcm) + 12000:]]
    single = [predictor.predict(audio_data=x.copy()) for x in seg]
    want_text = '，'.join(r['text'] for r in single if r['text'] != '')
    want_score = round(sum(r['score'] for r in single) / 3, 2)
    exact = predictor.predict_long(long_pcm.copy(), vad_predictor=FixedVAD(), batch_size=1)
    assert exact == {'text': want_text, 'score': want_score}
    batched = predictor.predict_long(long_pcm.copy(), vad_predictor=FixedVAD(), batch_size=8)
    assert _close(want_text, batched['text']) <= 0.05 and abs(batched['score'] - want_score) < 0.2
    # built-in energy VAD: silence-separated speech-like bursts come back as separate, recognisable segments
    from masr_amd.infer_utils.vad_predictor import EnergyVAD
    res = predictor.predict_long(long_pcm.copy(), vad_predictor=EnergyVAD(), batch_size=8)
    assert isinstance(res['text'], str) and res['score'] >= 0


def test_server_front_end_batches_requests_and_streams(predictor):
    """the reference server's protocol (infer_server.py) on the batching EngineWorker"""
    import io
    import threading
    import warnings
    import wave
    warnings.simplefilter('ignore')
    from starlette.testclient import TestClient
    from masr_amd.server import create_app
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']

    def wav_bytes(x):
        b = io.BytesIO()
        with wave.open(b, 'wb') as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes(x.astype('<i2').tobytes())
        return b.getvalue()

    clips = [pcm[:64000], pcm[30000:94000], pcm[60000:124000], pcm[10000:74000]]       # equal lengths: batch == single
    want = [predictor.predict(audio_data=c.copy()) for c in clips]
    stream_want = []
    predictor.reset_stream()
    chunks = [pcm[i:i + 16000] for i in range(0, len(pcm), 16000)]
    for i, ch in enumerate(chunks):
        r = predictor.predict_stream(audio_data=ch.astype('<i2').tobytes(), is_end=i == len(chunks) - 1)
        stream_want.append(r['text'] if r is not None else (stream_want[-1] if stream_want else ''))
    predictor.reset_stream()

    app = create_app(predictor, max_batch=8, max_wait_ms=1500.0, max_frames_out=400)
    with TestClient(app) as c:
        got = [None] * len(clips)

        def post(i):
            got[i] = c.post('/recognition', content=wav_bytes(clips[i])).json()

        th = [threading.Thread(target=post, args=(i,)) for i in range(len(clips))]
        [t.start() for t in th]
        [t.join() for t in th]
        for g, w in zip(got, want):
            assert g['code'] == 0 and _close(w['text'], g['result']) <= 0.05 and abs(g['score'] - w['score']) < 0.2
        stats = app.state.worker.stats
        assert stats['utterances'] == 4 and stats['batches'] < 4                          # requests shared device calls
        assert c.post('/recognition', content=b'not a wav').json() == {'error': 1, 'msg': 'audio read fail!'}
        # two websocket sessions at once, each the reference's predict_stream protocol
        with c.websocket_connect('/') as ws1, c.websocket_connect('/') as ws2:
            for i, ch in enumerate(chunks):
                data = ch.astype('<i2').tobytes() + (b'end' if i == len(chunks) - 1 else b'')
                ws1.send_bytes(data)
                ws2.send_bytes(data)
                r1, r2 = ws1.receive_json(), ws2.receive_json()
                assert r1 == r2 == {'code': 0, 'result': stream_want[i]}


def test_squeezeformer_predict_stream_facade(tmp_path):
    """squeezeformer.yml as shipped (streaming: True) through MASRPredictor.predict_stream (engine-level parity of the chunk
    path: test_gpu_parity.test_squeezeformer_stream_chunks_against_reference_fixture)"""
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    from oracle import decoders as od, fbank as ofb, squeezeformer as osq
    V = 300
    vocab = synthetic.synthetic_vocab(V)
    vpath = os.path.join(tmp_path, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in vocab:
            f.write(f'{t}\t1\n')
    cfg = {'encoder_conf': {'encoder_dim': 256, 'output_size': 256, 'attention_heads': 4, 'num_blocks': 12, 'reduce_idx': 5,
                            'recover_idx': 11, 'feed_forward_expansion_factor': 8, 'cnn_module_kernel': 31},
           'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'squeezeformer', 'streaming': True,
           'decoder': 'ctc_greedy', 'metrics_type': 'cer'}
    sd = synthetic.squeezeformer_state_dict(0, V, streaming=True)
    pred = MASRPredictor(configs=cfg, use_gpu=True, state_dict=sd)
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm'][:64000]
    def run():
        pred.reset_stream()
        last, parts = None, 0
        for s in range(0, len(pcm), 8000):
            r = pred.predict_stream(audio_data=pcm[s:s + 8000].tobytes(), is_end=(s + 8000 >= len(pcm)))
            if r is not None and r['text'] is not None:
                last, parts = r, parts + 1
        pred.reset_stream()
        return last, parts
    a, na = run()
    b, nb = run()                       # reset_stream gives a fresh stream: same partials again
    assert a is not None and len(a['text']) > 0 and na >= 5
    assert a == b and na == nb


def test_efficient_conformer_predict_stream_facade(tmp_path):
    """efficient_conformer.yml (streaming: True) through MASRPredictor.predict_stream (engine-level parity of the chunk path:
    test_gpu_parity.test_efficient_conformer_stream_chunks_against_reference_fixture)"""
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    V = 300
    vocab = synthetic.synthetic_vocab(V)
    vpath = os.path.join(tmp_path, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in vocab:
            f.write(f'{t}\t1\n')
    cfg = {'encoder_conf': {'output_size': 256, 'attention_heads': 4, 'linear_units': 2048, 'num_blocks': 12,
                            'cnn_module_kernel': 15,
                            'efficient_conf': {'stride_layer_idx': [3], 'stride': [2], 'group_layer_idx': [0, 1, 2, 3],
                                               'group_size': 3, 'stride_kernel': True}},
           'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'efficient_conformer', 'streaming': True,
           'decoder': 'ctc_greedy', 'metrics_type': 'cer'}
    pred = MASRPredictor(configs=cfg, use_gpu=True, state_dict=synthetic.efficient_conformer_state_dict(0, V))
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm'][:64000]

    def run():
        pred.reset_stream()
        last, parts = None, 0
        for s in range(0, len(pcm), 8000):
            r = pred.predict_stream(audio_data=pcm[s:s + 8000].tobytes(), is_end=(s + 8000 >= len(pcm)))
            if r is not None and r['text'] is not None:
                last, parts = r, parts + 1
        pred.reset_stream()
        return last, parts
    a, na = run()
    b, nb = run()
    assert a is not None and len(a['text']) > 0 and na >= 5
    assert a == b and na == nb


def test_stream_pool_equals_independent_predict_stream(predictor):
    """StreamPool (batched sessions): every session gets the partial results of its own predict_stream"""
    from masr_amd.serving import StreamPool
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    audios = [pcm[:72000], pcm[30000:110000], pcm[50000:83000]]
    step = 8000
    # reference behaviour: one predictor, one stream at a time
    want = []
    for a in audios:
        predictor.reset_stream()
        parts = []
        for s in range(0, len(a), step):
            parts.append(predictor.predict_stream(audio_data=a[s:s + step].tobytes(), is_end=(s + step >= len(a))))
        want.append(parts)
    predictor.reset_stream()
    # the same three streams concurrently
    pool = StreamPool(predictor)
    hs = [pool.open() for _ in audios]
    got = [[] for _ in audios]
    for k in range(max(len(a) for a in audios) // step + 1):
        for i, a in enumerate(audios):
            s = k * step
            if s < len(a):
                pool.feed(hs[i], a[s:s + step].tobytes(), is_end=(s + step >= len(a)))
        out = pool.step()
        for i, h in enumerate(hs):
            if h in out:
                got[i].append(out[h])
        # the device rows a multi-GPU front-end all-gathers (zero-copy view of the C pool's buffer): tokens | count | score bits of
        # exactly the sessions that advanced, equal to what the step returned on the host
        packed = pool.last_packed
        advanced = [h for h in hs if out.get(h) is not None]
        if advanced:
            rows_dev, tmax, sids = packed
            assert rows_dev.is_cuda and list(sids) == advanced and tuple(rows_dev.shape) == (len(advanced), tmax + 2)
            rows_h = rows_dev.cpu().numpy()
            for j, h in enumerate(sids):
                nt = int(rows_h[j, tmax])
                assert rows_h[j, :nt].tolist() == pool.last_tokens(h)
                score = float(rows_h[j, tmax + 1:tmax + 2].view(np.float32)[0]) * 100.0 if nt > 0 else 0
                assert abs(score - out[h]['score']) < 1e-6
        else:
            assert packed is None
    for i in range(len(audios)):
        assert len(got[i]) == len(want[i])
        for g_, w_ in zip(got[i], want[i]):
            assert (g_ is None) == (w_ is None or w_['text'] is None)
            if g_ is not None:
                assert _close(w_['text'], g_['text']) <= 0.02, (w_['text'], g_['text'])
                assert abs(g_['score'] - w_['score']) < 0.05
    # a session can be reused for the next utterance
    pool.reset(hs[0])
    pool.feed(hs[0], audios[2].tobytes(), is_end=True)
    again = pool.step()[hs[0]]
    predictor.reset_stream()
    one = predictor.predict_stream(audio_data=audios[2].tobytes(), is_end=True)       # same single-call feeding
    predictor.reset_stream()
    assert _close(one['text'], again['text']) <= 0.02 and abs(one['score'] - again['score']) < 0.05
    for h in hs:
        pool.close(h)


def test_c_pool_step_equals_the_python_framing(predictor, monkeypatch):
    """masr_pool_step (csrc/pool.hip, round 4) against the python framing it replaces (serving.py, MASR_POOL_PY=1) on the same
    engine: five sessions fed in irregular patterns -- a whole 8.4 s utterance in one call (the frame pool's rows widen), 50 ms
    crumbs, an empty feed that only carries is_end, two feeds of one session inside one step, a float32 array, a session reset
    and reused -- must return the same partial results call by call: identical token ids, scores to 1e-4."""
    from masr_amd.serving import StreamPool
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    monkeypatch.setenv('MASR_POOL_PY', '1')
    py_pool = StreamPool(predictor)
    monkeypatch.delenv('MASR_POOL_PY')
    c_pool = StreamPool(predictor)
    assert py_pool.framing == 'python' and c_pool.framing == 'c'
    rng = np.random.default_rng(11)
    script = []                                        # per step: list of (session, samples, is_end)
    cuts = {1: sorted(rng.integers(1, len(pcm) - 1, 40).tolist()), 2: list(range(800, 60000, 800)), 3: [30000, 90000, 90000]}
    pos = {k: 0 for k in (0, 1, 2, 3, 4)}
    for step in range(46):
        feeds = []
        if step == 0:
            feeds.append((0, pcm, True))                                   # everything at once
        for k in (1, 2, 3):
            if cuts[k]:
                hi = cuts[k].pop(0)
                feeds.append((k, pcm[pos[k]:hi], not cuts[k]))
                pos[k] = hi
        if step % 3 == 0 and pos[4] < 70000:
            a, b = pos[4], pos[4] + 3000
            feeds.append((4, pcm[a:b].astype(np.float32) / np.float32(32768.0), False))     # float samples, twice in one step
            feeds.append((4, pcm[b:b + 2500], b + 2500 >= 70000))
            pos[4] = b + 2500
        script.append(feeds)
    results = []
    for pool in (py_pool, c_pool):
        hs = [pool.open() for _ in range(5)]
        out = []
        for step, feeds in enumerate(script):
            if step == 20:                                                  # session 0: a second utterance on the same session
                pool.reset(hs[0])
                pool.feed(hs[0], pcm[:50000].tobytes(), is_end=True)
            for k, a, end in feeds:
                pool.feed(hs[k], a.tobytes() if a.dtype == np.int16 else a, is_end=end)
            res = pool.step()
            out.append({hs.index(h): (None if r is None else (r['text'], r['score'], tuple(pool.last_tokens(h)))) for h, r in res.items()})
        for h in hs:
            pool.close(h)
        results.append(out)
    n_results = 0
    for a, b in zip(*results):
        assert a.keys() == b.keys()
        for k in a:
            assert (a[k] is None) == (b[k] is None), (k, a[k], b[k])
            if a[k] is not None:
                assert a[k][2] == b[k][2] and a[k][0] == b[k][0] and abs(a[k][1] - b[k][1]) < 1e-4, (k, a[k][:2], b[k][:2])
                n_results += 1
    assert n_results > 20


def test_c_pool_step_leaves_a_full_session_out_and_validates_feeds(predictor):
    """masr_pool_step: (1) a session whose stream has no room for the frames a step would emit is LEFT OUT of the lock-step
    call (state -1) -- its neighbour's partials are what they are without it, call by call; (2) a malformed feed is rejected
    before any session state changes: the same step repeated with the feed fixed gives the undisturbed result."""
    import ctypes as C
    from masr_amd import _lib
    from masr_amd.serving import StreamPool
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    chunks = [pcm[i:i + 8000] for i in range(0, 64000, 8000)]          # 4 s: ~100 encoder frames
    alone = StreamPool(predictor)
    h = alone.open()
    want = []
    for k, c in enumerate(chunks):
        alone.feed(h, c.tobytes(), is_end=k == len(chunks) - 1)
        want.append(alone.step()[h])
    alone.close(h)
    alone.shutdown()
    # ONE pool whose limit only the first session reaches: `full` is fed three times as fast as its neighbour
    pool = StreamPool(predictor, max_frames_out=120)
    full, ok = pool.open(), pool.open()
    room = C.c_int32()
    assert pool.engine.lib.masr_stream_room(pool.engine.h, ok, C.byref(room)) == 0 and room.value == 120
    got, refused_at = [], None
    for k, c in enumerate(chunks):
        pool.feed(ok, c.tobytes(), is_end=k == len(chunks) - 1)
        pool.feed(full, np.concatenate([c, c, c]).tobytes(), is_end=False)
        res = pool.step()
        got.append(res[ok])
        if full in pool.errors and refused_at is None:
            refused_at = k
            assert res[full] is None
    assert refused_at is not None and refused_at > 0, 'the fast session never reached max_frames_out'
    for a, b in zip(got, want):
        assert (a is None) == (b is None) and (a is None or (a['text'] == b['text'] and abs(a['score'] - b['score']) < 1e-4))
    pool.reset(full)
    assert full not in pool.errors
    pool.feed(full, chunks[0].tobytes(), is_end=True)
    pool.step()                                               # the reset session takes audio again
    assert full not in pool.errors
    # (2) validation: a negative sample count is refused, nothing is committed
    p2 = StreamPool(predictor)
    a = p2.open()
    p2.feed(a, chunks[0].tobytes(), is_end=False)
    first = p2.step()[a]
    handles = np.array([a], np.int32)
    arr = np.ascontiguousarray(chunks[1])
    ptrs = np.array([arr.ctypes.data], np.uint64)
    ns, width = C.c_int32(), C.c_int32()
    outs = [C.c_void_p() for _ in range(4)]
    call = lambda count: p2._lib.masr_pool_step(p2._c, 1, handles.ctypes.data, ptrs.ctypes.data, np.array([count], np.int64).ctypes.data,
                                                np.array([0], np.int32).ctypes.data, np.array([0], np.int32).ctypes.data,
                                                C.cast(p2._gain_cb, C.c_void_p), None, C.byref(ns), C.byref(outs[0]), C.byref(outs[1]),
                                                C.byref(outs[2]), C.byref(width), C.byref(outs[3]),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(-5) != 0 and 'feed_n' in _lib.lib().masr_last_error().decode()
    assert call(1 << 40) != 0
    p2.feed(a, chunks[1].tobytes(), is_end=False)
    second = p2.step()[a]
    assert second == want[1] or (second is not None and want[1] is not None and second['text'] == want[1]['text'])
    assert (first is None) == (want[0] is None)
    p2.close(a)
    p2.shutdown()
    pool.shutdown()


def test_stream_pool_deepspeech2(tmp_path):
    """StreamPool over the streaming DeepSpeech2: two concurrent sessions == two sequential predict_stream runs"""
    from masr_amd.serving import StreamPool
    p = _ds2_predictor(str(tmp_path), True)
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    audios = [pcm[:64000], pcm[40000:96000]]
    want = []
    for a in audios:
        p.reset_stream()
        want.append([p.predict_stream(audio_data=a[s:s + 8000].tobytes(), is_end=(s + 8000 >= len(a)))
                     for s in range(0, len(a), 8000)])
    p.reset_stream()
    pool = StreamPool(p)
    hs = [pool.open() for _ in audios]
    got = [[] for _ in audios]
    for k in range(8):
        for i, a in enumerate(audios):
            if k * 8000 < len(a):
                pool.feed(hs[i], a[k * 8000:(k + 1) * 8000].tobytes(), is_end=((k + 1) * 8000 >= len(a)))
        out = pool.step()
        for i, h in enumerate(hs):
            if h in out:
                got[i].append(out[h])
    for i in range(2):
        assert len(got[i]) == len(want[i])
        for g_, w_ in zip(got[i], want[i]):
            assert (g_ is None) == (w_ is None or w_['text'] is None)
            if g_ is not None:
                assert _close(w_['text'], g_['text']) <= 0.02 and abs(g_['score'] - w_['score']) < 0.05
    for h in hs:
        pool.close(h)


@pytest.mark.parametrize('method', ['linear', 'mfcc'])
def test_facade_with_linear_and_mfcc_features(tmp_path, method):
    """preprocess_conf.feature_method linear / mfcc through MASRPredictor (featurizer + model input size 161 / n_mfcc)"""
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    from oracle import conformer as oc, decoders as od
    z = np.load(os.path.join(GOLDEN, 'features.npz'))
    dim = {'linear': 161, 'mfcc': 40}[method]
    vpath = os.path.join(tmp_path, 'vocabulary.txt')
    vocab = synthetic.synthetic_vocab(512)
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in vocab:
            f.write(f'{t}\t1\n')
    cfg = yaml.safe_load(CONFIG.replace('VOCAB', vpath).replace('feature_method: fbank', f'feature_method: {method}'))
    sd = synthetic.conformer_state_dict(0, 512, n_mels=dim)
    sd['encoder.global_cmvn.mean'] = torch.from_numpy(z[method + '_cmvn'][0])
    sd['encoder.global_cmvn.istd'] = torch.from_numpy(z[method + '_cmvn'][1])
    p = MASRPredictor(configs=cfg, use_gpu=True, state_dict=sd)
    assert p._audio_featurizer.feature_dim == dim
    res = p.predict(audio_data=z['pcm'].copy())
    score, text = od.greedy_decoder(z[method + '_probs'], vocab)          # decode of the reference model's probabilities
    assert od.cer(text, res['text']) <= 0.1 and abs(res['score'] - score) < 0.5
    batch = p.predict_batch([z['pcm'].copy(), z['pcm'].copy()])
    assert od.cer(text, batch[0]['text']) <= 0.1 and batch[0]['text'] == batch[1]['text']


def test_predict_batch_and_evaluate_through_the_rccl_exchange(predictor, tmp_path, monkeypatch):
    """the multi-GPU path of predict_batch / evaluate on ONE rank with the exchange forced on (MASR_FORCE_DIST=1): process
    group on the nccl (= RCCL) backend, length-balanced shard list, local decode as token ids, all-gather, text -- must return
    exactly what the single-process call returns (the 2-rank logic is covered on gloo in tests/test_distributed_cpu.py)"""
    import socket
    import torch.distributed as dist
    from masr_amd import parallel
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    pieces = [pcm[:32000].copy(), pcm[20000:68000].copy(), pcm[40000:56000].copy(), pcm[60000:124000].copy(), pcm[:900].copy()]
    want = predictor.predict_batch(pieces, batch_size=2)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    for k, v in (('MASR_FORCE_DIST', '1'), ('MASTER_ADDR', '127.0.0.1'), ('MASTER_PORT', str(port)), ('RANK', '0'),
                 ('WORLD_SIZE', '1'), ('LOCAL_RANK', '0')):
        monkeypatch.setenv(k, v)
    assert not dist.is_initialized()
    rank, world, local = parallel.init_from_env()
    try:
        assert dist.get_backend() == 'nccl' and parallel.collectives_on()
        got = predictor.predict_batch(pieces, batch_size=2, distributed=True)
        assert [g['text'] for g in got] == [w['text'] for w in want]
        assert all(abs(g['score'] - w['score']) < 1e-3 for g, w in zip(got, want))
        assert got[4] == {'text': '', 'score': 0.0} or got[4]['text'] == ''          # shorter than one decoding window
        # the stream router's exchange: the pool's device-packed rows through ONE fixed-width all-gather == the local partials
        from masr_amd.serving import StreamPool
        local_pool, sharded = StreamPool(predictor), parallel.ShardedStreamPool(StreamPool(predictor, max_frames_out=400))
        hl = [local_pool.open() for _ in range(3)]
        hg = [sharded.open() for _ in range(3)]
        for lo in range(0, 48000, 8000):
            for k in range(3):
                chunk = pcm[10000 * k + lo:10000 * k + lo + 8000].tobytes()
                local_pool.feed(hl[k], chunk, is_end=lo + 8000 >= 48000)
                sharded.feed(hg[k], chunk, is_end=lo + 8000 >= 48000)
            a, b = local_pool.step(), sharded.step(gather=True)
            for k in range(3):
                assert (a[hl[k]] is None) == (b[hg[k]] is None)
                if a[hl[k]] is not None:
                    assert a[hl[k]]['text'] == b[hg[k]]['text'] and abs(a[hl[k]]['score'] - b[hg[k]]['score']) < 1e-3
        assert any(v is not None and v['text'] for v in b.values())
    finally:
        dist.destroy_process_group()


def test_predict_on_8k_and_44k1_input_goes_through_the_reference_resampler(predictor):
    """Every request that is not at the model's rate passes AudioSegment.resample (audio_featurizer.py:37-69 ->
    audio.py:306-317 -> resampy's band-limited sinc interpolation; restated, parity unpinned; its three forms are pinned to each
    other bit for bit on the CPU, tests/test_host_logic.py).  Through the facade: ``predict(x, sample_rate=r)`` for r = 8000 and
    44100 (float and int16 samples) returns exactly what ``predict`` returns for the resampled samples handed over at 16 kHz,
    and the output length is resampy's ``int(n * 16000 / r)``."""
    from masr_amd.data_utils import resample as rs
    from masr_amd.data_utils.audio import AudioSegment
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm'][:64000].astype(np.float32) / 32768.0
    for rate in (8000, 44100):
        x = rs.resample(pcm, 16000, rate).astype(np.float32)            # an utterance "recorded" at that rate
        y = rs.resample(x, rate, 16000)
        assert len(y) == int(len(x) * 16000 / rate)
        seg = AudioSegment.from_ndarray(x, rate)
        seg.resample(16000)
        assert np.array_equal(seg.samples, y)                           # the facade's path (host C++ form) == the numpy form
        got, want = predictor.predict(x, sample_rate=rate), predictor.predict(y)
        assert got == want and len(want['text']) > 0, (rate, got, want)
        xi = np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)
        got_i = predictor.predict(xi, sample_rate=rate)
        want_i = predictor.predict(rs.resample(xi.astype(np.float32) * np.float32(1.0 / 32768.0), rate, 16000))
        assert got_i == want_i, (rate, got_i, want_i)
    batch = predictor.predict_batch([rs.resample(pcm, 16000, 8000).astype(np.float32)] * 2, sample_rate=8000)
    one = predictor.predict(rs.resample(pcm, 16000, 8000).astype(np.float32), sample_rate=8000)
    assert batch[0] == batch[1] and batch[0]['text'] == one['text'] and abs(batch[0]['score'] - one['score']) < 1e-3


def test_stream_pool_feed_forms_are_equivalent(predictor):
    """StreamPool.feed: int16 PCM bytes (kept raw until the step stages them), the same samples as an int16 / float32 ndarray,
    as a bytearray, and a chunk split over two feed calls must give identical partial results; audio at another sample rate
    takes the resampling path."""
    from masr_amd.serving import StreamPool
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm'][:64000]
    step = 8000
    forms = {
        'bytes': lambda c: [c.tobytes()],
        'bytearray': lambda c: [bytearray(c.tobytes())],
        'int16 ndarray': lambda c: [c.copy()],
        'float32 ndarray': lambda c: [c.astype(np.float32) * np.float32(1.0 / 32768.0)],
        'two feeds': lambda c: [c[:3001].tobytes(), c[3001:].tobytes()],
    }
    pool = StreamPool(predictor)
    hs = {name: pool.open() for name in forms}
    got = {name: [] for name in forms}
    for s in range(0, len(pcm), step):
        chunk, end = pcm[s:s + step], s + step >= len(pcm)
        for name, make in forms.items():
            parts = make(chunk)
            for j, part in enumerate(parts):
                pool.feed(hs[name], part, is_end=end and j == len(parts) - 1)
        out = pool.step()
        for name in forms:
            got[name].append(out[hs[name]])
    assert any(r is not None and r['text'] for r in got['bytes'])
    for name in forms:
        assert got[name] == got['bytes'], name
    # 8 kHz input: resampled to the model's rate before it is queued
    h8 = pool.open()
    pool.feed(h8, pcm[::2].copy().tobytes(), is_end=True, sample_rate=8000)
    r8 = pool.step()[h8]
    assert r8 is not None and isinstance(r8['text'], str)
    for h in list(hs.values()) + [h8]:
        pool.close(h)


def test_config2_bucketed_batch_gpu_search_equals_host_search(tmp_path):
    """BASELINE configs[2] as bench.py runs it: squeezeformer.yml non-streaming, 64 utterances of 2-20 s in two length buckets
    of 32, V = 4233, ctc_beam_search beam 300 / top-n 40 / alpha 2.2 / beta 4.3 with a 3-gram LM -- the GPU search (side stream,
    deferred collection) against the host-thread search of the same probabilities, utterance by utterance: text ==, score 1e-3"""
    from masr_amd.decoders.lm_scorer import write_synthetic_arpa
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    V = 4233
    sd = synthetic.squeezeformer_state_dict(0, V)
    vocab = synthetic.synthetic_vocab(V)
    lm_path = write_synthetic_arpa(os.path.join(tmp_path, 'lm3.arpa'), vocab, order=3, seed=5)
    cfg, _ = _squeezeformer_beam_cfg(tmp_path, V, 300, lm_path)
    pred = MASRPredictor(configs=cfg, use_gpu=True, state_dict=sd)
    rng = np.random.default_rng(1234)
    lens = rng.integers(32000, 320001, 64)
    pcm = synthetic.synthetic_pcm(64, int(lens.max()), seed=1234)
    audio = [pcm[i, :lens[i]].copy() for i in range(64)]
    dec = pred.beam_search_decoder
    assert dec.gpu_search_supported(498, V)
    # the shipped alpha 2.2 / beta 4.3 (on these noise posteriors the scorer keeps the transcripts short), then a setting that
    # rewards characters (long transcripts: hundreds of trie extensions per utterance)
    longest = []
    for alpha, beta in ((2.2, 4.3), (0.2, 8.0)):
        dec.alpha, dec.beta = alpha, beta
        dec.use_gpu_search = True
        gpu = pred.predict_batch(audio, batch_size=32)
        dec.use_gpu_search = False
        host = pred.predict_batch(audio, batch_size=32)
        longest.append(max(len(r['text']) for r in gpu))
        for g, h in zip(gpu, host):
            assert g['text'] == h['text']
            assert abs(g['score'] - h['score']) < 1e-3 * max(1.0, abs(h['score'])), (g['score'], h['score'])
    assert longest[1] > 50, longest


def test_auxiliary_engine_is_per_device():
    """runtime.aux_engine(): one weight-less engine per GPU (the decoders' vocabulary pruning / prefix search / collapse run on the
    device their inputs live on; round 3's process-wide engine sent the worker thread of GPU k to whichever device came first)"""
    from masr_amd import runtime
    a = runtime.aux_engine()
    assert a is runtime.aux_engine(torch.cuda.current_device()) and a is runtime.aux_engine(torch.device('cuda', torch.cuda.current_device()))
    assert a.device.index == torch.cuda.current_device()
    if torch.cuda.device_count() > 1:
        b = runtime.aux_engine(1)
        assert b is not a and b.device.index == 1 and runtime.aux_engine(torch.device('cuda', 1)) is b


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs (one beam-search predictor per GPU behind the router)')
def test_two_gpu_server_with_beam_search_predictors(tmp_path):
    """advisor finding of round 3: create_app(predictors=[one per GPU]) with ctc_beam_search predictors -- every worker thread
    searches on ITS GPU's auxiliary engine; both workers return what their own predictor returns when called directly"""
    from concurrent.futures import wait
    from masr_amd.predict import MASRPredictor
    from masr_amd.server import EngineWorker, WorkerRouter
    from masr_amd.utils import synthetic
    vpath = os.path.join(tmp_path, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(512):
            f.write(f'{t}\t1\n')
    cfg = yaml.safe_load(CONFIG.replace('VOCAB', vpath))
    cfg['decoder'] = 'ctc_beam_search'
    cfg['ctc_beam_search_decoder_conf'] = {'alpha': 0, 'beta': 0, 'beam_size': 50, 'cutoff_prob': 0.99, 'cutoff_top_n': 20,
                                           'num_processes': 2, 'language_model_path': None}
    preds = []
    for dev in (0, 1):
        torch.cuda.set_device(dev)
        preds.append(MASRPredictor(configs=cfg, use_gpu=True, state_dict=synthetic.conformer_state_dict(0, 512)))
    torch.cuda.set_device(0)
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    clips = [pcm[:48000], pcm[20000:90000], pcm[60000:120000], pcm[:100000]]
    router = WorkerRouter([EngineWorker(p, None, max_batch=2, max_wait_ms=2.0) for p in preds])
    try:
        futs = [router.recognize(c) for c in clips for _ in range(2)]
        wait(futs, timeout=120)
        got = [f.result() for f in futs]
    finally:
        router.shutdown()
    torch.cuda.set_device(0)
    want = [preds[0].predict(c) for c in clips for _ in range(2)]
    for g_, w_ in zip(got, want):
        assert g_['text'] == w_['text'] and abs(g_['score'] - w_['score']) < 1e-2


def test_two_lanes_of_one_engine_equal_one_lane(tmp_path, monkeypatch):
    """masr_select_lane: two passes in flight on two streams of ONE engine (two workspace sets, one set of weights) give the rows
    each pass gives alone on lane 0 -- bit-identical -- whichever lane runs which pass; then the facade: predict_batch in three
    length-sorted passes with MASR_LANES=2 (the default without a GPU prefix search) and =1 returns the same transcripts and scores, greedy and GPU prefix search."""
    from masr_amd.decoders.lm_scorer import write_synthetic_arpa
    from masr_amd.engine import HipEngine
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    V = 4233
    sd = synthetic.squeezeformer_state_dict(0, V)
    eng = HipEngine(sd, {}, streaming=False, use_model='squeezeformer')
    rng = np.random.default_rng(7)
    lens = np.sort(rng.integers(32000, 200001, 24).astype(np.int32))[::-1].copy()
    pcm = synthetic.synthetic_pcm(24, int(lens.max()), seed=7)
    passes = []
    for lo in (0, 12):
        sel = lens[lo:lo + 12]
        x = torch.from_numpy(np.ascontiguousarray(pcm[lo:lo + 12, :int(sel.max())])).to(eng.device)
        for i in range(12):
            x[i, int(sel[i]):] = 0
        n = torch.from_numpy(sel.copy()).to(eng.device)
        passes.append((x, n, eng.host_gains(x, n, -20.0)))
    def valid(rows):          # tokens | count | score bits: what lies behind a row's count is not written
        r = rows.cpu().numpy()
        return [(r[i, :r[i, -2]].tolist(), int(r[i, -2]), int(r[i, -1])) for i in range(r.shape[0])]
    alone = [valid(eng.transcribe_rows(x, n, True, -20.0, gain_in=g)) for x, n, g in passes]
    assert sum(c for rows in alone for _, c, _ in rows) > 0
    streams = [torch.cuda.current_stream(eng.device), eng.side_stream(4)]
    streams[1].wait_stream(streams[0])
    for order in ((0, 1), (1, 0), (0, 1)):
        outs = {}
        for k, lane in enumerate(order):
            x, n, g = passes[k]
            eng.select_lane(lane)
            with torch.cuda.stream(streams[lane]):
                outs[k] = eng.transcribe_rows(x, n, True, -20.0, gain_in=g)
        eng.select_lane(0)
        torch.cuda.synchronize()
        for k in (0, 1):
            assert valid(outs[k]) == alone[k], (order, k)
    with pytest.raises(Exception):
        eng.select_lane(2)
    eng.close()
    # a FRESH Conformer engine builds its packed weight copies on first use, on the calling stream: the first call ever runs on
    # lane 1 / the side stream, the second one right behind it on lane 0 / the main stream must wait for the packing launches
    csd = synthetic.conformer_state_dict(0, V)
    want = None
    for first_lane in (None, 1):
        ce = HipEngine(csd, {}, vocab_size=V, streaming=True, use_model='conformer')
        x, n, _ = passes[1]
        g = ce.host_gains(x, n, -20.0)
        main, side = torch.cuda.current_stream(ce.device), ce.side_stream(4)
        torch.cuda.synchronize()
        if first_lane is None:
            rows = [valid(ce.transcribe_rows(x, n, True, -20.0, gain_in=g)) for _ in range(2)]
        else:
            side.wait_stream(main)
            ce.select_lane(1)
            with torch.cuda.stream(side):
                r1 = ce.transcribe_rows(x, n, True, -20.0, gain_in=g)
            ce.select_lane(0)
            r0 = ce.transcribe_rows(x, n, True, -20.0, gain_in=g)
            torch.cuda.synchronize()
            rows = [valid(r1), valid(r0)]
        if want is None:
            want = rows[0]
        assert rows[0] == want and rows[1] == want, first_lane
        ce.close()

    audio = [pcm[i, :lens[i]].copy() for i in range(24)]
    vocab = synthetic.synthetic_vocab(V)
    lm_path = write_synthetic_arpa(os.path.join(tmp_path, 'lm3.arpa'), vocab, order=3, seed=5)
    cfg, _ = _squeezeformer_beam_cfg(tmp_path, V, 100, lm_path)
    for decoder in ('ctc_greedy', 'ctc_beam_search'):
        cfg['decoder'] = decoder
        pred = MASRPredictor(configs=cfg, use_gpu=True, state_dict=sd)
        got = {}
        for lanes in ('2', '1', '2'):
            monkeypatch.setenv('MASR_LANES', lanes)
            got.setdefault(lanes, []).append(pred.predict_batch(audio, batch_size=8))
        assert got['2'][0] == got['1'][0] == got['2'][1], decoder
        assert sum(len(r['text']) for r in got['2'][0]) > 0
        pred.predictor.engine.close()


def test_conformer_passes_on_two_lanes_equal_one_lane(predictor, monkeypatch):
    """predict_batch of the (streaming-trained) Conformer facade in four length-sorted passes, one of them holding an utterance too
    short for a feature frame: two lanes (default) and one lane return identical results, in input order"""
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    rng = np.random.default_rng(3)
    audio = [pcm[o:o + n].copy() for o, n in zip(rng.integers(0, 40000, 11), rng.integers(9000, 90000, 11))]
    audio.insert(4, pcm[:200].copy())                      # 200 samples: no frame -> empty transcript, like the reference's failure mode
    got = {}
    for lanes in ('2', '1', '2'):
        monkeypatch.setenv('MASR_LANES', lanes)
        got.setdefault(lanes, []).append(predictor.predict_batch(audio, batch_size=3))
    assert got['2'][0] == got['1'][0] == got['2'][1]
    assert got['2'][0][4] == {'text': '', 'score': 0} and sum(len(r['text']) for r in got['2'][0]) > 0
    assert predictor.predictor.engine.lane == 0


@pytest.mark.parametrize('family', ['conformer', 'efficient_conformer', 'squeezeformer', 'deepspeech2'])
def test_lanes_with_growing_ragged_passes_every_family(family):
    """eight ragged passes of growing and shrinking size alternate over the two lanes of one engine (every workspace of both sets
    is reallocated at least once while the other lane has work in flight); each pass must give the rows it gives on a fresh
    engine's lane 0, for every model family (the DeepSpeech2 workspaces are part of the sets too)"""
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    V = 300
    make = {'conformer': lambda: HipEngine(synthetic.conformer_state_dict(0, V), {}, vocab_size=V, streaming=True, use_model='conformer'),
            'efficient_conformer': lambda: HipEngine(synthetic.efficient_conformer_state_dict(0, V), {}, vocab_size=V, streaming=True,
                                                     use_model='efficient_conformer'),
            'squeezeformer': lambda: HipEngine(synthetic.squeezeformer_state_dict(0, V), {}, vocab_size=V, streaming=False,
                                               use_model='squeezeformer'),
            'deepspeech2': lambda: HipEngine(synthetic.deepspeech2_state_dict(0, V, bidirectional=True), vocab_size=V, streaming=False,
                                             use_model='deepspeech2')}[family]
    rng = np.random.default_rng(11)
    sizes = [(2, 30000), (5, 60000), (3, 20000), (9, 90000), (1, 120000), (12, 40000), (4, 150000), (6, 50000)]
    pcm = synthetic.synthetic_pcm(12, 150000, seed=11)

    def valid(rows):
        r = rows.cpu().numpy()
        return [(r[i, :r[i, -2]].tolist(), int(r[i, -2]), int(r[i, -1])) for i in range(r.shape[0])]
    ref_eng, eng = make(), make()
    try:
        passes = []
        for B, n_max in sizes:
            lens = np.sort(rng.integers(n_max // 3, n_max + 1, B).astype(np.int32))[::-1].copy()
            lens[0] = n_max
            x = torch.from_numpy(np.ascontiguousarray(pcm[:B, :n_max])).to(eng.device)
            for i in range(B):
                x[i, int(lens[i]):] = 0
            n = torch.from_numpy(lens).to(eng.device)
            g = ref_eng.host_gains(x, n, -20.0)
            passes.append((x, n, g, valid(ref_eng.transcribe_rows(x, n, True, -20.0, gain_in=g))))
        assert sum(c for p in passes for _, c, _ in p[3]) > 0
        streams = [torch.cuda.current_stream(eng.device), eng.side_stream(4)]
        streams[1].wait_stream(streams[0])
        for rep in range(2):
            outs = []
            for k, (x, n, g, _) in enumerate(passes):
                lane = (k + rep) & 1
                eng.select_lane(lane)
                with torch.cuda.stream(streams[lane]):
                    outs.append(eng.transcribe_rows(x, n, True, -20.0, gain_in=g))
            eng.select_lane(0)
            torch.cuda.synchronize()
            for k, (_, _, _, want) in enumerate(passes):
                assert valid(outs[k]) == want, (family, rep, k)
    finally:
        ref_eng.close()
        eng.close()


def test_deferred_passes_return_what_predict_batch_returns(predictor):
    """MASRPredictor.predict_batch_deferred: three passes launched back to back (they alternate over the engine's two lanes), then
    collected in order and out of order -- each returns exactly what predict_batch returns for its list"""
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    rng = np.random.default_rng(9)
    lists = [[pcm[o:o + n].copy() for o, n in zip(rng.integers(0, 40000, k), rng.integers(9000, 90000, k))] for k in (5, 3, 7)]
    lists[1].append(pcm[:100].copy())                      # no frame: the empty transcript
    want = [predictor.predict_batch(a) for a in lists]
    for order in ((0, 1, 2), (2, 0, 1)):
        fetch = [predictor.predict_batch_deferred(a) for a in lists]
        got = {k: fetch[k]() for k in order}
        assert [got[k] for k in range(3)] == want, order
    assert predictor.predictor.engine.lane == 0


def test_stream_sessions_step_between_deferred_passes(predictor):
    """a server's mixed load on one engine: offline batches launched as deferred passes (alternating over the two lanes) with
    stream-pool steps in between, nothing waited for until the end -- the partial results of the sessions and the batches' results
    equal what each gives alone"""
    from masr_amd.serving import StreamPool
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    rng = np.random.default_rng(21)
    batches = [[pcm[o:o + n].copy() for o, n in zip(rng.integers(0, 30000, 6), rng.integers(20000, 100000, 6))] for _ in range(4)]
    chunks = [[pcm[10000 * k + lo:10000 * k + lo + 8000].tobytes() for lo in range(0, 48000, 8000)] for k in range(3)]

    def stream_run(pool, between=None):
        hs = [pool.open() for _ in chunks]
        outs = []
        for c in range(6):
            for k, h in enumerate(hs):
                pool.feed(h, chunks[k][c], is_end=c == 5)
            if between is not None:
                between(c)
            step = pool.step()
            outs.append([step[h] for h in hs])
        for h in hs:
            pool.close(h)
        return outs
    want_batches = [predictor.predict_batch(b) for b in batches]
    pool = StreamPool(predictor)
    want_stream = stream_run(pool)
    fetches = []
    got_stream = stream_run(pool, between=lambda c: fetches.append(predictor.predict_batch_deferred(batches[c])) if c < 4 else None)
    got_batches = [f() for f in fetches]
    pool.shutdown()
    assert got_stream == want_stream
    assert got_batches == want_batches
    assert any(r is not None and r['text'] for step in got_stream for r in step)
