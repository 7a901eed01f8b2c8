"""``nbest=N`` at the public surface (MASRPredictor.predict / predict_batch / predict_batch_deferred / predict_stream) and
``attention_rescoring_decoder_conf.first_pass: 'gpu'``, on a synthetic two-block Conformer with a 50-word vocabulary and 1 - 1.5 s of
audio."""
import numpy as np
import pytest
import torch

from tests.test_gpu_rescoring import V, _cfg, _sd

pytestmark = pytest.mark.gpu

BEAM_CONF = {'alpha': 0, 'beta': 0, 'beam_size': 8, 'cutoff_prob': 0.99, 'cutoff_top_n': 40, 'num_processes': 2,
             'language_model_path': None}
LENS = (24000, 17000, 20000)


@pytest.fixture(scope='module')
def sd():
    return _sd()


@pytest.fixture(scope='module')
def audio():
    from masr_amd.utils import synthetic
    pcm = synthetic.synthetic_pcm(len(LENS), max(LENS), seed=21)
    return [pcm[i, :n].copy() for i, n in enumerate(LENS)]


@pytest.fixture(scope='module')
def pred(tmp_path_factory, sd):
    from masr_amd.predict import MASRPredictor
    tmp = str(tmp_path_factory.mktemp('nbest'))
    return MASRPredictor(configs=_cfg(tmp, 'ctc_beam_search', ctc_beam_search_decoder_conf=dict(BEAM_CONF)), use_gpu=True, state_dict=sd)


def _entry0(res):
    assert set(res) == {'text', 'score', 'nbest'} and 1 <= len(res['nbest']) <= 3
    assert all(set(e) == {'text', 'score'} for e in res['nbest'])
    assert res['nbest'][0] == {'text': res['text'], 'score': res['score']}
    scores = [e['score'] for e in res['nbest']]
    assert scores == sorted(scores, reverse=True) and len({e['text'] for e in res['nbest']}) == len(scores)


def test_predict_and_predict_batch_with_and_without_nbest(pred, audio):
    one, one_n = pred.predict(audio_data=audio[0]), pred.predict(audio_data=audio[0], nbest=3)
    assert set(one) == {'text', 'score'} and (one_n['text'], one_n['score']) == (one['text'], one['score'])
    _entry0(one_n)
    plain, many = pred.predict_batch(audio), pred.predict_batch(audio, nbest=3)
    deferred = pred.predict_batch_deferred(audio, nbest=3)()
    for p, m, d in zip(plain, many, deferred):
        assert set(p) == {'text', 'score'} and (m['text'], m['score']) == (p['text'], p['score'])
        _entry0(m)
        assert d == m
    stamped = pred.predict(audio_data=audio[0], nbest=3, timestamps=True)
    assert stamped['nbest'] == one_n['nbest'] and stamped['text'] == one['text'] and 'tokens' in stamped
    with pytest.raises(ValueError, match=r'nbest must be an integer in 1 \.\. beam_size = 8'):
        pred.predict(audio_data=audio[0], nbest=9)
    with pytest.raises(ValueError, match='sharded path'):
        pred.predict_batch(audio, nbest=3, distributed=True)


def test_predict_stream_with_nbest_at_the_end_of_the_utterance(pred, audio):
    from masr_amd._lib import MasrError
    raw = audio[0].tobytes()
    pred.reset_stream()
    half = (len(raw) // 4) * 2
    pred.predict_stream(raw[:half], nbest=3)
    with pytest.raises(MasrError, match='the first call of an utterance decides'):
        pred.predict_stream(raw[half:], is_end=True)
    res = pred.predict_stream(raw[half:], is_end=True, nbest=3)
    _entry0(res)
    pred.reset_stream()
    plain = pred.predict_stream(raw[:half])
    plain = pred.predict_stream(raw[half:], is_end=True)
    assert set(plain) == {'text', 'score'} and (plain['text'], plain['score']) == (res['text'], res['score'])
    pred.reset_stream()


def test_first_pass_gpu_rescoring_reads_the_gpu_nbest(tmp_path, sd, audio):
    from masr_amd.decoders.attention_rescoring import combine
    from masr_amd.predict import MASRPredictor
    conf = {'beam_size': 4, 'ctc_weight': 0.5, 'first_pass': 'gpu'}
    p = MASRPredictor(configs=_cfg(str(tmp_path), 'attention_rescoring', attention_rescoring_decoder_conf=conf), use_gpu=True,
                      state_dict=sd)
    dec = p.rescoring_decoder
    assert dec.first_pass == 'gpu'
    seen = {}
    inner_nbest, inner_launch = dec.nbest, dec.rescore_launch

    def spy_nbest(probs, frames):
        seen['probs'], seen['frames'] = probs.clone(), np.array(frames)
        return inner_nbest(probs, frames)

    def spy_launch(eng_, enc, enc_lens, nbest):
        collect = inner_launch(eng_, enc, enc_lens, nbest)

        def collect_and_record():
            seen['nbest'], seen['out'] = nbest, collect()
            return seen['out']
        return collect_and_record
    dec.nbest, dec.rescore_launch = spy_nbest, spy_launch
    res = p.predict_batch(audio)
    # the hypotheses handed to the second pass are the GPU search's n-best of this pass's posteriors, to the bit
    direct = dec._pruner._batch(seen['probs'], frames=seen['frames'], want_tokens=True, nbest=4)
    assert seen['nbest'] == direct and all(1 <= len(h) <= 4 for h in direct)
    for r, h, (toks, score, w, (att, r_att, total)) in zip(res, seen['nbest'], seen['out']):
        ctc = np.array([s for _, s in h], np.float32)
        want = combine(att, r_att, ctc, dec.ctc_weight, dec.reverse_weight)
        assert total.dtype == np.float64 and np.array_equal(total, want) and w == int(np.argmax(want))
        assert toks == h[w][0] and r['score'] == float(want[w]) and r['text'] == p._text(toks)


def test_first_pass_gpu_and_host_pick_the_same_winner_on_a_peaked_posterior(tmp_path, sd):
    """a posterior with one dominant symbol per frame: both first passes give the second pass the same leading hypotheses, and the
    rescoring over the same encoder rows picks the same winner"""
    from masr_amd.decoders.attention_rescoring import AttentionRescoringDecoder
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    p = MASRPredictor(configs=_cfg(str(tmp_path), 'attention_rescoring'), use_gpu=True, state_dict=sd)
    eng = p.predictor.engine
    rng = np.random.default_rng(4)
    B, Ts = 2, 40
    ids = rng.integers(0, V - 1, (B, Ts))
    ids[rng.random((B, Ts)) < 0.5] = 0
    probs = np.full((B, Ts, V), 1e-4, np.float32)
    for b in range(B):
        probs[b, np.arange(Ts), ids[b]] = 1.0 - 1e-4 * (V - 1)
    frames = np.array([Ts, Ts - 9], np.int32)
    dev = torch.from_numpy(probs).to(eng.device)
    enc = torch.from_numpy(rng.normal(0, 1, (B, Ts, 256)).astype(np.float32)).to(eng.device)
    enc_lens = torch.from_numpy(frames).to(eng.device)
    vocab = synthetic.synthetic_vocab(V)
    won = {}
    for first_pass in ('host', 'gpu'):
        dec = AttentionRescoringDecoder(vocab, beam_size=4, ctc_weight=0.5, reverse_weight=0.3, first_pass=first_pass)
        nbest = dec.nbest(dev, frames)
        won[first_pass] = (nbest, dec.rescore(eng, enc, enc_lens, nbest))
    for b in range(B):
        (hn, hr), (gn, gr) = won['host'], won['gpu']
        assert gn[b][0][0] == hn[b][0][0] and abs(gn[b][0][1] - hn[b][0][1]) <= 1e-3 * max(1.0, abs(hn[b][0][1]))
        assert gr[b][0] == hr[b][0], (gr[b], hr[b])
