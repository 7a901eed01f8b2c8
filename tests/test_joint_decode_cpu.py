"""CPU: ``decoder: joint`` without a device -- the CTC prefix recursion against a brute-force sum over all alignments, the joint
search restatement (tests/joint_decode_ref.py) against the attention one and on hand-made tables, ``validate_joint_conf``, the
refusals of the predictor and of the C ABI, and the safety cap of the GPU search-parity test's inputs."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_decode_ref as ar            # noqa: E402
import budget            # noqa: E402
import ctc_prefix_ref as cp            # noqa: E402
import fake_engine            # noqa: E402
import joint_decode_ref as jr            # noqa: E402
import rescoring_ref as rr            # noqa: E402
from masr_amd import _lib            # noqa: E402
from masr_amd.decoders import joint_decoder as jd            # noqa: E402
from masr_amd.utils import synthetic            # noqa: E402

V = 64            # the model of the GPU tests (tests/test_gpu_joint_decode.py)
VS = 50           # a vocabulary below 64 for the configuration checks
DEC = dict(linear_units=384, num_blocks=2, r_num_blocks=2)


@pytest.fixture(scope='module')
def sd():
    return synthetic.conformer_state_dict(11, V, d_ff=256, num_blocks=2, decoder=DEC)


# ---- the recursion against all V^T alignments --------------------------------------------------------------------------------------
def _posteriors(T, Vt, seed):
    p = np.random.default_rng(seed).random((T, Vt)) + 0.05
    return p / p.sum(axis=1, keepdims=True)


@pytest.mark.parametrize('T,Vt', [(1, 4), (2, 3), (3, 4), (4, 4), (5, 3)])
def test_recursion_equals_the_brute_force_sum(T, Vt):
    """every prefix of length <= 3 (tokens other than blank and eos) followed by every token: the extension's psi is the summed
    probability of the alignments that start with it, eos gives the whole-sequence probability, blank -inf; a prefix longer than
    the frames can carry (T < |g| + 1, or a repeat that needs a blank between) comes out as exactly -inf"""
    p = _posteriors(T, Vt, 7 * T + Vt)
    lp, eos = cp.log_post(p), Vt - 1
    seen_inf = seen_repeat = 0
    for L in range(4):
        for g in itertools.product(range(1, eos), repeat=L):
            psi_g, psi_c = cp.prefix_scores(lp, list(g), list(range(Vt)))
            want_g = cp.brute_force(p, g)
            assert (psi_g == want_g == -np.inf) or abs(psi_g - want_g) <= 1e-12, (g, psi_g, want_g)
            for c in range(Vt):
                want = -np.inf if c == 0 else cp.brute_force(p, g, whole=True) if c == eos else cp.brute_force(p, list(g) + [c])
                if want == -np.inf:
                    assert psi_c[c] == -np.inf, (g, c)
                    seen_inf += c not in (0, eos)
                else:
                    assert abs(psi_c[c] - want) <= 1e-12, (g, c, psi_c[c], want)
                    seen_repeat += L > 0 and c == g[-1]
    assert seen_inf > 0 or T >= 5
    assert seen_repeat > 0 or T < 3


def test_too_few_frames_is_exactly_minus_infinity():
    lp = cp.log_post(_posteriors(2, 4, 1))
    assert cp.prefix_scores(lp, [1, 2], [1, 2])[1].tolist() == [-np.inf, -np.inf]          # T = |g| < |g| + 1
    assert cp.prefix_scores(lp, [1], [1])[1][0] == -np.inf                                 # 1 1 needs a blank between: three frames
    assert np.isfinite(cp.prefix_scores(lp, [1], [2])[1][0])
    lp0 = cp.log_post(np.array([[0.5, 0.5, 0.0, 0.0]], np.float32))
    assert cp.prefix_scores(lp0, [], [1, 2, 3, 0])[1].tolist() == [np.log(0.5), -np.inf, np.log(0.5), -np.inf]


def test_float32_restatement_stays_close():
    p = _posteriors(40, 6, 3).astype(np.float32)
    a = cp.prefix_scores(cp.log_post(p, np.float64), [1, 2, 2, 3], list(range(6)))
    b = cp.prefix_scores(cp.log_post(p, np.float32), [1, 2, 2, 3], list(range(6)))
    assert b[1].dtype == np.float32 and np.abs(a[1][1:] - b[1][1:]).max() < 1e-4 and abs(a[0] - b[0]) < 1e-4


# ---- the search ---------------------------------------------------------------------------------------------------------------------
def test_no_ctc_no_bonus_is_the_attention_search_decision_for_decision(sd):
    mem = np.random.default_rng(0).standard_normal((12, 256)).astype(np.float32)
    sd64 = rr.to64(sd)
    for s in (sd64, sd):
        a = ar.search(s, mem, 4)
        j = jr.search(s, mem, None, 4, 4, 0.0, 0.0, dtype=np.float64 if s is sd64 else np.float32)
        assert j['trace'] == [(p, t, [float(x) for x in sc]) for p, t, sc in a['trace']]
        assert j['hyps'] == [(h, float(x)) for h, x in a['hyps']] and j['steps'] == a['steps']


def _peaked(tokens, Vt, T, blanks=1):
    """posteriors peaked on ``tokens`` with ``blanks`` blank frames between them"""
    path = []
    for t in tokens:
        path += [t] + [0] * blanks
    path += [0] * (T - len(path))
    p = np.full((T, Vt), 0.02 / (Vt - 1))
    for t, s in enumerate(path):
        p[t, s] = 0.98
    return p


def test_the_ctc_score_keeps_a_search_going_that_the_attention_alone_ends():
    """a hand-made table: the attention prefers eos at step 1; the posteriors are peaked on 2 2 3 (a repeat).  ctc_weight 0 gives
    the empty transcript, 0.5 the string"""
    Vt, eos = 6, 5

    def logp(toks):
        return np.log(np.array([0.02, 0.1, 0.1, 0.1, 0.08, 0.6]))
    lp = cp.log_post(_peaked([2, 2, 3], Vt, 8))
    mem = np.zeros((8, 1))
    r0 = jr.search(None, mem, lp, 2, 4, 0.0, 0.0, logp_fn=logp, vocab=Vt)
    assert r0['hyps'][0][0] == [] and r0['steps'] == 2
    r5 = jr.search(None, mem, lp, 2, 4, 0.5, 0.0, logp_fn=logp, vocab=Vt)
    assert r5['hyps'][0][0] == [2, 2, 3]
    att, psi = r5['parts'][0]
    assert np.isclose(att, 3 * np.log(0.1) + np.log(0.6)) and np.isclose(r5['hyps'][0][1], 0.5 * att + 0.5 * psi)
    assert np.isclose(psi, cp.brute_force(np.exp(lp), [2, 2, 3], whole=True))


def test_the_length_bonus_alone_lengthens_the_result():
    Vt = 6

    def logp(toks):
        return np.log(np.array([0.02, 0.3, 0.1, 0.1, 0.08, 0.4]))
    mem = np.zeros((5, 1))
    r0 = jr.search(None, mem, None, 2, 2, 0.0, 0.0, logp_fn=logp, vocab=Vt)
    r1 = jr.search(None, mem, None, 2, 2, 0.0, 1.5, logp_fn=logp, vocab=Vt)
    assert r0['hyps'][0][0] == [] and len(r1['hyps'][0][0]) > 0
    # ln 0.3 + 1.5 > 0 > ln 0.4: every further token 1 raises the key, up to the limit (returned unfinished, as it stands)
    assert r1['hyps'][0][0] == [1] * 5 and np.isclose(r1['hyps'][0][1], 5 * (np.log(0.3) + 1.5))


# ---- configuration and refusals -----------------------------------------------------------------------------------------------------
def test_joint_conf_defaults_fallback_and_refusals():
    assert jd.validate_joint_conf(None) == {'beam_size': 10, 'max_len': 0, 'ctc_weight': 0.3, 'length_bonus': 0.0, 'ctc_candidates': 20}
    assert jd.validate_joint_conf({}, {'ctc_weight': 0.5})['ctc_weight'] == 0.5
    assert jd.validate_joint_conf({}, {'ctc_weight': 1.0})['ctc_weight'] == 0.3
    assert jd.validate_joint_conf({}, {'ctc_weight': 'x'})['ctc_weight'] == 0.3
    assert jd.validate_joint_conf({'ctc_weight': 0}, {'ctc_weight': 0.5})['ctc_weight'] == 0.0
    assert jd.validate_joint_conf({'beam_size': 40})['ctc_candidates'] == 64
    assert jd.validate_joint_conf({'beam_size': 30}, None, VS)['ctc_candidates'] == VS
    got = jd.validate_joint_conf({'beam_size': 4, 'max_len': 7, 'ctc_weight': 0.7, 'length_bonus': -1, 'ctc_candidates': 4}, None, VS)
    assert got == {'beam_size': 4, 'max_len': 7, 'ctc_weight': 0.7, 'length_bonus': -1.0, 'ctc_candidates': 4}
    with pytest.raises(_lib.MasrError, match='joint_decoder_conf.reverse_weight is not a known key'):
        jd.validate_joint_conf({'reverse_weight': 0.5})
    for beam in (0, 65, True, 2.0, '4'):
        with pytest.raises(_lib.MasrError, match='joint_decoder_conf.beam_size'):
            jd.validate_joint_conf({'beam_size': beam})
    with pytest.raises(_lib.MasrError, match='exceeds the vocabulary of 50'):
        jd.validate_joint_conf({'beam_size': 51}, None, VS)
    for max_len in (-1, 1.5, False):
        with pytest.raises(_lib.MasrError, match='joint_decoder_conf.max_len'):
            jd.validate_joint_conf({'max_len': max_len})
    for w in (1.0, -0.1, 1.5, True, '0.3', None, float('nan')):
        with pytest.raises(_lib.MasrError, match='joint_decoder_conf.ctc_weight'):
            jd.validate_joint_conf({'ctc_weight': w})
    for g in (float('inf'), float('nan'), False, '1'):
        with pytest.raises(_lib.MasrError, match='joint_decoder_conf.length_bonus'):
            jd.validate_joint_conf({'length_bonus': g})
    for m in (3, 65, True, 8.0):
        with pytest.raises(_lib.MasrError, match='joint_decoder_conf.ctc_candidates'):
            jd.validate_joint_conf({'beam_size': 4, 'ctc_candidates': m})
    with pytest.raises(_lib.MasrError, match='joint_decoder_conf.ctc_candidates'):
        jd.validate_joint_conf({'beam_size': 4, 'ctc_candidates': 51}, None, VS)
    for text in (jd.STREAM_REFUSAL, jd.DS2_REFUSAL, jd.DECODE_REFUSAL, jd.NBEST_REFUSAL):
        assert "decoder='joint'" in text


def test_c_abi_refuses_by_name_before_it_needs_a_device():
    lib = _lib.lib()
    err = lambda: lib.masr_last_error().decode()
    buf = np.ones(64, np.int32)
    p = buf.ctypes.data_as(C.c_void_p)
    dec = lambda B, Tp, N, M, lam, gam, max_len, lcap, post=p: lib.masr_joint_decode(None, p, p, B, Tp, post, 0, N, M, lam, gam, max_len,
                                                                                     p, lcap, p, p, None, None, None, None)
    assert dec(1, 4, 0, 4, 0.3, 0.0, 0, 4) != 0 and 'beam_size = 0 is outside 1 .. 64' in err()
    assert dec(1, 4, 65, 65, 0.3, 0.0, 0, 4) != 0 and 'beam_size = 65 is outside 1 .. 64' in err()
    assert dec(1, 4, 4, 3, 0.3, 0.0, 0, 4) != 0 and 'ctc_candidates = 3 is outside beam_size .. 64' in err()
    assert dec(1, 4, 4, 65, 0.3, 0.0, 0, 4) != 0 and 'ctc_candidates = 65' in err()
    assert dec(1, 4, 4, 4, 1.0, 0.0, 0, 4) != 0 and 'ctc_weight' in err()
    assert dec(1, 4, 4, 4, float('nan'), 0.0, 0, 4) != 0 and 'ctc_weight' in err()
    assert dec(1, 4, 4, 4, 0.3, float('inf'), 0, 4) != 0 and 'length_bonus' in err()
    assert dec(1, 4, 4, 4, 0.3, 0.0, 0, 4, None) != 0 and 'post_dev' in err()
    assert dec(1, 4, 4, 4, 0.3, 0.0, 0, 0) != 0 and 'Lcap must be at least 1' in err()
    assert dec(1024, 4, 64, 64, 0.3, 0.0, 0, 4) != 0 and 'must not exceed 65535' in err()
    assert dec(1, 4, 4, 4, 0.3, 0.0, -1, 4) != 0 and 'max_len' in err()
    assert dec(1, 4, 4, 4, 0.3, 0.0, 0, 4) != 0 and err() == 'engine not finalized'
    op = lambda R, L, M: lib.masr_op_ctc_prefix_scores(None, p, 0, p, 1, 4, p, p, p, R, L, p, M, p, p, None)
    assert op(0, 1, 1) != 0 and 'R = 0' in err()
    assert op(1, 0, 1) != 0 and 'L must be at least 1' in err()
    assert op(1, 1, 65) != 0 and 'M = 65' in err()
    assert op(1, 1, 1) != 0 and err() == 'engine not finalized'


def _stub(decoder, use_model='conformer'):
    from masr_amd.utils.utils import dict_to_object
    return dict_to_object({'streaming': True, 'use_model': use_model, 'decoder': decoder})


def test_streams_decode_and_nbest_refuse_the_decoder_by_name():
    from masr_amd.infer_utils.inference_predictor import InferencePredictor
    from masr_amd.predict import MASRPredictor
    from masr_amd.serving import StreamPool

    class Stub:
        configs = _stub('joint')
    with pytest.raises(Exception) as err:
        StreamPool(Stub())
    assert str(err.value) == jd.STREAM_REFUSAL and 'unknown decoder' not in str(err.value)
    pred = object.__new__(MASRPredictor)
    pred.configs, pred._pool = Stub.configs, None
    # (an engine that computes nothing stands behind the predictor: no refusal may reach it)
    pred.predictor = object.__new__(InferencePredictor)
    pred.predictor.engine = fake_engine.make('conformer', None, V)
    with pytest.raises(Exception) as err:
        pred.predict_stream(b'\x00' * 3200)
    assert str(err.value) == jd.STREAM_REFUSAL and pred._pool is None
    with pytest.raises(Exception) as err:
        pred.decode(np.zeros((4, V), np.float32), False, False)
    assert str(err.value) == jd.DECODE_REFUSAL
    for call in (lambda: pred.predict(np.zeros(16000, np.float32), nbest=2), lambda: pred.predict_batch([np.zeros(16000, np.float32)], nbest=2),
                 lambda: pred.predict_batch_deferred([np.zeros(16000, np.float32)], nbest=2)):
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == jd.NBEST_REFUSAL.format(nbest=2)
    assert pred.predictor.engine.calls == 0


def test_deepspeech2_is_refused_before_anything_is_loaded(tmp_path):
    from masr_amd.predict import MASRPredictor
    vpath = os.path.join(tmp_path, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(V):
            f.write(f'{t}\t1\n')
    cfg = {'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'deepspeech2', 'streaming': True, 'decoder': 'joint',
           'metrics_type': 'cer'}
    with pytest.raises(Exception) as err:
        MASRPredictor(configs=cfg, use_gpu=True, state_dict={})
    assert str(err.value) == jd.DS2_REFUSAL
    cfg.update(use_model='conformer', joint_decoder_conf={'ctc_weight': 1.0})
    with pytest.raises(_lib.MasrError, match='joint_decoder_conf.ctc_weight'):
        MASRPredictor(configs=cfg, use_gpu=True, state_dict={})


def test_inference_predictor_asks_for_the_decoder_for_joint(monkeypatch, sd):
    from masr_amd.infer_utils import inference_predictor as ip
    from masr_amd.utils.utils import dict_to_object
    seen = {}

    class Engine:
        def __init__(self, state_dict, **kw):
            seen.update(kw)
    monkeypatch.setattr(ip, 'HipEngine', Engine)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    dconf = dict(attention_heads=4, **DEC)
    cfg = dict_to_object({'decoder': 'joint', 'encoder_conf': {'num_blocks': 2}, 'decoder_conf': dconf, 'preprocess_conf': {}})
    ip.InferencePredictor(configs=cfg, use_model='conformer', streaming=True, state_dict=sd)
    assert seen['attention_decoder'] is True and dict(seen['decoder_conf']) == dconf


# ---- the end-to-end inputs ------------------------------------------------------------------------------------------------------------
def test_end_to_end_safety_cap_holds_for_the_float32_restatement(sd):
    """the cap of the GPU search-parity test for ITS inputs (joint_decode_ref.E2E), on the CPU: the utterances through the oracle's
    features, encoder and CTC head; 18 .. 32 frames, all different; for every (ctc_weight, length_bonus) of the grid at most 2 of
    the 8 float64 searches have an unsafe step, and on the safe ones the float32 search returns the float64 one's hypotheses"""
    from oracle import conformer as oc, fbank as ofb
    E = jr.E2E
    pcm = synthetic.synthetic_pcm(len(E['lens']), max(E['lens']), seed=E['pcm_seed'])
    feats = [ofb.featurize_pcm16(pcm[i, :n])[0] for i, n in enumerate(E['lens'])]
    T = max(f.shape[0] for f in feats)
    batch = np.zeros((len(feats), T, 80), np.float32)
    for i, f in enumerate(feats):
        batch[i, :f.shape[0]] = f
    frames = [f.shape[0] for f in feats]
    with torch.no_grad():
        enc = oc.encoder_full(sd, torch.from_numpy(batch), torch.tensor(frames), -1).numpy()
    valid = [oc.subsampled_len(f) for f in frames]
    assert min(valid) >= 18 and max(valid) <= 32 and len(set(valid)) == 8
    sd64 = rr.to64(sd)
    safe = {g: 0 for g in E['grid']}
    for b in range(len(feats)):
        mem = enc[b, :valid[b]]
        post = np.exp(jr.log_posteriors(sd, mem, np.float32))            # float32 probabilities, as the CTC head leaves them
        memo = ({}, {})
        fns = [lambda toks, s=s, c=c: c.setdefault(tuple(toks), ar.step_logp(s, mem, toks)) for s, c in zip((sd64, sd), memo)]
        for lam, gam in E['grid']:
            r64 = jr.search(None, mem, cp.log_post(post, np.float64), E['beam_size'], E['ctc_candidates'], lam, gam, logp_fn=fns[0],
                            vocab=V)
            r32 = jr.search(None, mem, cp.log_post(post, np.float32), E['beam_size'], E['ctc_candidates'], lam, gam, logp_fn=fns[1],
                            vocab=V, dtype=np.float32)
            e_ref, unsafe = ar.safety(r64, r32, budget.C)
            print(f'joint E2E (CPU) utterance {b} lam {lam} gamma {gam}: limit {r64["limit"]}, steps {r64["steps"]}, min margin '
                  f'{min(r64["margins"]):.3e}, 2 C max|e_ref| {2 * budget.C * e_ref:.3e}, first unsafe step {unsafe}')
            if unsafe is None:
                safe[(lam, gam)] += 1
                assert [h for h, _ in r32['hyps']] == [h for h, _ in r64['hyps']]
    assert all(n >= 6 for n in safe.values()), safe
