"""CPU: ``decoder: joint`` with a language model (``language_model_path`` / ``lm_weight``) without a device --
``validate_joint_conf`` and the decoder's constructor over the new keys, the refusals of masr_joint_decode_lm and
masr_op_lm_scores, the restatement of the fused search (tests/joint_lm_ref.py) against the LM-free one and on a hand-made case in
which the model changes the winner, and the safety cap of the GPU search-parity test's inputs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_decode_ref as ar            # noqa: E402
import budget            # noqa: E402
import ctc_prefix_ref as cp            # noqa: E402
import joint_decode_ref as jr            # noqa: E402
import joint_lm_ref as jl            # noqa: E402
import rescoring_ref as rr            # noqa: E402
from masr_amd import _lib            # noqa: E402
from masr_amd.decoders import joint_decoder as jd            # noqa: E402
from masr_amd.decoders.lm_scorer import LanguageModel, write_synthetic_word_arpa            # noqa: E402

V = jl.V


@pytest.fixture(scope='module')
def sd():
    return jl.state_dict()


# ---- configuration ------------------------------------------------------------------------------------------------------------------
def test_joint_conf_takes_the_language_model_keys_and_refuses_by_name():
    base = {'beam_size': 10, 'max_len': 0, 'ctc_weight': 0.3, 'length_bonus': 0.0, 'ctc_candidates': 20}
    assert jd.validate_joint_conf({'language_model_path': 'lm/zh.arpa'}) == dict(base, language_model_path='lm/zh.arpa', lm_weight=0.3)
    assert jd.DEFAULT_LM_WEIGHT == 0.3
    got = jd.validate_joint_conf({'language_model_path': 'lm/zh.arpa', 'lm_weight': 1})
    assert got['lm_weight'] == 1.0 and isinstance(got['lm_weight'], float)
    # a path with lm_weight 0 loads nothing; no path: the default weight is 0
    assert jd.validate_joint_conf({'language_model_path': 'lm/zh.arpa', 'lm_weight': 0}) == dict(base, language_model_path=None, lm_weight=0.0)
    assert jd.validate_joint_conf({'language_model_path': None}) == dict(base, language_model_path=None, lm_weight=0.0)
    assert jd.validate_joint_conf({'lm_weight': 0.0}) == dict(base, language_model_path=None, lm_weight=0.0)
    with pytest.raises(_lib.MasrError, match='joint_decoder_conf.lm_weight=0.5 needs joint_decoder_conf.language_model_path'):
        jd.validate_joint_conf({'lm_weight': 0.5})
    for w in (-0.1, float('inf'), float('nan'), True, '0.3', None):
        with pytest.raises(_lib.MasrError, match='joint_decoder_conf.lm_weight'):
            jd.validate_joint_conf({'language_model_path': 'lm/zh.arpa', 'lm_weight': w})
    for path in (True, 3, '', ['a']):
        with pytest.raises(_lib.MasrError, match='joint_decoder_conf.language_model_path'):
            jd.validate_joint_conf({'language_model_path': path})
    with pytest.raises(_lib.MasrError, match='joint_decoder_conf.reverse_weight is not a known key'):
        jd.validate_joint_conf({'reverse_weight': 0.5, 'lm_weight': 0.0})
    with pytest.raises(_lib.MasrError, match='joint_decoder_conf.alpha is not a known key'):
        jd.validate_joint_conf({'alpha': 1.0})


def _word_model(tmp_path):
    vocab = ['<blank>', '<unk>', '<space>', 'a', 'b', 'c', '<eos>']
    path = write_synthetic_word_arpa(os.path.join(tmp_path, 'words.arpa'), ['ab', 'ca', 'b'], order=2, seed=1, n_higher=6)
    return LanguageModel(path, vocab), vocab


def test_the_decoder_refuses_a_word_based_model_a_missing_one_and_a_missing_file(tmp_path):
    lm, vocab = _word_model(str(tmp_path))
    assert not lm.is_character_based
    with pytest.raises(_lib.MasrError, match='is a word-based language model'):
        jd.JointDecoder(vocab, beam_size=2, language_model=lm, lm_weight=0.3)
    with pytest.raises(_lib.MasrError, match='is a word-based language model'):
        jd.load_language_model(lm.path, vocab)
    with pytest.raises(_lib.MasrError, match='lm_weight=0.3 needs a language model'):
        jd.JointDecoder(vocab, beam_size=2, lm_weight=0.3)
    for w in (-1.0, float('nan'), True, '1'):
        with pytest.raises(_lib.MasrError, match='joint_decoder_conf.lm_weight'):
            jd.JointDecoder(vocab, beam_size=2, lm_weight=w)
    with pytest.raises(AssertionError, match='语言模型不存在'):
        jd.load_language_model(os.path.join(str(tmp_path), 'absent.arpa'), vocab)
    char, toks = jl.synthetic_model(os.path.join(str(tmp_path), 'c.arpa'), 20, 2, n_higher=30)
    with pytest.raises(_lib.MasrError, match='loaded for a vocabulary of 20 tokens'):
        jd.JointDecoder(toks + ['x'], beam_size=2, language_model=char, lm_weight=0.3)
    dec = jd.JointDecoder(toks, beam_size=2, language_model=char, lm_weight=0.25)
    assert dec.lm_weight == 0.25 and dec.language_model is char and dec.last_lm is None and dec.last_parts is None
    assert jd.JointDecoder(toks, beam_size=2).lm_weight == 0.0


def test_the_predictor_refuses_the_new_keys_before_anything_is_loaded(tmp_path):
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    vpath = os.path.join(tmp_path, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(V):
            f.write(f'{t}\t1\n')
    cfg = {'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'conformer', 'streaming': True, 'decoder': 'joint',
           'metrics_type': 'cer', 'joint_decoder_conf': {'lm_weight': 0.3}}
    with pytest.raises(_lib.MasrError, match='needs joint_decoder_conf.language_model_path'):
        MASRPredictor(configs=cfg, use_gpu=True, state_dict={})
    cfg['joint_decoder_conf'] = {'language_model_path': os.path.join(tmp_path, 'absent.arpa')}
    with pytest.raises(AssertionError, match='语言模型不存在'):
        MASRPredictor(configs=cfg, use_gpu=True, state_dict={})


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_by_name_before_it_needs_a_device(tmp_path):
    lib = _lib.lib()
    err = lambda: lib.masr_last_error().decode()
    buf = np.ones(64, np.int32)
    p = buf.ctypes.data_as(C.c_void_p)
    char, _ = jl.synthetic_model(os.path.join(str(tmp_path), 'c.arpa'), 20, 2, n_higher=30)
    word, _ = _word_model(str(tmp_path))

    def dec(B, Tp, N, M, lam, gam, lm, mu, max_len, lcap, post=p):
        return lib.masr_joint_decode_lm(None, p, p, B, Tp, post, 0, N, M, lam, gam, lm, mu, max_len, p, lcap, p, p, None, None, None,
                                        None, None)
    # what masr_joint_decode refuses, under the new name
    assert dec(1, 4, 0, 4, 0.3, 0.0, None, 0.0, 0, 4) != 0 and 'masr_joint_decode_lm: beam_size = 0 is outside 1 .. 64' in err()
    assert dec(1, 4, 4, 3, 0.3, 0.0, None, 0.0, 0, 4) != 0 and 'ctc_candidates = 3 is outside beam_size .. 64' in err()
    assert dec(1, 4, 4, 4, 1.0, 0.0, None, 0.0, 0, 4) != 0 and 'ctc_weight' in err()
    assert dec(1, 4, 4, 4, 0.3, float('inf'), None, 0.0, 0, 4) != 0 and 'length_bonus' in err()
    assert dec(1, 4, 4, 4, 0.3, 0.0, None, 0.0, 0, 4, None) != 0 and 'post_dev' in err()
    assert dec(1, 4, 4, 4, 0.3, 0.0, None, 0.0, 0, 0) != 0 and 'Lcap must be at least 1' in err()
    assert dec(1024, 4, 64, 64, 0.3, 0.0, None, 0.0, 0, 4) != 0 and 'must not exceed 65535' in err()
    assert dec(1, 4, 4, 4, 0.3, 0.0, None, 0.0, -1, 4) != 0 and 'max_len' in err()
    # its own
    for mu in (-0.5, float('nan'), float('inf')):
        assert dec(1, 4, 4, 4, 0.3, 0.0, char.h, mu, 0, 4) != 0 and 'masr_joint_decode_lm: lm_weight' in err()
    assert dec(1, 4, 4, 4, 0.3, 0.0, None, 0.3, 0, 4) != 0 and 'lm_weight > 0 needs a language model' in err()
    assert dec(1, 4, 4, 4, 0.3, 0.0, word.h, 0.3, 0, 4) != 0 and 'word-based language models' in err()
    assert dec(1, 4, 4, 4, 0.3, 0.0, char.h, 0.3, 0, 4) != 0 and err() == 'engine not finalized'
    assert dec(1, 4, 4, 4, 0.0, 0.0, char.h, 0.3, 0, 4, None) != 0 and err() == 'engine not finalized'      # attention + LM: no posteriors
    op = lambda lm, R, L, M: lib.masr_op_lm_scores(None, lm, p, p, p, R, L, M, p, None)
    assert op(None, 1, 1, 1) != 0 and 'masr_op_lm_scores: null argument' in err()
    assert op(char.h, 0, 1, 1) != 0 and 'R = 0' in err()
    assert op(char.h, 65536, 1, 1) != 0 and 'R = 65536' in err()
    assert op(char.h, 1, 0, 1) != 0 and 'L must be at least 1' in err()
    assert op(char.h, 1, 1, 0) != 0 and 'M = 0' in err()
    assert op(char.h, 1, 1, 65) != 0 and 'M = 65' in err()
    assert op(word.h, 1, 1, 1) != 0 and 'word-based language models' in err()
    assert op(char.h, 1, 1, 1) != 0 and err() == 'engine not finalized'


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_lm_weight_zero_is_the_joint_search_exactly(sd):
    mem = np.random.default_rng(0).standard_normal((12, 256)).astype(np.float32)
    sd64 = rr.to64(sd)
    for s, dt in ((sd64, np.float64), (sd, np.float32)):
        lp = jr.log_posteriors(sd, mem, dt)
        memo = {}
        fn = lambda toks: memo.setdefault(tuple(toks), ar.step_logp(s, mem, toks))
        for lam, gam in ((0.3, 0.5), (0.0, 0.0)):
            a = jr.search(None, mem, lp, 4, 8, lam, gam, logp_fn=fn, vocab=V, dtype=dt)
            b = jl.search(mem, lp, 4, 8, lam, 0.0, gam, fn, V, lm_fn=None, dtype=dt)          # (the model is never asked)
            assert b['trace'] == a['trace'] and b['hyps'] == a['hyps'] and b['parts'] == a['parts']
            assert b['steps'] == a['steps'] and b['margins'] == a['margins'] and b['lm'] == [0.0] * 4


HAND_VOCAB = ['<blank>', 'a', 'b', 'c', 'd', '<eos>']
HAND_ARPA = """\\data\\
ngram 1=7
ngram 2=1

\\1-grams:
-99\t<s>\t-0.3
-1.0\t</s>
-2.0\t<unk>
-1.0\ta\t-0.3
-2.5\tb\t-0.3
-1.0\tc\t-0.3
-1.0\td\t-0.3

\\2-grams:
-0.01\ta b

\\end\\
"""


def _hand_case(tmp_path):
    """attention: a first (0.9), then c (0.5) a little ahead of b (0.3), then eos; posteriors that tell b and c apart by nothing;
    a bigram model whose one bigram, a b, is strongly preferred (ln P(b | a) = -0.023 against ln P(c | a) = -2.99)"""
    path = os.path.join(str(tmp_path), 'hand.arpa')
    with open(path, 'w', encoding='utf-8') as f:
        f.write(HAND_ARPA)
    lm = LanguageModel(path, HAND_VOCAB)
    assert lm.is_character_based and lm.max_order == 2
    tables = [np.log(np.array([0.01, 0.9, 0.03, 0.025, 0.02, 0.015])), np.log(np.array([0.02, 0.03, 0.3, 0.5, 0.05, 0.1])),
              np.log(np.array([0.01, 0.02, 0.03, 0.025, 0.015, 0.9]))]
    logp = lambda toks: tables[min(len(toks), 2)]
    post = np.full((6, 6), 0.1)
    post[:, 0] = 0.5                   # blank 0.5, every token 0.1 at every frame
    return lm, logp, post


def test_a_language_model_changes_the_winner_of_a_hand_made_search(tmp_path):
    lm, logp, post = _hand_case(tmp_path)
    mem, lp = np.zeros((6, 1)), cp.log_post(post)
    fn = jl.lm_fn_of(lm, 6)
    ln10 = np.log(10.0)
    assert np.isclose(fn([1], 2), -0.01 * ln10) and np.isclose(fn([1], 3), (-0.3 - 1.0) * ln10) and np.isclose(fn([1, 2], 5), (-0.3 - 1.0) * ln10)
    for lam in (0.0, 0.3):
        r0 = jl.search(mem, lp, 2, 4, lam, 0.0, 0.0, logp, 6, lm_fn=fn)
        r1 = jl.search(mem, lp, 2, 4, lam, 0.5, 0.0, logp, 6, lm_fn=fn)
        assert r0['hyps'][0][0] == [1, 3] and r1['hyps'][0][0] == [1, 2], lam
        att, psi = r1['parts'][0]
        want_lm = float(fn([], 1)) + float(fn([1], 2)) + float(fn([1, 2], 5))
        assert np.isclose(att, np.log(0.9) + np.log(0.3) + np.log(0.9)) and np.isclose(r1['lm'][0], want_lm)
        assert np.isclose(r1['hyps'][0][1], (1 - lam) * att + lam * psi + 0.5 * want_lm)
        assert min(r1['margins']) > 1e-3


# ---- the end-to-end inputs ------------------------------------------------------------------------------------------------------------
def test_end_to_end_safety_cap_holds_for_the_float32_restatement(sd, tmp_path):
    """the cap of the GPU search-parity test for ITS inputs (joint_lm_ref.E2E_LM), on the CPU: the utterances through the oracle's
    features, encoder and CTC head; 18 .. 32 frames, all different; for every (ctc_weight, lm_weight, length_bonus) of the grid at
    most 2 of the 8 float64 searches have an unsafe step, and on the safe ones the float32 search returns the float64 one's
    hypotheses"""
    from masr_amd.utils import synthetic
    from oracle import conformer as oc, fbank as ofb
    E = jl.E2E_LM
    lm, _ = jl.synthetic_model(os.path.join(str(tmp_path), 'e2e.arpa'), V, E['arpa_order'], E['arpa_seed'], E['arpa_n_higher'])
    lm_fn = jl.lm_fn_of(lm, V)
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
        for lam, mu, gam in E['grid']:
            r64 = jl.search(mem, cp.log_post(post, np.float64), E['beam_size'], E['ctc_candidates'], lam, mu, gam, fns[0], V, lm_fn)
            r32 = jl.search(mem, cp.log_post(post, np.float32), E['beam_size'], E['ctc_candidates'], lam, mu, gam, fns[1], V, lm_fn,
                            dtype=np.float32)
            e_ref, unsafe = ar.safety(r64, r32, budget.C)
            print(f'joint LM E2E (CPU) utterance {b} lam {lam} mu {mu} gamma {gam}: limit {r64["limit"]}, steps {r64["steps"]}, min '
                  f'margin {min(r64["margins"]):.3e}, 2 C max|e_ref| {2 * budget.C * e_ref:.3e}, first unsafe step {unsafe}')
            if unsafe is None:
                safe[(lam, mu, gam)] += 1
                assert [h for h, _ in r32['hyps']] == [h for h, _ in r64['hyps']]
    assert all(n >= 6 for n in safe.values()), safe
