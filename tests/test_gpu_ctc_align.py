"""GPU: CTC forced alignment (masr_ctc_align, csrc/ctc_align.hip) and the token timestamps built on it.

Op level with ``input_is_log=1``: the kernel only adds and compares float32 values, so start / end / peak / score / status must equal
the float32 numpy restatement (tests/ctc_align_ref.py) TO THE BIT, at the smallest shapes where the kernel can go wrong: the
workgroup is 256 threads (states loop beyond), a wave 64, the LDS rows hold S <= 2 * 1024 + 1.  With ``input_is_log=0`` (the
kernel takes the logarithm of masr_ctc_probs' probabilities itself) the float64 budget rule of tests/budget.py holds, C = 8 unchanged.
End to end: ``timestamps=True`` through MASRPredictor for each of the four decoders."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import budget            # noqa: E402
import ctc_align_ref as ar            # noqa: E402

pytestmark = pytest.mark.gpu

V = 50
DEC = dict(linear_units=384, num_blocks=2, r_num_blocks=2)
DEC_CONF = dict(attention_heads=4, **DEC)
ENC_CONF = dict(num_blocks=2, linear_units=256)
WORKGROUP, MAX_TOKENS = 256, 1024


def _log_softmax32(x):
    x = np.asarray(x, np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)


def _hyp(rng, L, vocab):
    """L ids in [1, vocab) with exactly two adjacent repeats (L >= 6; none below): feasible from L + 2 frames on"""
    h = rng.integers(1, vocab, L)
    for i in range(1, L):
        while h[i] == h[i - 1]:
            h[i] = rng.integers(1, vocab)
    if L >= 6:
        for i in (1, L // 2 + 1):
            h[i] = h[i - 1]
            while i + 1 < L and (h[i + 1] == h[i] or (i + 2 < L and h[i + 1] == h[i + 2])):
                h[i + 1] = rng.integers(1, vocab)
        assert sum(a == b for a, b in zip(h, h[1:])) == 2
    return h.astype(np.int32)


@pytest.fixture(scope='module')
def bare():
    """a weight-less engine: the alignment needs no model"""
    from masr_amd.engine import HipEngine
    e = HipEngine(None, vocab_size=V)
    yield e
    e.close()


def _run(eng, post, n_frames, tokens, n_tokens, is_log=True):
    dev = eng.device
    out = eng.ctc_align(torch.from_numpy(np.ascontiguousarray(post, np.float32)).to(dev),
                        torch.tensor(np.asarray(n_frames), dtype=torch.int32, device=dev),
                        torch.from_numpy(np.ascontiguousarray(tokens, np.int32)).to(dev),
                        torch.tensor(np.asarray(n_tokens), dtype=torch.int32, device=dev), input_is_log=is_log)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, name):
    for g, w, what in zip(got, want, ('start', 'end', 'peak', 'score', 'status')):
        assert g.dtype == w.dtype and np.array_equal(_bits(g), _bits(w)), f'{name}: {what}\n{g}\n{w}'


def _check(eng, post, n_frames, tokens, n_tokens, name):
    got = _run(eng, post, n_frames, tokens, n_tokens)
    _same(got, ar.align_batch(post, n_frames, tokens, n_tokens, np.float32), name)
    return got


def _single(eng, rng, T, hyp, vocab, name, Tp=None):
    """one utterance of T valid frames (padded to Tp with NaN) and hypothesis ``hyp``"""
    Tp = Tp or max(T, 1)
    post = np.full((1, Tp, vocab), np.nan, np.float32)
    post[0, :T] = _log_softmax32(rng.standard_normal((T, vocab)) * 3)
    tok = np.zeros((1, max(len(hyp), 1)), np.int32)
    tok[0, :len(hyp)] = hyp
    return _check(eng, post, [T], tok, [len(hyp)], name)


def test_smallest_trellises(bare):
    rng = np.random.default_rng(1)
    assert _single(bare, rng, 1, [], 5, "T'=1 L=0")[4][0] == 0
    got = _single(bare, rng, 1, [3], 5, "T'=1 L=1")
    assert got[4][0] == 0 and got[0][0, 0] == 0 and got[1][0, 0] == 0
    got = _single(bare, rng, 5, [], 5, "T'=5 L=0")
    assert got[4][0] == 0 and got[0][0, 0] == -1
    got = _single(bare, rng, 6, [1, 2, 3, 4, 5, 6], 8, "T'=L distinct")             # the diagonal is the only path
    assert got[0][0].tolist() == [0, 1, 2, 3, 4, 5] and got[1][0].tolist() == [0, 1, 2, 3, 4, 5]
    got = _single(bare, rng, 3, [2, 2], 5, "a a at T'=3")                              # token, blank, token
    assert got[4][0] == 0 and got[0][0].tolist() == [0, 2]
    got = _single(bare, rng, 2, [2, 2], 5, "a a at T'=2")
    assert got[4][0] == 1 and got[0][0].tolist() == [-1, -1] and got[3][0] == 0
    got = _single(bare, rng, 4, [1, 2, 3, 4, 1], 6, "L = T'+1", Tp=8)
    assert got[4][0] == 1
    assert _single(bare, rng, 0, [], 5, 'no frames, no tokens', Tp=3)[4][0] == 0
    assert _single(bare, rng, 0, [1], 5, 'no frames, one token', Tp=3)[4][0] == 1


@pytest.mark.parametrize('L', [31, 32, (WORKGROUP - 2) // 2, WORKGROUP // 2, MAX_TOKENS])
def test_states_around_a_wave_the_workgroup_and_the_lds_rows(bare, L):
    """S = 63 / 65 (a wave), 255 / 257 (S is odd: one less and one more than the workgroup of 256), 2049 (the largest accepted)"""
    rng = np.random.default_rng(L)
    got = _single(bare, rng, L + 3, _hyp(rng, L, V), V, f'L={L}')
    assert got[4][0] == 0


def test_refusals_by_name(bare):
    from masr_amd._lib import MasrError
    rng = np.random.default_rng(2)
    T = MAX_TOKENS + 4
    post = _log_softmax32(rng.standard_normal((1, T, 4)))
    with pytest.raises(MasrError, match='MASR_ALIGN_MAX_TOKENS'):
        _run(bare, post, [T], np.ones((1, MAX_TOKENS + 1), np.int32), [MAX_TOKENS + 1])
    with pytest.raises(MasrError, match="Lmax 6 > T' 5"):
        _run(bare, post[:, :5], [5], np.ones((1, 6), np.int32), [3])
    with pytest.raises(MasrError, match='V > 16384'):
        _run(bare, np.zeros((1, 2, 16385), np.float32), [2], np.ones((1, 1), np.int32), [1])


def test_ragged_batch_equals_each_utterance_alone_on_either_lane(bare):
    """B = 5, mixed n_frames (one 0) and n_tokens; NaN in every padded frame, ids -1 and V in every padded token slot"""
    rng = np.random.default_rng(3)
    Tp, Lmax = 23, 9
    n_frames, n_tokens = [23, 11, 0, 17, 5], [9, 4, 0, 0, 5]
    post = np.full((5, Tp, V), np.nan, np.float32)
    tokens = np.where(rng.integers(0, 2, (5, Lmax)) == 0, -1, V).astype(np.int32)
    for b in range(5):
        post[b, :n_frames[b]] = _log_softmax32(rng.standard_normal((n_frames[b], V)) * 3)
        tokens[b, :n_tokens[b]] = _hyp(rng, n_tokens[b], V)
    tokens[4, :5] = [7, 7, 7, 8, 8]                       # 5 frames < 5 + 3: no path
    got = _check(bare, post, n_frames, tokens, n_tokens, 'ragged')
    assert got[4].tolist() == [0, 0, 0, 0, 1]
    for b in range(5):
        L = max(n_tokens[b], 1)
        one = _run(bare, post[b:b + 1, :max(n_frames[b], L)], n_frames[b:b + 1], tokens[b:b + 1, :L], n_tokens[b:b + 1])
        for g, o in zip(got, one):
            assert np.array_equal(_bits(g[b:b + 1].reshape(1, -1)[:, :o.reshape(1, -1).shape[1]]), _bits(o.reshape(1, -1))), b
    bare.select_lane(1)                                    # its own predecessor workspace
    try:
        _same(_run(bare, post, n_frames, tokens, n_tokens), got, 'lane 1')
    finally:
        bare.select_lane(0)
    # lengths out of range and ids outside [1, V) inside a hypothesis are reported, not read
    bad = tokens.copy()
    bad[0, 2] = V
    bad[1, 0] = 0
    st = _run(bare, post, [24, 11, 0, 17, 5], bad, [9, 4, 0, 10, 5])[4]
    assert st.tolist() == [2, 2, 0, 2, 1]


def test_vocabulary_edges(bare):
    rng = np.random.default_rng(4)
    big = 16384
    got = _single(bare, rng, 7, [1, big - 1, big - 1, 1], big, 'V=16384')
    assert got[4][0] == 0
    got = _single(bare, rng, 6, [1, 1, 1], 2, 'V=2')
    assert got[4][0] == 0


def test_exact_ties_follow_the_tie_rule(bare):
    rng = np.random.default_rng(5)
    # every log-probability equal: every path ties
    post = np.full((1, 9, 6), -1.75, np.float32)
    got = _check(bare, post, [9], [[1, 2, 2, 3]], [4], 'all equal')
    assert got[4][0] == 0 and got[0][0].tolist() == [0, 1, 3, 4]
    # two frames equal only in the columns the hypothesis reads (blank, 2, 4); the others differ
    post = _log_softmax32(rng.standard_normal((1, 8, 6)) * 2)
    post[0, 4, [0, 2, 4]] = post[0, 3, [0, 2, 4]]
    post[0, 5, [0, 2, 4]] = post[0, 3, [0, 2, 4]]
    _check(bare, post, [8], [[2, 4, 2]], [3], 'rows equal in the hypothesis columns')
    # the end tie: the last blank and the last token as likely on every frame
    post = _log_softmax32(rng.standard_normal((1, 5, 4)))
    post[0, :, 0] = post[0, :, 3]
    _check(bare, post, [5], [[1, 3]], [2], 'end tie')


def test_random_rows_eight_seeds_in_one_batch(bare):
    T, L = 40, 12
    post = np.stack([_log_softmax32(np.random.default_rng(s).standard_normal((T, V)) * 4) for s in range(8)])
    tokens = np.stack([_hyp(np.random.default_rng(100 + s), L, V) for s in range(8)])
    got = _check(bare, post, [T] * 8, tokens, [L] * 8, 'random')
    assert (got[4] == 0).all()


# ---- input_is_log = 0: the probabilities of masr_ctc_probs, float64 budget ----------------------------------------------------------
def _sd():
    from masr_amd.utils import synthetic
    import json
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rescoring_v50.npz'))
    return synthetic.conformer_state_dict(json.loads(str(z['recipe']))['seed'], V, d_ff=256, num_blocks=2, decoder=DEC)


@pytest.fixture(scope='module')
def sd():
    return _sd()


@pytest.fixture(scope='module')
def probs(sd):
    """the synthetic Conformer's CTC probabilities for 3 utterances (T' = 49, 32, 16), computed once -> (engine, device tensor,
    numpy, valid frames)"""
    from masr_amd.engine import HipEngine
    e = HipEngine(sd, encoder_conf=ENC_CONF, vocab_size=V)
    rng = np.random.default_rng(3)
    lens = np.array([199, 131, 67], np.int32)
    feats = (rng.standard_normal((3, 199, 80)) * 3 + 13).astype(np.float32)
    for b in range(3):
        feats[b, lens[b]:] = 0
    enc = e.encode_full(torch.from_numpy(feats).to(e.device), torch.from_numpy(lens).to(e.device), -1)
    p = e.ctc_probs(enc)
    torch.cuda.synchronize()
    yield e, p, p.cpu().numpy(), np.asarray(e.enc_frames(lens)).astype(np.int32)
    e.close()


def _greedy_tokens(p, n):
    best = p[:n].argmax(axis=-1)
    keep = np.concatenate([[True], best[1:] != best[:-1]])
    return best[keep & (best != 0)].astype(np.int32)


def _budget_case(eng, p_dev, p, n_frames, hyps, name):
    """-> (figures of the score check, per-utterance truth / GPU results).  Truth: float64 restatement over the float64 log;
    reference: float32 restatement over numpy's float32 log; the GPU's path is valued in the truth's log-probabilities."""
    B = p.shape[0]
    Lmax = max(1, max(len(h) for h in hyps))
    tokens = np.zeros((B, Lmax), np.int32)
    for b, h in enumerate(hyps):
        tokens[b, :len(h)] = h
    n_tok = np.array([len(h) for h in hyps], np.int32)
    dev = eng.device
    got = [t.cpu().numpy() for t in eng.ctc_align(p_dev, torch.from_numpy(n_frames).to(dev), torch.from_numpy(tokens).to(dev),
                                                  torch.from_numpy(n_tok).to(dev), input_is_log=False)]
    with np.errstate(divide='ignore'):
        lp64 = [np.maximum(np.log(p[b, :n_frames[b]].astype(np.float64)), ar.NEG) for b in range(B)]
        lp32 = [np.maximum(np.log(p[b, :n_frames[b]]), np.float32(ar.NEG)) for b in range(B)]
    t64 = [ar.align(lp64[b], hyps[b], np.float64) for b in range(B)]
    t32 = [ar.align(lp32[b], hyps[b], np.float32) for b in range(B)]
    assert all(t['status'] == 0 for t in t64) and (got[4] == 0).all(), name
    f = budget.check(name + ' score', [t['score'] for t in t64], [t['score'] for t in t32], got[3])
    for b in range(B):
        L = len(hyps[b])
        for path, who in ((t32[b]['path'], 'float32 restatement'),
                          (ar.states_from_spans(got[0][b], got[1][b], n_frames[b], L), 'GPU')):
            # a valid alignment of the hypothesis, short of the truth's optimum by at most twice the bar: each of the two paths is
            # off the truth by at most the bar (the restatement must hold this itself, or the utterance is no case for the test)
            assert ar.path_is_valid(path, hyps[b]), (name, b, who)
            short = float(t64[b]['score'] - ar.path_score(lp64[b], path, hyps[b]))
            print(f'ALIGN {name} utterance {b} {who}: short of the optimum by {short:.3e}, 2 x bar {2 * f["bar_max"]:.3e}', flush=True)
            assert -1e-9 <= short <= 2 * f['bar_max'], (name, b, who, short)
        for j in range(L):          # peak: the kernel's own log of the token's largest probability over its frames
            want = np.log(p[b, got[0][b, j]:got[1][b, j] + 1, hyps[b][j]].astype(np.float64)).max()
            assert abs(got[2][b, j] - want) <= budget.C * budget.ULP32 * max(1.0, abs(want)), (name, b, j)
    return f, t64, got, lp64


def test_probabilities_of_the_ctc_head_hold_the_float64_budget(probs):
    eng, p_dev, p, n_frames = probs
    rng = np.random.default_rng(8)
    greedy = [_greedy_tokens(p[b], n_frames[b]) for b in range(3)]
    _budget_case(eng, p_dev, p, n_frames, greedy, 'greedy hypotheses')
    # hypotheses the head did not choose (what an attention decoder may hand over), with repeats
    other = [_hyp(rng, min(9, int(n_frames[b]) // 3), V) for b in range(3)]
    _budget_case(eng, p_dev, p, n_frames, other, 'foreign hypotheses')


def test_greedy_tokens_align_to_the_frame_maxima(probs):
    """no oracle: the best path over ALL labellings is the per-frame argmax, and it collapses to the greedy tokens -- so their
    aligned score is the sum over the valid frames of the log of the frame maximum, and on frames whose top-2 log margin exceeds
    twice the bar the path's label IS the argmax (start / end are the run boundaries of the per-frame argmax)"""
    eng, p_dev, p, n_frames = probs
    greedy = [_greedy_tokens(p[b], n_frames[b]) for b in range(3)]
    f, t64, got, lp64 = _budget_case(eng, p_dev, p, n_frames, greedy, 'greedy')
    sums64 = [float(lp64[b].max(axis=-1).sum()) for b in range(3)]
    sums32 = []
    for b in range(3):
        acc = np.float32(0)
        for v in np.log(p[b, :n_frames[b]].max(axis=-1)):
            acc = np.float32(acc + v)
        sums32.append(acc)
    g = budget.check('greedy score = sum of log frame maxima', sums64, sums32, got[3])
    checked = 0
    for b in range(3):
        assert abs(float(t64[b]['score']) - sums64[b]) <= 1e-9 * max(1.0, abs(sums64[b]))
        safe = budget.argmax_margin(lp64[b], max(g['bar_max'], f['bar_max']) / budget.C)
        labels = ar.labels_of(ar.states_from_spans(got[0][b], got[1][b], n_frames[b], len(greedy[b])), greedy[b])
        best = lp64[b].argmax(axis=-1)
        for t in np.nonzero(safe)[0]:
            assert labels[t] == best[t], (b, t)
        checked += int(safe.sum())
    assert checked > 0


# ---- masr_frame_reduction -------------------------------------------------------------------------------------------------------
def _family_engines():
    from masr_amd.utils import synthetic
    yield 'conformer', dict(), synthetic.conformer_state_dict(1, V, d_ff=256, num_blocks=1), dict(encoder_conf=dict(num_blocks=1, linear_units=256)), 4
    for il, r in (('conv2d6', 6), ('conv2d8', 8)):
        yield f'conformer {il}', dict(), synthetic.conformer_state_dict(1, V, d_ff=256, num_blocks=1, input_layer=il), \
            dict(encoder_conf=dict(num_blocks=1, linear_units=256, input_layer=il)), r
    yield 'squeezeformer', dict(use_model='squeezeformer', streaming=False), synthetic.squeezeformer_state_dict(2, V, num_blocks=12), dict(), 4
    yield 'efficient_conformer', dict(use_model='efficient_conformer'), synthetic.efficient_conformer_state_dict(2, V, num_blocks=12), dict(), 8


def test_frame_reduction_agrees_with_encoder_frames():
    import ctypes as C
    from masr_amd._lib import check
    from masr_amd.engine import HipEngine
    seen = []
    for name, kw, sd_, more, want in _family_engines():
        e = HipEngine(sd_, vocab_size=V, **kw, **more)
        try:
            r = e.frame_reduction()
            assert r == want, (name, r)
            for F in (1000, 1003, 4999):
                a, b = C.c_int32(), C.c_int32()
                check(e.lib.masr_encoder_frames(e.h, F, C.byref(a)))
                check(e.lib.masr_encoder_frames(e.h, F + r, C.byref(b)))
                assert b.value - a.value == 1, (name, F)
                assert e.out_frames(F) == a.value
            seen.append(name)
        finally:
            e.close()
    assert len(seen) == 5


def test_frame_reduction_deepspeech2():
    import ctypes as C
    from masr_amd._lib import check
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sd_ = synthetic.deepspeech2_state_dict(3, V, rnn_size=256, num_rnn_layers=1, bidirectional=False)
    e = HipEngine(sd_, vocab_size=V, use_model='deepspeech2', encoder_conf=dict(rnn_size=256, num_rnn_layers=1))
    try:
        assert e.frame_reduction() == 4
        a, b = C.c_int32(), C.c_int32()
        check(e.lib.masr_encoder_frames(e.h, 1001, C.byref(a)))
        check(e.lib.masr_encoder_frames(e.h, 1005, C.byref(b)))
        assert b.value - a.value == 1
    finally:
        e.close()


# ---- end to end through the facade ----------------------------------------------------------------------------------------------
def _cfg(tmp_path, decoder):
    from masr_amd.utils import synthetic
    vpath = os.path.join(tmp_path, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(V):
            f.write(f'{t}\t1\n')
    return {'encoder_conf': dict(ENC_CONF), 'decoder_conf': dict(DEC_CONF), 'model_conf': {'ctc_weight': 0.3, 'reverse_weight': 0.3},
            'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                                'use_dB_normalization': True, 'target_dB': -20},
            'attention_decoder_conf': {'beam_size': 4},
            'attention_rescoring_decoder_conf': {'beam_size': 4, 'ctc_weight': 0.5},
            'ctc_beam_search_decoder_conf': {'alpha': 0, 'beta': 0, 'beam_size': 8, 'cutoff_prob': 0.99, 'cutoff_top_n': 20,
                                             'num_processes': 2, 'language_model_path': None},
            'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'conformer', 'streaming': True, 'decoder': decoder,
            'metrics_type': 'cer'}


LENS = [24000, 17000, 300]            # the last one is too short for a frame
FRAME_S = 0.04                        # one encoder frame of the conv2d front end


def _check_tokens(res, seconds, may_lack_a_path=False):
    if res['text'] == '':
        assert res['tokens'] == []
        return
    toks = res['tokens']
    if toks is None:
        # only a hypothesis the CTC head did not produce, and only when the trellis really has no path for it: it holds the blank
        # id, or more tokens plus adjacent repeats than the utterance has encoder frames (the vocabulary's other tokens are
        # single characters)
        frames = 1 + (int(round(seconds * 16000)) - 400) // 160
        enc_frames = ((frames - 1) // 2 - 1) // 2
        assert may_lack_a_path
        if '<blank>' in res['text']:            # an attention decoder may emit id 0, which no CTC path can carry (status 2)
            return
        text = res['text'].replace('<unk>', '\x01').replace('<eos>', '\x02')
        assert len(text) + sum(a == b for a, b in zip(text, text[1:])) > enc_frames, (text, enc_frames)
        return
    assert toks is not None and ''.join(t['token'] for t in toks) == res['text']
    last = 0.0
    for t in toks:
        assert 0 <= t['start'] < t['end'] <= seconds + 1e-9 and t['start'] >= last and 0 < t['score'] <= 1.0 + 1e-6, t
        last = t['start']


@pytest.mark.parametrize('decoder', ['ctc_greedy', 'ctc_beam_search', 'attention_rescoring', 'attention'])
def test_timestamps_through_the_predictor(tmp_path, sd, decoder):
    from masr_amd.data_utils.audio import AudioSegment
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    pred = MASRPredictor(configs=_cfg(str(tmp_path), decoder), use_gpu=True, state_dict=sd)
    pcm = synthetic.synthetic_pcm(3, max(LENS), seed=5)
    audio = [pcm[i, :n].copy() for i, n in enumerate(LENS)]
    plain = pred.predict_batch(audio)
    timed = pred.predict_batch(audio, timestamps=True)
    assert all('tokens' not in r for r in plain) and len(timed) == 3
    for r0, r1, n in zip(plain, timed, LENS):
        assert r1['text'] == r0['text'] and r1['score'] == r0['score'], (decoder, r0, r1)
        _check_tokens(r1, n / 16000.0, may_lack_a_path=decoder in ('attention', 'attention_rescoring'))
    assert timed[2] == {'text': '', 'score': 0, 'tokens': []}
    # the longest utterance has no padding in its batch: alone (predict) it gets the same tokens on the same frames
    one = pred.predict(audio_data=audio[0], timestamps=True)
    assert one['text'] == timed[0]['text']
    assert [(t['token'], t['start'], t['end']) for t in one['tokens'] or []] == [(t['token'], t['start'], t['end']) for t in timed[0]['tokens'] or []]
    # the deferred form, twice: consecutive calls alternate over the engine's lanes -- the same results either way
    first = pred.predict_batch_deferred(audio, timestamps=True)
    second = pred.predict_batch_deferred(audio, timestamps=True)
    assert first() == timed and second() == timed
    assert pred.predict_batch_deferred(audio)() == plain
    # the same samples given at 8 kHz: times are seconds of the utterance
    low = (np.sin(np.arange(12000) * 0.37) * 0.1 + np.random.default_rng(7).standard_normal(12000) * 0.05).astype(np.float32)
    seg = AudioSegment.from_ndarray(low.copy(), 8000)
    seg.resample(16000)
    at8 = pred.predict(audio_data=low, sample_rate=8000, timestamps=True)
    at16 = pred.predict(audio_data=np.asarray(seg.samples, np.float32), sample_rate=16000, timestamps=True)
    assert at8['text'] == at16['text'] and len(at8['tokens'] or []) == len(at16['tokens'] or [])
    _check_tokens(at8, 1.5, may_lack_a_path=decoder in ('attention', 'attention_rescoring'))
    for a, b in zip(at8['tokens'] or [], at16['tokens'] or []):
        assert abs(a['start'] - b['start']) <= FRAME_S and abs(a['end'] - b['end']) <= FRAME_S
    with pytest.raises(Exception, match='sharded path'):
        pred.predict_batch(audio, timestamps=True, distributed=True)
