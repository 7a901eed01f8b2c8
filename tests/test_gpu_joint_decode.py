"""GPU: ``decoder: joint`` (masr_joint_decode / masr_op_ctc_prefix_scores, csrc/decoder_joint.hip): the CTC prefix scorer alone
against the float64 recursion (tests/ctc_prefix_ref.py) under the budget rule of tests/budget.py (C = 8 unchanged: truth = the
recursion in float64, reference = the same in float32), the search against the float64 joint search (tests/joint_decode_ref.py)
wherever its decisions are safe, bit equality with masr_attention_decode at ctc_weight 0 / length_bonus 0 / M = N, bit-for-bit
invariance of an utterance's result, and the mode end to end through MASRPredictor.

V = 64, d = 256 / 4 heads, decoder 2 + 2 blocks, linear_units 384 unless a case says otherwise."""
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
import rescoring_ref as rr            # noqa: E402

pytestmark = pytest.mark.gpu

V = 64
SEED = 11
DEC = dict(linear_units=384, num_blocks=2, r_num_blocks=2)
DEC_CONF = dict(attention_heads=4, **DEC)
ENC_CONF = dict(num_blocks=2, linear_units=256)


def _sd(vocab=V):
    from masr_amd.utils import synthetic
    return synthetic.conformer_state_dict(SEED, vocab, d_ff=256, num_blocks=2, decoder=DEC)


def _engine(sd_, vocab=V):
    from masr_amd.engine import HipEngine
    return HipEngine(sd_, encoder_conf=ENC_CONF, vocab_size=vocab, attention_decoder=True, decoder_conf=DEC_CONF)


@pytest.fixture(scope='module')
def sd():
    return _sd()


@pytest.fixture(scope='module')
def eng(sd):
    e = _engine(sd)
    yield e
    e.close()


@pytest.fixture
def poll(monkeypatch):
    def set_(n):
        monkeypatch.setenv('MASR_ATTENTION_POLL', str(n))
    return set_


# ---- the scorer alone -------------------------------------------------------------------------------------------------------------
def _post(rng, B, Tp, vocab, gain=3.0):
    z = rng.standard_normal((B, Tp, vocab)) * gain
    z[..., 0] += gain                       # blank a little likelier, as a CTC head has it
    p = np.exp(z - z.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)).astype(np.float32)


def _check_scorer(name, eng_, post, frames, rows, c_max=None):
    """``rows`` [(utterance, prefix, candidates)] through the op and through the recursion in float64 / float32: entries that are
    -inf in float64 are exactly -inf on the device, the finite ones hold the budget"""
    R, L, M = len(rows), max(1, max(len(r[1]) for r in rows)), len(rows[0][2])
    prefixes, lens = np.zeros((R, L), np.int32), np.array([len(r[1]) for r in rows], np.int32)
    for i, r in enumerate(rows):
        prefixes[i, :len(r[1])] = r[1]
    cands = np.array([r[2] for r in rows], np.int32)
    psi, psi_c = eng_.ctc_prefix_scores(torch.from_numpy(post).to(eng_.device), frames, [r[0] for r in rows], prefixes, lens, cands)
    y = np.concatenate([psi[:, None], psi_c], axis=1).astype(np.float64)
    ref = []
    for dt in (np.float64, np.float32):
        out = np.zeros((R, M + 1), np.float64)
        for i, (b, g, c) in enumerate(rows):
            a, bb = cp.prefix_scores(cp.log_post(post[b, :frames[b]], dt), g, c)
            out[i, 0], out[i, 1:] = a, bb
        ref.append(out)
    y64, y32 = ref
    inf = y64 == -np.inf
    assert np.array_equal(y == -np.inf, inf), (name, np.argwhere((y == -np.inf) != inf))
    assert np.array_equal(y32 == -np.inf, inf)
    print(f'{name}: {int(inf.sum())} of {inf.size} entries are -inf', flush=True)
    if (~inf).any():
        budget.check(name, y64[~inf], y32[~inf], y[~inf], c_max=c_max)
    return y, y64


def test_scorer_frame_count_edges(eng):
    """T = 1; T = |g| + 1 and T = |g| (all -inf but where defined); the empty prefix; a repeated last token; eos and blank among
    the candidates; three utterances of different frame counts in one call with Tp above the longest"""
    rng = np.random.default_rng(1)
    post = _post(rng, 3, 9, V)
    frames = np.array([1, 4, 3], np.int32)
    c = [0, V - 1, 5, 7, 9, 63 - 1]
    rows = [(0, [], c), (0, [5], c),                          # T = 1: the empty prefix; T = |g|: eos alone is defined
            (1, [5, 7, 9], c), (1, [5, 7, 9, 11], c),         # T = |g| + 1, T = |g|
            (1, [5, 5], c), (1, [7, 5], c), (1, [5], c),      # repeats: 5 5 + 5 needs five frames, 7 5 + 5 needs four
            (2, [], c), (2, [9, 9], c), (2, [9, 7], c), (2, [62, 5, 7], c)]
    y, y64 = _check_scorer('frame edges', eng, post, frames, rows)
    assert y[1, 1] == -np.inf and np.isfinite(y[1, 2]) and (y[1, 3:] == -np.inf).all()          # [5] at T = 1: blank, eos, tokens
    assert (y[3, 1] == -np.inf) and np.isfinite(y[3, 2]) and (y[3, 3:] == -np.inf).all()
    assert y[0, 0] == 0.0 and y[7, 0] == 0.0


def test_scorer_zero_posteriors(eng):
    rng = np.random.default_rng(2)
    post = _post(rng, 1, 7, V)
    post[0, 2, 5] = 0.0             # token 5 cannot be emitted at frame 2
    post[0, :, 9] = 0.0             # token 9 never
    post[0, 3, 0] = 0.0             # no blank at frame 3
    c = [5, 9, 0, V - 1, 7, 11]
    _check_scorer('zeros', eng, post, np.array([7], np.int32), [(0, [], c), (0, [5], c), (0, [9], c), (0, [7, 5], c), (0, [7, 7], c)])


@pytest.mark.parametrize('M', [1, 64])
def test_scorer_one_and_sixty_four_candidates(eng, M):
    rng = np.random.default_rng(3)
    post = _post(rng, 2, 12, V)
    c = [7] if M == 1 else list(range(V))
    _check_scorer(f'M={M}', eng, post, np.array([12, 10], np.int32), [(0, [3, 7], c), (1, [], c), (1, [7], c), (0, [2, 2, 9, 4], c)])


def test_scorer_vocabulary_4233():
    vocab = 4233
    e = _engine(_sd(vocab), vocab)
    try:
        rng = np.random.default_rng(4)
        post = _post(rng, 2, 40, vocab, gain=2.0)
        c = [0, vocab - 1, 1, 4231, 2048, 77, 4000, 300]
        _check_scorer('V=4233', e, post, np.array([40, 33], np.int32), [(0, [77, 4231, 4231, 9], c), (1, [], c), (1, [2048] * 3, c)])
    finally:
        e.close()


def test_scorer_three_hundred_frames(eng):
    """the error growth over the recursion: 300 frames, prefixes of 1 to 24 tokens"""
    rng = np.random.default_rng(5)
    post = _post(rng, 1, 300, V, gain=1.5)
    g = rng.integers(1, V - 1, 24).tolist()
    c = [0, V - 1] + rng.integers(1, V - 1, 6).tolist() + [g[-1], g[0]]
    _check_scorer('T=300', eng, post, np.array([300], np.int32), [(0, g[:1], c), (0, g[:8], c), (0, g, c)])


def test_scorer_refusals(eng):
    from masr_amd._lib import MasrError
    post = torch.from_numpy(_post(np.random.default_rng(0), 1, 4, V)).to(eng.device)
    z = np.zeros((1, 2), np.int32)
    with pytest.raises(MasrError, match='outside 1 .. Tp'):
        eng.ctc_prefix_scores(post, [5], [0], z, [0], [[1]])
    with pytest.raises(MasrError, match='outside 0 .. B - 1'):
        eng.ctc_prefix_scores(post, [4], [1], z, [0], [[1]])
    with pytest.raises(MasrError, match='outside 0 .. L'):
        eng.ctc_prefix_scores(post, [4], [0], z, [3], [[1]])
    for bad in (0, V - 1, V):
        with pytest.raises(MasrError, match='neither blank nor eos'):
            eng.ctc_prefix_scores(post, [4], [0], np.array([[3, bad]], np.int32), [2], [[1]])
    with pytest.raises(MasrError, match='candidate id 64'):
        eng.ctc_prefix_scores(post, [4], [0], z, [0], [[V]])


# ---- the search -------------------------------------------------------------------------------------------------------------------
def _mem(T, seed=0, d=256):
    return np.random.default_rng(seed).standard_normal((T, d)).astype(np.float32)


def _pad(items, tp, width):
    out = np.zeros((len(items), tp, width), np.float32)
    for b, m in enumerate(items):
        out[b, :len(m)] = m
    return out


def _decode(eng_, memories, posts, n, m, lam, gam, max_len=0, tp=None, lcap=None):
    """joint_decode over a list of utterances ([T_b, d] encoder rows, [T_b, V] posteriors) -> (per utterance [(tokens, J, A, psi)]
    x N, steps)"""
    B, tp = len(memories), tp or max(len(x) for x in memories)
    enc = torch.from_numpy(_pad(memories, tp, memories[0].shape[1])).to(eng_.device)
    post = None if posts is None else torch.from_numpy(_pad(posts, tp, posts[0].shape[1])).to(eng_.device)
    lens = torch.tensor([len(x) for x in memories], dtype=torch.int32).to(eng_.device)
    tokens, hl, key, att, psi, steps = eng_.joint_decode(enc, lens, post, n, m, lam, gam, max_len, lcap)
    tokens, hl, key, att, psi = (x.cpu().numpy() for x in (tokens, hl, key, att, psi))
    vocab = eng_.vocab_size
    assert ((tokens == vocab - 1) | (np.arange(tokens.shape[2])[None, None] < hl[..., None])).all()      # eos behind every length
    return [[(tokens[b, k, :hl[b, k]].tolist(), key[b, k], att[b, k], psi[b, k]) for k in range(n)] for b in range(B)], steps


def _same(a, b):
    bits = lambda x: np.float32(x).tobytes()
    return len(a) == len(b) and all(len(x) == len(y) and all(p[0] == q[0] and all(bits(u) == bits(v) for u, v in zip(p[1:], q[1:]))
                                                             for p, q in zip(x, y)) for x, y in zip(a, b))


def _refs(sd_, mem, post, n, m, lam, gam, max_len=0, fns=None):
    """the float64 and the float32 joint search over the posteriors the device reads (float32 probabilities)"""
    sd64 = rr.to64(sd_)
    fns = fns or [lambda toks, s=s: ar.step_logp(s, mem, toks) for s in (sd64, sd_)]
    vocab = post.shape[1]
    r64 = jr.search(None, mem, cp.log_post(post, np.float64), n, m, lam, gam, max_len, logp_fn=fns[0], vocab=vocab)
    r32 = jr.search(None, mem, cp.log_post(post, np.float32), n, m, lam, gam, max_len, logp_fn=fns[1], vocab=vocab, dtype=np.float32)
    return r64, r32


def _assert_search(name, got, r64, r32):
    """the device's N hypotheses against the float64 search: equal in order with J within the budget when every step is safe"""
    e_ref, unsafe = ar.safety(r64, r32)
    print(f'{name}: steps {r64["steps"]} of {r64["limit"]}, min margin {min(r64["margins"]):.3e}, 2 C max|e_ref| '
          f'{2 * budget.C * e_ref:.3e}, first unsafe step {unsafe}', flush=True)
    if unsafe is not None:
        return False
    assert [h[0] for h in got] == [h for h, _ in r64['hyps']], name
    s64 = np.array([s for _, s in r64['hyps']], np.float64)
    s = np.array([h[1] for h in got], np.float64)
    fin = np.isfinite(s64)
    assert np.array_equal(np.isfinite(s), fin)
    if not fin.any():            # (every hypothesis outgrew its frames: all keys are -inf, the order is the tie rule's)
        return True
    bar = budget.C * max(e_ref, budget.ULP32 * np.abs(s64[fin]).max())
    print(f'{name}: max |J - J64| {np.abs(s[fin] - s64[fin]).max():.3e}, bar {bar:.3e}', flush=True)
    assert np.abs(s[fin] - s64[fin]).max() <= bar, name
    return True


@pytest.fixture(scope='module')
def e2e(sd, eng):
    """the 8 utterances of joint_decode_ref.E2E through the engine's own front end, encoder and CTC head, once; the step
    log-probabilities of the restatement are remembered per utterance and prefix, the grid's searches share them"""
    from masr_amd.utils import synthetic
    E = jr.E2E
    pcm = synthetic.synthetic_pcm(8, max(E['lens']), seed=E['pcm_seed'])
    for i, n in enumerate(E['lens']):
        pcm[i, n:] = 0
    ns = torch.tensor(E['lens'], dtype=torch.int32, device=eng.device)
    feats, frames = eng.fbank_batch(torch.from_numpy(pcm).to(eng.device), ns)
    enc = eng.encode_full(feats, frames, -1)
    probs = eng.ctc_probs(enc)
    mem_lens = np.asarray(eng.enc_frames(frames.cpu().numpy())).astype(np.int32)
    assert 18 <= mem_lens.min() and mem_lens.max() <= 32 and len(set(mem_lens.tolist())) == 8
    mems = [enc[b, :mem_lens[b]].cpu().numpy() for b in range(8)]
    posts = [probs[b, :mem_lens[b]].cpu().numpy() for b in range(8)]
    sd64 = rr.to64(sd)
    fns = []
    for mem in mems:
        memo = ({}, {})
        fns.append([lambda toks, s=s, c=c, mem=mem: c.setdefault(tuple(toks), ar.step_logp(s, mem, toks)) for s, c in zip((sd64, sd), memo)])
    return dict(pcm=pcm, mems=mems, posts=posts, fns=fns, n=E['beam_size'], m=E['ctc_candidates'])


def test_no_ctc_no_bonus_is_the_attention_search_bit_for_bit(eng, e2e):
    n = e2e['n']
    tp = max(len(x) for x in e2e['mems'])
    enc = torch.from_numpy(_pad(e2e['mems'], tp, 256)).to(eng.device)
    lens = torch.tensor([len(x) for x in e2e['mems']], dtype=torch.int32).to(eng.device)
    t0, l0, s0, steps0 = eng.attention_decode(enc, lens, n)
    t1, l1, s1, a1, p1, steps1 = eng.joint_decode(enc, lens, None, n, n, 0.0, 0.0)
    assert steps0 == steps1
    assert torch.equal(t0, t1) and torch.equal(l0, l1)
    assert np.array_equal(s0.cpu().numpy().view(np.int32), s1.cpu().numpy().view(np.int32))
    assert np.array_equal(a1.cpu().numpy().view(np.int32), s1.cpu().numpy().view(np.int32)) and not p1.any()


@pytest.mark.parametrize('lam,gam', jr.E2E['grid'])
def test_search_parity_with_the_float64_joint_search(sd, eng, e2e, lam, gam):
    n, m = e2e['n'], e2e['m']
    got, _ = _decode(eng, e2e['mems'], e2e['posts'], n, m, lam, gam)
    safe = 0
    for b in range(8):
        r64, r32 = _refs(sd, e2e['mems'][b], e2e['posts'][b], n, m, lam, gam, fns=e2e['fns'][b])
        if _assert_search(f'E2E lam {lam} gamma {gam} utterance {b}', got[b], r64, r32):
            safe += 1
            # A and psi beside J: every finite key is the float32 formula of the parts that came back with it, to the bit
            for toks, key, att, psi in got[b]:
                if np.isfinite(key):
                    f = np.float32
                    want = ((f(1) - f(lam)) * att + f(lam) * psi) + f(gam) * f(len(toks))
                    assert f(want).tobytes() == f(key).tobytes(), (b, toks, key, att, psi)
    assert safe >= 6, safe


def test_posteriors_passed_by_hand_drive_the_search(sd, eng):
    """posteriors peaked on a string with a repeat, independent of the encoder rows: at ctc_weight 0.7 the device returns the
    float64 search's hypotheses, and its winner is the string"""
    mem = _mem(14, 3)
    want = [9, 9, 30, 4]
    path = [9, 0, 9, 30, 30, 0, 4] + [0] * 7
    post = np.full((14, V), 0.001 / (V - 1), np.float32)
    for t, s in enumerate(path):
        post[t, s] = 0.999
    got, _ = _decode(eng, [mem], [post], 4, V, 0.7, 0.0)
    r64, r32 = _refs(sd, mem, post, 4, V, 0.7, 0.0)
    assert r64['hyps'][0][0] == want
    assert _assert_search('peaked posteriors', got[0], r64, r32)
    assert got[0][0][0] == want
    free, _ = _decode(eng, [mem], None, 4, V, 0.0, 0.0)
    assert free[0][0][0] != want


def test_an_utterance_alone_in_a_batch_padded_on_the_other_lane_and_polled(eng, e2e, poll):
    """bit for bit: tokens, J, A, psi of an utterance's N hypotheses do not depend on B, its neighbours, the padding of Tp, the
    lane, or on how often the host polls for the end"""
    n, m = e2e['n'], e2e['m']
    run = lambda mems, posts, **kw: _decode(eng, mems, posts, n, m, 0.3, 0.5, **kw)
    full, _ = run(e2e['mems'], e2e['posts'])
    for b in (0, 7):
        alone, _ = run([e2e['mems'][b]], [e2e['posts'][b]])
        assert _same(alone, [full[b]]), b
    wide, _ = run(e2e['mems'][2:5], e2e['posts'][2:5], tp=77)
    assert _same(wide, full[2:5])
    eng.select_lane(1)
    try:
        with torch.cuda.stream(eng.side_stream(4)):
            lane1, _ = run(e2e['mems'], e2e['posts'])
    finally:
        eng.select_lane(0)
    assert _same(lane1, full)
    for every in (0, 1, 8):
        poll(every)
        polled, steps = run(e2e['mems'], e2e['posts'])
        assert _same(polled, full), every
        assert every != 0 or steps == 32


def test_max_len_cuts_the_same_search(sd, eng, e2e):
    n, m, mem, post = e2e['n'], e2e['m'], e2e['mems'][0], e2e['posts'][0]
    a, steps = _decode(eng, [mem], [post], n, m, 0.3, 0.0, max_len=5)
    assert steps == 5
    b, _ = _decode(eng, [mem], [post], n, m, 0.3, 0.0, max_len=5, lcap=32)
    c, _ = _decode(eng, [mem], [post], n, m, 0.3, 0.0, max_len=0, lcap=5)
    d, _ = _decode(eng, [mem, e2e['mems'][7][:3]], [post, e2e['posts'][7][:3]], n, m, 0.3, 0.0, max_len=5)
    assert _same(a, b) and _same(a, c) and _same(a, d[:1])
    assert all(len(h[0]) <= 3 for h in d[1])
    r64, r32 = _refs(sd, mem, post, n, m, 0.3, 0.0, max_len=5, fns=e2e['fns'][0])
    _assert_search('max_len=5', a[0], r64, r32)


@pytest.mark.parametrize('n,m', [(1, 1), (1, 6), (V, V)])
def test_beam_of_one_and_of_the_whole_vocabulary(sd, eng, n, m, poll):
    poll(1)
    mem = _mem(6, 1)
    post = _post(np.random.default_rng(9), 1, 6, V)[0]
    got, steps = _decode(eng, [mem], [post], n, m, 0.3, 0.0)
    r64, r32 = _refs(sd, mem, post, n, m, 0.3, 0.0)
    assert steps == r64['steps']
    safe = _assert_search(f'N={n} M={m}', got[0], r64, r32)
    assert safe or n == V
    if not safe:
        # thousands of candidates: some lie closer than the float32 error.  The same decisions up to the first unsafe step (the
        # search cut there by max_len), and a full beam of distinct hypotheses in descending order behind it
        _, k = ar.safety(r64, r32)
        assert k > 1
        cut, _ = _decode(eng, [mem], [post], n, m, 0.3, 0.0, max_len=k - 1)
        c64, _ = _refs(sd, mem, post, n, m, 0.3, 0.0, max_len=k - 1)
        assert [h[0] for h in cut[0]] == [h for h, _ in c64['hyps']]
        s = np.array([h[1] for h in got[0]])
        assert (np.diff(s[np.isfinite(s)]) <= 0).all() and len({tuple(h[0]) + (i,) * (not np.isfinite(h[1])) for i, h in enumerate(got[0])}) == n


def test_raised_eos_bias_finished_rows_and_early_stop(sd, poll):
    sd2 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
    sd2['decoder.left_decoder.output_layer.bias'][V - 1] += 16.0
    e = _engine(sd2)
    try:
        mem = _mem(20, 0)
        post = _post(np.random.default_rng(6), 1, 20, V, gain=1.0)[0]
        r64, r32 = _refs(sd2, mem, post, 4, 8, 0.3, 0.0)
        assert r64['steps'] < r64['limit']
        poll(1)
        got, steps = _decode(e, [mem], [post], 4, 8, 0.3, 0.0)
        assert _assert_search('eos bias', got[0], r64, r32)
        assert steps == r64['steps']
        poll(0)                      # never polled: the steps up to the limit change nothing
        again, steps = _decode(e, [mem], [post], 4, 8, 0.3, 0.0)
        assert steps == r64['limit'] and _same(again, got)
    finally:
        e.close()


def test_workspace_is_counted_and_refusals_on_a_live_engine(sd, eng):
    from masr_amd._lib import MasrError
    enc = torch.zeros(1, 4, 256, device=eng.device)
    post = torch.full((1, 4, V), 1.0 / V, device=eng.device)
    lens = torch.tensor([4], dtype=torch.int32, device=eng.device)
    before = eng.decoder_info()['workspace_bytes']
    eng.joint_decode(torch.zeros(2, 300, 256, device=eng.device), torch.tensor([300, 4], dtype=torch.int32, device=eng.device),
                     torch.full((2, 300, V), 1.0 / V, device=eng.device), 8, 16, 0.3, 0.0, 2)
    assert eng.decoder_info()['workspace_bytes'] >= max(before, 2 * 2 * 8 * 2 * 300 * 4)
    with pytest.raises(MasrError, match='ctc_candidates = 65'):
        eng.joint_decode(enc, lens, post, 4, 65)
    with pytest.raises(MasrError, match='ctc_candidates = 3 is outside beam_size'):
        eng.joint_decode(enc, lens, post, 4, 3)
    with pytest.raises(MasrError, match='ctc_weight'):
        eng.joint_decode(enc, lens, post, 4, 8, 1.0)
    with pytest.raises(MasrError, match='post_dev'):
        eng.joint_decode(enc, lens, None, 4, 8, 0.3)
    with pytest.raises(MasrError, match='outside 1 .. 64'):
        eng.joint_decode(enc, lens, post, 65, 65)


# ---- through the facade -------------------------------------------------------------------------------------------------------------
def _cfg(tmp_path, decoder, **more):
    from masr_amd.utils import synthetic
    vpath = os.path.join(tmp_path, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(V):
            f.write(f'{t}\t1\n')
    cfg = {'encoder_conf': dict(ENC_CONF), 'decoder_conf': dict(DEC_CONF),
           'model_conf': {'ctc_weight': 0.3, 'reverse_weight': 0.3},
           'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'attention_decoder_conf': {'beam_size': jr.E2E['beam_size']},
           'joint_decoder_conf': {'beam_size': jr.E2E['beam_size'], 'ctc_candidates': jr.E2E['ctc_candidates'], 'length_bonus': 0.5},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'conformer', 'streaming': True, 'decoder': decoder,
           'metrics_type': 'cer'}
    cfg.update(more)
    return cfg


def test_predictor_end_to_end(tmp_path, sd, eng):
    """predict_batch texts are the float64 search's on the safe utterances (over the encoder output and posteriors the facade
    searched); timestamps=True returns the winner's tokens aligned; the same predictor configured with decoder: attention gives
    what masr_attention_decode gives"""
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    pred = MASRPredictor(configs=_cfg(str(tmp_path), 'joint'), use_gpu=True, state_dict=sd)
    dec = pred.joint_decoder
    assert (dec.ctc_weight, dec.length_bonus, dec.ctc_candidates) == (0.3, 0.5, jr.E2E['ctc_candidates'])
    seen = []
    inner = dec.search_launch

    def spy(eng_, enc, enc_lens, probs):
        seen.append((enc.cpu().numpy(), enc_lens.cpu().numpy(), probs.cpu().numpy()))
        return inner(eng_, enc, enc_lens, probs)
    dec.search_launch = spy
    E = jr.E2E
    pcm = synthetic.synthetic_pcm(8, max(E['lens']), seed=E['pcm_seed'])
    audio = [pcm[i, :n].copy() for i, n in enumerate(E['lens'])]
    res = pred.predict_batch(audio, timestamps=True)
    assert len(seen) == 1 and len(res) == 8
    memory, mem_lens, probs = seen[0]
    kept = 0
    for b in range(8):
        mem, post = memory[b, :mem_lens[b]], probs[b, :mem_lens[b]]
        r64, r32 = _refs(sd, mem, post, E['beam_size'], E['ctc_candidates'], 0.3, 0.5)
        e_ref, unsafe = ar.safety(r64, r32)
        if unsafe is not None:
            continue
        kept += 1
        toks, score = r64['hyps'][0]
        assert res[b]['text'] == pred._text(toks), b
        if np.isfinite(score):
            assert abs(res[b]['score'] - score) <= budget.C * max(e_ref, budget.ULP32 * abs(score)), b
        else:
            assert res[b]['score'] == score, b
        assert dec.last_parts is not None and len(dec.last_parts[b]) == E['beam_size']
        # the alignment is the winner's: one entry per token, in order (None: the CTC trellis holds no path for it)
        if res[b]['tokens'] is not None:
            assert [t['token'] for t in res[b]['tokens']] == [pred._text_featurizer.vocab_list[t] for t in toks]
            assert all(t['start'] <= t['end'] for t in res[b]['tokens'])
    assert kept >= 6, kept
    one = pred.predict(audio_data=audio[0])
    assert set(one) == {'text', 'score'}
    with pytest.raises(Exception, match="decoder='joint' does not run on streaming sessions"):
        pred.predict_stream(pcm[0, :16000].tobytes())
    with pytest.raises(ValueError, match="decoder='joint'"):
        pred.predict(audio_data=audio[0], nbest=2)
    # decoder: attention on the same checkpoint: the facade's results are masr_attention_decode's over its own encoder output
    att = MASRPredictor(configs=_cfg(str(tmp_path), 'attention'), use_gpu=True, state_dict=sd)
    seen_a = []
    inner_a = att.attention_decoder.search_launch

    def spy_a(eng_, enc, enc_lens):
        seen_a.append((enc.clone(), enc_lens.clone()))
        return inner_a(eng_, enc, enc_lens)
    att.attention_decoder.search_launch = spy_a
    res_a = att.predict_batch(audio)
    enc, enc_lens = seen_a[0]
    engine = att.predictor.engine
    t0, l0, s0, _ = engine.attention_decode(enc, enc_lens, E['beam_size'])
    t0, l0, s0 = t0.cpu().numpy(), l0.cpu().numpy(), s0.cpu().numpy()
    for b in range(8):
        assert res_a[b]['text'] == att._text(t0[b, 0, :l0[b, 0]].tolist()) and np.float32(res_a[b]['score']) == s0[b, 0]
