"""GPU: ``decoder: joint`` with a language model (masr_joint_decode_lm / masr_op_lm_scores, csrc/decoder_joint.hip): the LM score
kernel alone, bit for bit against ``LanguageModel.cond_log_prob`` at the window, order, shape and vocabulary edges; the fused search
against the float64 restatement (tests/joint_lm_ref.py) wherever its decisions are safe (the rule, bars and cap of
tests/test_gpu_joint_decode.py), bit equality with masr_joint_decode at lm_weight 0, a hand-made model that changes the winner,
bit-for-bit invariance of an utterance's result, and the mode end to end through MASRPredictor.

V = 50, d = 256 / 4 heads, encoder of 2 blocks, left decoder of 1 block, no right decoder, unless a case says otherwise."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_decode_ref as ar            # noqa: E402
import budget            # noqa: E402
import ctc_prefix_ref as cp            # noqa: E402
import joint_lm_ref as jl            # noqa: E402
import rescoring_ref as rr            # noqa: E402

pytestmark = pytest.mark.gpu

V = jl.V
DEC_CONF = dict(attention_heads=4, **jl.DEC)
ENC_CONF = dict(num_blocks=2, linear_units=256)
OOV = np.float32(-1000.0)


def _engine(sd_, vocab=V):
    from masr_amd.engine import HipEngine
    return HipEngine(sd_, encoder_conf=ENC_CONF, vocab_size=vocab, attention_decoder=True, decoder_conf=DEC_CONF)


@pytest.fixture(scope='module')
def sd():
    return jl.state_dict()


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


@pytest.fixture(scope='module')
def models(tmp_path_factory):
    """order -> (LanguageModel over the V = 50 vocabulary, its n-grams per order as id tuples)"""
    root = tmp_path_factory.mktemp('arpa')
    out = {}
    for order in (1, 3, 5):
        lm, toks = jl.synthetic_model(os.path.join(str(root), f'o{order}.arpa'), V, order, seed=order, n_higher=300)
        assert lm.max_order == order and lm.is_character_based
        out[order] = (lm, _ngrams(lm.path, toks, lm))
    return out


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------------
def _ngrams(path, toks, lm):
    """the ARPA file's n-grams as {order: {id tuple: (log10 p, log10 backoff)}} (<s> / </s> as lm.bos / lm.eos; <unk> left out)"""
    ids = {t: i for i, t in reversed(list(enumerate(toks)))}
    ids.update({'<s>': lm.bos, '</s>': lm.eos})
    grams, n = {}, 0
    for line in open(path, encoding='utf-8'):
        line = line.rstrip('\n')
        if line.startswith('\\') and line.endswith('-grams:'):
            n = int(line[1:line.index('-')])
            grams[n] = {}
        elif line.startswith('\\'):
            n = 0
        elif n and line:
            f = line.split('\t')
            words = f[1].split(' ')
            if all(w in ids and w != '<unk>' for w in words):
                grams[n][tuple(ids[w] for w in words)] = (float(f[0]), float(f[2]) if len(f) > 2 else 0.0)
    return grams


def _want(lm, vocab, prefix, cands):
    return np.array([lm.cond_log_prob(list(prefix) + [lm.eos if c == vocab - 1 else c]) for c in cands], np.float32)


def _check_op(eng_, lm, rows, vocab=V):
    """``rows`` [(prefix, candidates)] through the op: bit-equal to cond_log_prob, entry by entry"""
    R, L, M = len(rows), max(1, max(len(r[0]) for r in rows)), len(rows[0][1])
    prefixes, lens = np.zeros((R, L), np.int32), np.array([len(r[0]) for r in rows], np.int32)
    for i, r in enumerate(rows):
        prefixes[i, :len(r[0])] = r[0]
    cands = np.array([r[1] for r in rows], np.int32)
    got = eng_.lm_scores(lm, prefixes, lens, cands)
    want = np.stack([_want(lm, vocab, p, c) for p, c in rows])
    assert got.shape == want.shape == (R, M)
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert len(bad) == 0, (bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def _known(rng, n, vocab=V):
    return rng.integers(3, vocab - 1, n).tolist()          # (ids 0 .. 2 and vocab - 1 are no single characters: unknown to the model)


def _rows_on_ngrams(rng, grams, order, length, n_rows, m):
    """prefixes of ``length`` tokens that END in the context of one of the model's longest n-grams (as far as they have room),
    candidates: that n-gram's last word, then random known ones"""
    top = [g for g in grams[order] if all(w < V - 1 for w in g)] if order > 1 else []
    rows = []
    for i in range(n_rows):
        ctx, last = [], None
        if top:
            g = top[int(rng.integers(0, len(top)))]
            ctx, last = list(g[:-1]), g[-1]
        prefix = (_known(rng, length) + ctx)[-length:] if length else []
        cands = ([last] if last is not None else []) + _known(rng, m)
        rows.append((prefix, cands[:m]))
    return rows


@pytest.mark.parametrize('order,length', sorted({(o, n) for o in (1, 3, 5) for n in (0, 1, max(o - 2, 0), o - 1, o, o + 3)}))
def test_op_prefix_lengths_around_the_window(eng, models, order, length):
    lm, grams = models[order]
    rng = np.random.default_rng(100 * order + length)
    got = _check_op(eng, lm, _rows_on_ngrams(rng, grams, order, length, 6, 8))
    assert (got > OOV).all()
    if order > 1 and length >= order - 1:          # the whole context of a longest n-gram is in the window: its own probability
        g = next(g for g in grams[order] if all(w < V - 1 for w in g))
        one = _check_op(eng, lm, [(list(g[:-1]), [g[-1]])])
        assert np.isclose(one[0, 0], grams[order][g][0] * np.log(10.0), rtol=1e-6)


@pytest.mark.parametrize('M', [1, 64])
def test_op_one_and_sixty_four_candidates(eng, models, M):
    lm, grams = models[3]
    rng = np.random.default_rng(M)
    rows = _rows_on_ngrams(rng, grams, 3, 4, 3, 1) if M == 1 else [(p, (list(range(V)) + _known(rng, 14))) for p, _ in
                                                                    _rows_on_ngrams(rng, grams, 3, 4, 3, 1)]
    _check_op(eng, lm, rows)


@pytest.mark.parametrize('R', [1, 130])
def test_op_one_row_and_more_than_two_waves_of_rows(eng, models, R):
    lm, grams = models[5]
    rng = np.random.default_rng(R)
    rows = []
    for i in range(R):
        rows += _rows_on_ngrams(rng, grams, 5, i % 7, 1, 5)
    _check_op(eng, lm, rows)


def test_op_eos_blank_and_unknown_candidates(eng, models):
    lm, grams = models[3]
    g = next(g for g in grams[3] if g[-1] == lm.eos and max(g[:2]) < V - 1)          # a trigram that ends the sentence
    cands = [V - 1, 0, 1, 2, g[1], 7]
    got = _check_op(eng, lm, [(list(g[:-1]), cands), ([], cands), ([g[1]], cands)])
    assert np.isclose(got[0, 0], grams[3][g][0] * np.log(10.0), rtol=1e-6)          # eos is read as </s>
    assert (got[:, 1:4] == OOV).all() and (got[:, 0] > OOV).all() and (got[:, 4:] > OOV).all()


def test_op_unknown_token_inside_and_just_outside_the_window(eng, models):
    lm, _ = models[3]
    cands = [5, 9, V - 1, 0]
    got = _check_op(eng, lm, [([7, 1, 9], cands), ([7, 9, 2], cands), ([1, 7, 9], cands), ([0, 7, 9], cands), ([V - 1, 7, 9], cands)])
    assert (got[:2] == OOV).all()                                   # <unk> / <space> among the last two tokens
    assert (got[2:, :3] > OOV).all() and (got[2:, 3] == OOV).all()          # one token further back: out of the window


def test_op_two_backoffs_are_summed(eng, models):
    """context x y that is a bigram of the model, candidate c with neither x y c nor y c in it: bo(x y) + bo(y) + P(c)"""
    lm, grams = models[3]
    ln10 = np.float32(np.log(10.0))
    found = None
    for (x, y), (_, bo_xy) in grams[2].items():
        if x >= V - 1 or y >= V - 1:
            continue
        for c in range(3, V - 1):
            if (x, y, c) not in grams[3] and (y, c) not in grams[2] and (c,) in grams[1]:
                found = (x, y, c)
                break
        if found:
            break
    assert found is not None
    x, y, c = found
    got = _check_op(eng, lm, [([x, y], [c])])
    want = grams[2][(x, y)][1] + grams[1][(y,)][1] + grams[1][(c,)][0]
    assert np.isclose(got[0, 0], want * ln10, rtol=1e-5)


def test_op_vocabulary_4233(tmp_path):
    vocab = 4233
    lm, toks = jl.synthetic_model(os.path.join(str(tmp_path), 'big.arpa'), vocab, 3, seed=3, n_higher=3000)
    grams = _ngrams(lm.path, toks, lm)
    e = _engine(jl.state_dict(vocab), vocab)
    try:
        rng = np.random.default_rng(4)
        top = [g for g in grams[3] if all(w < vocab - 1 for w in g)]
        rows = []
        for i in range(12):
            g = top[int(rng.integers(0, len(top)))]
            rows.append(([4231, 300] * (i % 2) + list(g[:-1]), [g[-1], vocab - 1, 0, 4231, 2048, 300, 77, 4000]))
        assert max(max(p) for p, _ in rows) > 255
        got = _check_op(e, lm, rows, vocab)
        assert (got[:, 0] > OOV).all() and (got[:, 2] == OOV).all()
    finally:
        e.close()


# ---- the search -------------------------------------------------------------------------------------------------------------------
def _mem(T, seed=0, d=256):
    return np.random.default_rng(seed).standard_normal((T, d)).astype(np.float32)


def _post(rng, T, vocab, gain=3.0):
    z = rng.standard_normal((T, vocab)) * gain
    z[..., 0] += gain
    p = np.exp(z - z.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)).astype(np.float32)


def _pad(items, tp, width):
    out = np.zeros((len(items), tp, width), np.float32)
    for b, m in enumerate(items):
        out[b, :len(m)] = m
    return out


def _lm_sum(lm, toks, finished, vocab=V):
    """Lm of a hypothesis as the library defines it: the float32 running sum of cond_log_prob over its tokens (and </s> when it
    finished), added in that order"""
    acc = np.float32(0.0)
    seq = list(toks) + ([vocab - 1] if finished else [])
    for i, t in enumerate(seq):
        acc = np.float32(acc + np.float32(lm.cond_log_prob(seq[:i] + [lm.eos if t == vocab - 1 else t])))
    return acc


def _decode(eng_, memories, posts, n, m, lam, mu, gam, lm, max_len=0, tp=None, lcap=None):
    """joint_decode_lm over a list of utterances -> (per utterance [(tokens, J, A, psi, Lm)] x N, steps).  Every hypothesis with a
    finite key is checked on the way: Lm is the float32 sum of the model's scores of its tokens, J the float32 formula of the parts"""
    B, tp = len(memories), tp or max(len(x) for x in memories)
    enc = torch.from_numpy(_pad(memories, tp, memories[0].shape[1])).to(eng_.device)
    post = None if posts is None else torch.from_numpy(_pad(posts, tp, posts[0].shape[1])).to(eng_.device)
    lens = torch.tensor([len(x) for x in memories], dtype=torch.int32).to(eng_.device)
    tokens, hl, key, att, psi, lms, steps = eng_.joint_decode_lm(enc, lens, post, lm, mu, n, m, lam, gam, max_len, lcap)
    tokens, hl, key, att, psi, lms = (x.cpu().numpy() for x in (tokens, hl, key, att, psi, lms))
    vocab = eng_.vocab_size
    assert ((tokens == vocab - 1) | (np.arange(tokens.shape[2])[None, None] < hl[..., None])).all()
    f = np.float32
    for b in range(B):
        limit = ar.limit_of(len(memories[b]), max_len)
        limit = min(limit, tokens.shape[2])
        for k in range(n):
            if not np.isfinite(key[b, k]):
                continue
            toks = tokens[b, k, :hl[b, k]].tolist()
            if mu > 0:
                assert f(lms[b, k]).tobytes() == _lm_sum(lm, toks, hl[b, k] < limit, vocab).tobytes(), (b, k, toks, lms[b, k])
            else:
                assert lms[b, k] == 0.0
            mix = (f(1) - f(lam)) * att[b, k]
            if lam != 0:
                mix = f(mix + f(lam) * psi[b, k])
            if mu != 0:
                mix = f(mix + f(mu) * lms[b, k])
            want = f(mix + f(gam) * f(len(toks)))
            assert want.tobytes() == f(key[b, k]).tobytes(), (b, k, toks, key[b, k], att[b, k], psi[b, k], lms[b, k])
    return [[(tokens[b, k, :hl[b, k]].tolist(), key[b, k], att[b, k], psi[b, k], lms[b, k]) for k in range(n)] for b in range(B)], steps


def _same(a, b):
    bits = lambda x: np.float32(x).tobytes()
    return len(a) == len(b) and all(len(x) == len(y) and all(p[0] == q[0] and all(bits(u) == bits(v) for u, v in zip(p[1:], q[1:]))
                                                             for p, q in zip(x, y)) for x, y in zip(a, b))


def _fns(sd_, mem):
    memo = ({}, {})
    return [lambda toks, s=s, c=c: c.setdefault(tuple(toks), ar.step_logp(s, mem, toks)) for s, c in zip((rr.to64(sd_), sd_), memo)]


def _refs(mem, post, n, m, lam, mu, gam, fns, lm_fn, max_len=0):
    """the float64 and the float32 fused search over the posteriors the device reads (float32 probabilities)"""
    vocab = post.shape[1]
    r64 = jl.search(mem, cp.log_post(post, np.float64), n, m, lam, mu, gam, fns[0], vocab, lm_fn, max_len)
    r32 = jl.search(mem, cp.log_post(post, np.float32), n, m, lam, mu, gam, fns[1], vocab, lm_fn, max_len, dtype=np.float32)
    return r64, r32


def _assert_search(name, got, r64, r32):
    """the device's N hypotheses against the float64 search: equal in order with J within the budget when every step is safe (the
    rule and the bars of tests/test_gpu_joint_decode.py)"""
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
    if not fin.any():
        return True
    bar = budget.C * max(e_ref, budget.ULP32 * np.abs(s64[fin]).max())
    print(f'{name}: max |J - J64| {np.abs(s[fin] - s64[fin]).max():.3e}, bar {bar:.3e}', flush=True)
    assert np.abs(s[fin] - s64[fin]).max() <= bar, name
    return True


@pytest.fixture(scope='module')
def e2e(sd, eng, tmp_path_factory):
    """the 8 utterances of joint_lm_ref.E2E_LM through the engine's own front end, encoder and CTC head, once, and its model; the
    step log-probabilities of the restatement are remembered per utterance and prefix, the grid's searches share them"""
    from masr_amd.utils import synthetic
    E = jl.E2E_LM
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
    path = os.path.join(str(tmp_path_factory.mktemp('e2e')), 'e2e.arpa')
    lm, _ = jl.synthetic_model(path, V, E['arpa_order'], E['arpa_seed'], E['arpa_n_higher'])
    return dict(pcm=pcm, mems=mems, posts=posts, fns=[_fns(sd, mem) for mem in mems], n=E['beam_size'], m=E['ctc_candidates'], lm=lm,
                lm_fn=jl.lm_fn_of(lm, V), path=path)


def test_lm_weight_zero_with_a_model_is_masr_joint_decode_bit_for_bit(eng, e2e):
    n, m = e2e['n'], e2e['m']
    tp = max(len(x) for x in e2e['mems'])
    enc = torch.from_numpy(_pad(e2e['mems'], tp, 256)).to(eng.device)
    post = torch.from_numpy(_pad(e2e['posts'], tp, V)).to(eng.device)
    lens = torch.tensor([len(x) for x in e2e['mems']], dtype=torch.int32).to(eng.device)
    bits = lambda x: x.cpu().numpy().view(np.int32)
    for lam, gam, p in ((0.3, 0.5, post), (0.0, 0.0, None)):
        t0, l0, s0, a0, p0, steps0 = eng.joint_decode(enc, lens, p, n, m, lam, gam)
        for model in (e2e['lm'], None):
            t1, l1, s1, a1, p1, lm1, steps1 = eng.joint_decode_lm(enc, lens, p, model, 0.0, n, m, lam, gam)
            assert steps0 == steps1 and torch.equal(t0, t1) and torch.equal(l0, l1)
            assert np.array_equal(bits(s0), bits(s1)) and np.array_equal(bits(a0), bits(a1)) and np.array_equal(bits(p0), bits(p1))
            assert not lm1.any()


def test_attention_and_lm_alone_needs_no_posteriors(sd, eng, e2e):
    n, m, lm = e2e['n'], e2e['m'], e2e['lm']
    got, _ = _decode(eng, e2e['mems'][:2], None, n, m, 0.0, 0.3, 0.0, lm)
    with_post, _ = _decode(eng, e2e['mems'][:2], e2e['posts'][:2], n, m, 0.0, 0.3, 0.0, lm)
    assert _same(got, with_post) and all(h[3] == 0.0 for u in got for h in u)
    for b in range(2):
        r64, r32 = _refs(e2e['mems'][b], e2e['posts'][b], n, m, 0.0, 0.3, 0.0, e2e['fns'][b], e2e['lm_fn'])
        _assert_search(f'attention + LM utterance {b}', got[b], r64, r32)


@pytest.mark.parametrize('lam,mu,gam', jl.E2E_LM['grid'])
def test_search_parity_with_the_float64_fused_search(eng, e2e, lam, mu, gam):
    n, m = e2e['n'], e2e['m']
    got, _ = _decode(eng, e2e['mems'], e2e['posts'], n, m, lam, mu, gam, e2e['lm'])          # (J = the formula of its parts: _decode)
    safe = 0
    for b in range(8):
        r64, r32 = _refs(e2e['mems'][b], e2e['posts'][b], n, m, lam, mu, gam, e2e['fns'][b], e2e['lm_fn'])
        if _assert_search(f'E2E_LM lam {lam} mu {mu} gamma {gam} utterance {b}', got[b], r64, r32):
            safe += 1
    assert safe >= 6, safe


def hand_flip_case(sd_):
    """(mem, post, X, Y, ARPA text): an utterance whose LM-free float64 winner starts X W; Y is the best other known character
    among the attention candidates behind X; the bigram model prefers X Y strongly and knows every other character equally"""
    from masr_amd.utils import synthetic
    mem = _mem(14, 3)
    post = _post(np.random.default_rng(8), 14, V, gain=0.5)
    fns = _fns(sd_, mem)
    r0 = jl.search(mem, cp.log_post(post, np.float64), 4, 8, 0.3, 0.0, 0.0, fns[0], V)
    win = r0['hyps'][0][0]
    assert len(win) >= 2 and 3 <= win[0] < V - 1
    X = win[0]
    Y = next(t for _, t in ar.top_n(np.asarray(fns[0]([X])), 8) if 3 <= t < V - 1 and t != win[1])
    toks = synthetic.synthetic_vocab(V)
    chars = [toks[i] for i in range(3, V - 1)]
    lines = ['\\data\\', f'ngram 1={len(chars) + 3}', 'ngram 2=1', '', '\\1-grams:', '-99\t<s>\t-0.5', '-2.0\t</s>', '-3.0\t<unk>']
    lines += [f'-2.0\t{c}\t-0.5' for c in chars] + ['', '\\2-grams:', f'-0.01\t{toks[X]} {toks[Y]}', '', '\\end\\', '']
    return mem, post, X, Y, win, '\n'.join(lines), fns


def test_a_hand_made_model_changes_the_winner_on_the_device(sd, eng, tmp_path):
    from masr_amd.decoders.lm_scorer import LanguageModel
    from masr_amd.utils import synthetic
    mem, post, X, Y, win, text, fns = hand_flip_case(sd)
    path = os.path.join(str(tmp_path), 'hand.arpa')
    with open(path, 'w', encoding='utf-8') as f:
        f.write(text)
    lm = LanguageModel(path, synthetic.synthetic_vocab(V))
    lm_fn = jl.lm_fn_of(lm, V)
    mu = 1.0
    r64, r32 = _refs(mem, post, 4, 8, 0.3, mu, 0.0, fns, lm_fn)
    assert r64['hyps'][0][0][:2] == [X, Y] and win[:2] != [X, Y]
    plain, _ = _decode(eng, [mem], [post], 4, 8, 0.3, 0.0, 0.0, lm)
    fused, _ = _decode(eng, [mem], [post], 4, 8, 0.3, mu, 0.0, lm)
    assert _assert_search('hand-made model', fused[0], r64, r32)
    assert plain[0][0][0] == win and fused[0][0][0][:2] == [X, Y]


def test_an_utterance_alone_in_a_batch_padded_on_the_other_lane_and_polled(eng, e2e, poll):
    """bit for bit: tokens, J, A, psi, Lm of an utterance's N hypotheses do not depend on B, its neighbours, the padding of Tp, the
    lane, or on how often the host polls for the end"""
    n, m = e2e['n'], e2e['m']
    run = lambda mems, posts, **kw: _decode(eng, mems, posts, n, m, 0.3, 0.3, 0.5, e2e['lm'], **kw)
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
    for every in (0, 1):
        poll(every)
        polled, steps = run(e2e['mems'], e2e['posts'])
        assert _same(polled, full), every
        assert every != 0 or steps == 32


def test_a_finished_row_keeps_its_lm(sd, e2e, poll):
    """a raised eos bias finishes every hypothesis before the limit; polled at every step the search stops there, never polled it
    runs to the limit: the finished rows offer themselves step after step and come back with the same Lm (and everything else)
    to the bit"""
    sd2 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
    sd2['decoder.left_decoder.output_layer.bias'][V - 1] += 24.0
    e = _engine(sd2)
    try:
        mem, lm = _mem(20, 0), e2e['lm']
        post = _post(np.random.default_rng(6), 20, V, gain=1.0)
        r64, r32 = _refs(mem, post, 4, 8, 0.3, 0.3, 0.0, _fns(sd2, mem), e2e['lm_fn'])
        assert r64['steps'] < r64['limit']
        poll(1)
        got, steps = _decode(e, [mem], [post], 4, 8, 0.3, 0.3, 0.0, lm)
        assert _assert_search('eos bias', got[0], r64, r32)
        assert steps == r64['steps'] and all(len(h[0]) < steps for h in got[0]) and all(h[4] != 0.0 for h in got[0])
        poll(0)
        again, steps = _decode(e, [mem], [post], 4, 8, 0.3, 0.3, 0.0, lm)
        assert steps == r64['limit'] and _same(again, got)
    finally:
        e.close()


def test_refusals_on_a_live_engine_and_the_workspace(eng, e2e, tmp_path):
    from masr_amd._lib import MasrError
    from masr_amd.decoders.lm_scorer import LanguageModel, write_synthetic_word_arpa
    lm = e2e['lm']
    enc = torch.zeros(1, 4, 256, device=eng.device)
    post = torch.full((1, 4, V), 1.0 / V, device=eng.device)
    lens = torch.tensor([4], dtype=torch.int32, device=eng.device)
    small, _ = jl.synthetic_model(os.path.join(str(tmp_path), 's.arpa'), 20, 2, n_higher=30)
    words = ['<blank>', '<unk>', '<space>'] + [chr(ord('a') + i) for i in range(V - 4)] + ['<eos>']
    word = LanguageModel(write_synthetic_word_arpa(os.path.join(str(tmp_path), 'w.arpa'), ['ab', 'ca', 'b'], order=2, seed=1, n_higher=6),
                         words)
    with pytest.raises(MasrError, match='loaded for a vocabulary of 20 tokens, the engine has 50'):
        eng.joint_decode_lm(enc, lens, post, small, 0.3, 4, 8)
    with pytest.raises(MasrError, match='word-based language models'):
        eng.joint_decode_lm(enc, lens, post, word, 0.3, 4, 8)
    with pytest.raises(MasrError, match='lm_weight > 0 needs a language model'):
        eng.joint_decode_lm(enc, lens, post, None, 0.3, 4, 8)
    for mu in (-0.1, float('nan')):
        with pytest.raises(MasrError, match='lm_weight'):
            eng.joint_decode_lm(enc, lens, post, lm, mu, 4, 8)
    with pytest.raises(MasrError, match='ctc_candidates = 3 is outside beam_size'):
        eng.joint_decode_lm(enc, lens, post, lm, 0.3, 4, 3)
    with pytest.raises(MasrError, match='post_dev'):
        eng.joint_decode_lm(enc, lens, None, lm, 0.3, 4, 8, 0.3)
    z = np.zeros((1, 2), np.int32)
    with pytest.raises(MasrError, match='loaded for a vocabulary of 20 tokens'):
        eng.lm_scores(small, z, [0], [[1]])
    with pytest.raises(MasrError, match='word-based language models'):
        eng.lm_scores(word, z, [0], [[1]])
    with pytest.raises(MasrError, match='outside 0 .. L'):
        eng.lm_scores(lm, z, [3], [[1]])
    for bad in (-1, V):
        with pytest.raises(MasrError, match='of prefix 0 is outside the vocabulary'):
            eng.lm_scores(lm, np.array([[3, bad]], np.int32), [2], [[1]])
        with pytest.raises(MasrError, match='of row 0 is outside the vocabulary'):
            eng.lm_scores(lm, z, [0], [[bad]])
    with pytest.raises(MasrError, match='M = 65'):
        eng.lm_scores(lm, z, [0], [[1] * 65])
    # the candidates' LM scores are part of the lane's decoder workspace
    eng.joint_decode_lm(torch.zeros(2, 40, 256, device=eng.device), torch.tensor([40, 4], dtype=torch.int32, device=eng.device),
                        None, lm, 0.3, 32, 50, 0.0, 0.0, 2)
    assert eng.decoder_info()['workspace_bytes'] >= (8 * 64 + 2 * 64 * 50) * 4


# ---- through the facade -------------------------------------------------------------------------------------------------------------
def _cfg(tmp_path, **jconf):
    from masr_amd.utils import synthetic
    vpath = os.path.join(tmp_path, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(V):
            f.write(f'{t}\t1\n')
    E = jl.E2E_LM
    return {'encoder_conf': dict(ENC_CONF), 'decoder_conf': dict(DEC_CONF), 'model_conf': {'ctc_weight': 0.3, 'reverse_weight': 0.0},
            'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                                'use_dB_normalization': True, 'target_dB': -20},
            'joint_decoder_conf': dict({'beam_size': E['beam_size'], 'ctc_candidates': E['ctc_candidates'], 'length_bonus': 0.5}, **jconf),
            'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'conformer', 'streaming': True, 'decoder': 'joint',
            'metrics_type': 'cer'}


def test_predictor_end_to_end(tmp_path, sd, e2e):
    """predict_batch with language_model_path + lm_weight: the texts are the float64 fused search's on the safe utterances (over the
    encoder output and posteriors the facade searched), ``last_lm`` holds the winner's Lm; timestamps=True aligns the winner's
    tokens; a path with lm_weight 0 loads no model; streams and nbest stay refused with the joint decoder's messages"""
    from masr_amd.decoders import joint_decoder as jd
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    E = jl.E2E_LM
    mu = 0.6
    pred = MASRPredictor(configs=_cfg(str(tmp_path), language_model_path=e2e['path'], lm_weight=mu), use_gpu=True, state_dict=sd)
    dec = pred.joint_decoder
    assert (dec.ctc_weight, dec.lm_weight, dec.length_bonus) == (0.3, mu, 0.5) and dec.language_model.max_order == E['arpa_order']
    seen = []
    inner = dec.search_launch

    def spy(eng_, enc, enc_lens, probs):
        seen.append((enc.cpu().numpy(), enc_lens.cpu().numpy(), probs.cpu().numpy()))
        return inner(eng_, enc, enc_lens, probs)
    dec.search_launch = spy
    pcm = synthetic.synthetic_pcm(8, max(E['lens']), seed=E['pcm_seed'])
    audio = [pcm[i, :n].copy() for i, n in enumerate(E['lens'])]
    res = pred.predict_batch(audio, timestamps=True)
    assert len(seen) == 1 and len(res) == 8
    memory, mem_lens, probs = seen[0]
    kept = 0
    for b in range(8):
        mem, post = memory[b, :mem_lens[b]], probs[b, :mem_lens[b]]
        r64, r32 = _refs(mem, post, E['beam_size'], E['ctc_candidates'], 0.3, mu, 0.5, _fns(sd, mem), e2e['lm_fn'])
        e_ref, unsafe = ar.safety(r64, r32)
        if unsafe is not None:
            continue
        kept += 1
        toks, score = r64['hyps'][0]
        assert res[b]['text'] == pred._text(toks), b
        assert len(dec.last_parts[b]) == E['beam_size'] and len(dec.last_lm[b]) == E['beam_size']
        if np.isfinite(score):
            assert abs(res[b]['score'] - score) <= budget.C * max(e_ref, budget.ULP32 * abs(score)), b
        else:            # (every hypothesis outgrew its frames: all keys are -inf, the order is the tie rule's)
            assert res[b]['score'] == score, b
        # Lm is a function of the tokens alone: the float32 sum of the model's scores, </s> included where the winner finished
        assert np.float32(dec.last_lm[b][0]).tobytes() == _lm_sum(dec.language_model, toks, len(toks) < len(mem)).tobytes(), b
        if res[b]['tokens'] is not None:
            assert [t['token'] for t in res[b]['tokens']] == [pred._text_featurizer.vocab_list[t] for t in toks]
    assert kept >= 6, kept
    assert set(pred.predict(audio_data=audio[0])) == {'text', 'score'}
    with pytest.raises(Exception) as err:
        pred.predict_stream(pcm[0, :16000].tobytes())
    assert str(err.value) == jd.STREAM_REFUSAL
    with pytest.raises(ValueError) as err:
        pred.predict(audio_data=audio[0], nbest=2)
    assert str(err.value) == jd.NBEST_REFUSAL.format(nbest=2)
    off = MASRPredictor(configs=_cfg(str(tmp_path), language_model_path=e2e['path'], lm_weight=0), use_gpu=True, state_dict=sd)
    assert off.joint_decoder.language_model is None and off.joint_decoder.lm_weight == 0.0
    off.predict_batch(audio[:2])
    assert off.joint_decoder.last_lm == [[0.0] * E['beam_size']] * 2
