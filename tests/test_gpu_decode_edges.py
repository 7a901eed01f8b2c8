"""GPU: the decode tail at its wave, slice and tie edges -- argmax_rows_kernel, softmax_argmax_kernel, ctc_collapse_kernel in its
three launch forms, topk_prune_kernel (csrc/elementwise.hip) and the fused CTC head (csrc/rowgemm.hip, RG_EPI_CTC) -- against the
exact restatements of tests/decode_ref.py.  Indices, counts, tokens, the -1 padding and scores are compared bit for bit; only
probabilities (the rule of tests/budget.py) and logarithms (2 float32 ulp) carry an allowance.  Nothing is asserted where the
contract is silent: NaN inputs, slots at or behind a returned count, two different logits that round to one probability."""
import ctypes as C

import numpy as np
import pytest
import torch

from masr_amd import _lib
from masr_amd._lib import debug_keys
from tests import budget, decode_ref as dr

pytestmark = pytest.mark.gpu


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope='module')
def eng():
    from masr_amd.engine import HipEngine
    e = HipEngine(None)
    yield e
    e.close()


# ---- a. masr_argmax_rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [1, 2, 63, 64, 65, 255, 256, 257, 1023, 8192, 8193, 16384])
def test_argmax_rows_first_maximum(eng, V):
    """the designed rows of decode_ref.argmax_cases in launches of M = 300 (the last one filled up from the start) and M = 1:
    index and maximum bit-equal to argmax_first"""
    rows = dr.argmax_cases(V)
    want_i, want_m = dr.argmax_first(rows)
    for r0 in range(0, len(rows), 300):
        sel = np.arange(r0, r0 + 300) % len(rows)
        idx, mp = eng.argmax_rows(dev(rows[sel]))
        assert np.array_equal(idx.cpu().numpy(), want_i[sel]), (V, r0)
        assert np.array_equal(bits(mp.cpu().numpy()), bits(want_m[sel])), (V, r0)
    for r in sorted({0, len(rows) // 2, len(rows) - 3, len(rows) - 2, len(rows) - 1}):      # M = 1: a peak, ties, the all-equal row
        idx, mp = eng.argmax_rows(dev(rows[r:r + 1]))
        assert idx.item() == want_i[r] and bits(mp.cpu().numpy())[0] == bits(want_m[r:r + 1])[0], (V, r)


def test_argmax_rows_refuses_a_row_past_16384(eng):
    x = torch.zeros(1, 16385, device='cuda')
    with pytest.raises(_lib.MasrError, match='V > 16384'):
        eng.argmax_rows(x)


# ---- b. the head with designed logits ---------------------------------------------------------------------------------------------
def held(res, name, y64, y32, y):
    """one output under the rule of tests/budget.py: printed now, asserted at the end of the test with all the others"""
    res.append((name, budget.evaluate(y64, y32, y)))
    print(budget.line(name, res[-1][1]), flush=True)


def m1_rows(kinds):
    """one row of every kind, and the first two placements"""
    return sorted({0, 1} | {kinds.index(k) for k in ('tie', 'equal', 'pm80', 'margin')})


@pytest.mark.parametrize('V', [5, 256, 257, 4233, 8192, 8193, 16384])
def test_ctc_head_designed_logits(V):
    """A one-block Conformer engine whose CTC weight is decode_ref.head_weight(V) and whose bias is 0, on the rows of the 256 x 256
    identity: row k's logits are column k of the weight exactly (every other product is 0 * w).  The premise is checked on the
    device: masr_op_gemm returns the weight's columns bit for bit, and the two columns of a tie pair come back from masr_ctc_probs
    with bit-equal probabilities.

    Column c of the fused head (rowgemm.hip, RG_EPI_CTC): tile c // 256 (wrow_of(t) = 256 t + 32 wave), stripe = wave (c % 256) // 32,
    and with x = c % 32 half-wave fh = (x >> 2) & 1, accumulator register r = (x & 3) + 4 (x >> 3) -- the inverse of the column
    order (r & 3) + 8 (r >> 2) + 4 fh.  A bit-equal pair therefore meets the register scan (one half-wave), the lane ^ 32 exchange
    (two half-waves of a tile), the running state (two tiles of a stripe) or the merge of the eight stripes, and the first index
    has to win each; decode_ref.head_placements lists the pairs, the other tie rows hold seeded random pairs.

    Routes: masr_ctc_probs; masr_ctc_greedy_frames through the tiled GEMM + statistics launch (ctc_fused_blocks out of reach);
    the fused head (ctc_fused_blocks = 1) under rowgemm_packed 0 and 1.  M = 256, 33 (a ragged second row block: the head
    placements, one row of every kind, then every eighth row) and 1; the fused routes also at M = 3584 = 14 x the 256 rows, the
    first M at which rowgemm() hands the packed weights to the kernel (below it both switch values run the slab kernel).

    No row is left out: the argmax is the first index of the exact maximum on every route; probabilities and max-probs hold the
    budget rule against the float64 softmax of the exact logits (reference: torch CPU float32 softmax); rows sum to 1 within 1e-4;
    on the masr_ctc_probs route the max-prob is probs[row, argmax] bit for bit; the all-equal row has V bit-equal probabilities."""
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    W, kinds = dr.head_weight(V)
    sd = synthetic.conformer_state_dict(0, V, num_blocks=1)
    assert tuple(sd['ctc.ctc_lo.weight'].shape) == W.shape
    sd['ctc.ctc_lo.weight'] = torch.from_numpy(W.copy())
    sd['ctc.ctc_lo.bias'] = torch.zeros(V)
    logits = np.ascontiguousarray(W.T)                                   # [256 rows, V]
    want, _ = dr.argmax_first(logits)
    p64 = torch.softmax(torch.from_numpy(logits).double(), -1).numpy()
    p32 = torch.softmax(torch.from_numpy(logits), -1).numpy()
    eye = np.eye(256, dtype=np.float32)
    n_place = len(dr.head_placements(V))
    sel33 = (list(range(n_place)) + m1_rows(kinds) + list(range(0, 256, 8)))[:33] if n_place < 29 else list(range(33))
    subsets = [np.arange(256), np.array(sel33)] + [np.array([r]) for r in m1_rows(kinds)]
    e = HipEngine(sd, encoder_conf={'num_blocks': 1}, vocab_size=V)
    res = []
    try:
        got = e.op_gemm(dev(eye), dev(W), dev(np.zeros(V, np.float32))).cpu().numpy()
        assert np.array_equal(bits(got), bits(logits)), 'identity rows do not give the exact weight columns'
        for rows in subsets:
            M = len(rows)
            case = f'designed head V={V} M={M}' + (f' row {rows[0]}' if M == 1 else '')
            enc = dev(eye[rows])
            probs, idx, mp = e.ctc_probs(enc, want_argmax=True)
            probs, idx, mp = probs.cpu().numpy(), idx.cpu().numpy(), mp.cpu().numpy()
            assert np.array_equal(idx, want[rows]), case
            assert np.isfinite(probs).all() and np.abs(probs.astype(np.float64).sum(-1) - 1).max() < 1e-4, case
            assert np.array_equal(bits(mp), bits(probs[np.arange(M), idx])), case
            for i, k in enumerate(rows):
                top = np.nonzero(logits[k] == logits[k].max())[0]
                assert len(set(bits(probs[i, top]).tolist())) == 1, (case, k, 'bit-equal logits, different probabilities')
            held(res, case + ' probs', p64[rows], p32[rows], probs)
            held(res, case + ' max prob', p64[rows].max(-1), p32[rows].max(-1), mp)
            routes = [('tiled', {'ctc_fused_blocks': 1 << 30}), ('fused slabs', {'ctc_fused_blocks': 1, 'rowgemm_packed': 0}),
                      ('fused packed', {'ctc_fused_blocks': 1, 'rowgemm_packed': 1})]
            for name, keys in routes:
                with debug_keys(e, keys):
                    idx2, mp2 = e.ctc_greedy_frames(enc)
                    idx2, mp2 = idx2.cpu().numpy(), mp2.cpu().numpy()
                assert np.array_equal(idx2, want[rows]), (case, name, np.nonzero(idx2 != want[rows])[0][:8])
                held(res, f'{case} {name} max prob', p64[rows].max(-1), p32[rows].max(-1), mp2)
        big = np.tile(np.arange(256), 14)                                # 112 row blocks: the packed weights are used
        for name, keys in routes[1:]:
            with debug_keys(e, keys):
                idx2, mp2 = e.ctc_greedy_frames(dev(eye[big]))
                idx2, mp2 = idx2.cpu().numpy(), mp2.cpu().numpy()
            assert np.array_equal(idx2, want[big]), (V, name, 'M=3584')
            held(res, f'designed head V={V} M=3584 {name} max prob', p64[big].max(-1), p32[big].max(-1), mp2)
    finally:
        e.close()
    over = [budget.line(name, f) for name, f in res if not f['ok']]
    assert not over, 'over budget:\n' + '\n'.join(over)


# ---- c. collapse ----------------------------------------------------------------------------------------------------------------
VC = 256


def garbage(idx, maxp, nfr, fill):
    """copies with the frames behind min(n_frames[b], Tp) replaced: fill 0 = random tokens and probabilities, 1 = one token and 1e30"""
    rng = np.random.default_rng(fill)
    idx, maxp = idx.copy(), maxp.copy()
    for b in range(idx.shape[0]):
        n = min(int(nfr[b]), idx.shape[1])
        idx[b, n:] = rng.integers(0, VC, idx.shape[1] - n) if fill == 0 else 7
        maxp[b, n:] = rng.uniform(0, 1, idx.shape[1] - n) if fill == 0 else 1e30
    return idx, maxp


def collapse_want(idx, maxp, nfr, blank):
    B, Tp = idx.shape
    tok = np.full((B, Tp), -1, np.int32)
    cnt = np.zeros(B, np.int32)
    sc = np.zeros(B, np.float32)
    for b in range(B):
        t, cnt[b], sc[b] = dr.collapse(idx[b], maxp[b], nfr[b], blank)
        tok[b, :cnt[b]] = t
    return tok, cnt, sc


@pytest.mark.parametrize('blank', [0, VC - 1])
@pytest.mark.parametrize('B', [1, 70])
@pytest.mark.parametrize('Tp', [1, 63, 64, 65, 127, 128, 129, 200])
def test_ctc_collapse_rounds_and_forms(eng, Tp, B, blank):
    """decode_ref.collapse_cases (repeat runs, blanks and token changes across the 64-frame rounds of the kernel, all blank, one
    token, all distinct; n_frames 0 .. Tp + 5, and NULL) through the three launch forms: tokens, count, the -1 padding and the
    score bit-equal to decode_ref.collapse; two different fills of the frames behind n_frames give the same output; the packed-row
    form and the history-row form (in_rows a permutation, a list with one row twice, a list that skips rows; ld_in = Tp and
    Tp + 37) equal [tokens | count | score bits] of the first form."""
    idx, maxp, nfr = dr.collapse_cases(Tp, B, VC, blank)
    want = collapse_want(idx, maxp, nfr, blank)
    outs = []
    for fill in (0, 1):
        gi, gp = garbage(idx, maxp, nfr, fill)
        tok, cnt, sc = (t.cpu().numpy() for t in eng.ctc_collapse(dev(gi), dev(gp), dev(nfr), blank=blank))
        assert np.array_equal(tok, want[0]) and np.array_equal(cnt, want[1]), (Tp, B, blank, fill)
        assert np.array_equal(bits(sc), bits(want[2])), (Tp, B, blank, fill)
        outs.append(np.concatenate([tok, cnt[:, None], bits(sc)[:, None]], 1))
        rows = eng.op_ctc_collapse_rows(dev(gi), dev(gp), dev(nfr), blank=blank).cpu().numpy()
        assert np.array_equal(rows, outs[-1]), (Tp, B, blank, fill, 'packed rows')
    assert np.array_equal(outs[0], outs[1])
    # n_frames NULL: all Tp frames
    full = np.full(B, Tp, np.int32)
    wf = collapse_want(idx, maxp, full, blank)
    tok, cnt, sc = (t.cpu().numpy() for t in eng.ctc_collapse(dev(idx), dev(maxp), None, blank=blank))
    assert np.array_equal(tok, wf[0]) and np.array_equal(cnt, wf[1]) and np.array_equal(bits(sc), bits(wf[2]))
    if B > 1:
        assert (cnt[5::7] == Tp).all() and (tok[5::7] >= 0).all()          # the all-distinct pattern: no -1 in the row
    # history rows: R = B + 3 rows of ld_in frames, utterance b reads row in_rows[b] with ITS OWN n_frames[b]
    rng = np.random.default_rng(Tp + B)
    R = B + 3
    extra = dr.collapse_cases(Tp, R, VC, blank, seed=1)
    lists = {'permutation': rng.permutation(R)[:B], 'skips rows': np.arange(3, R)}
    if B > 1:
        twice = rng.permutation(R)[:B]
        twice[B // 2] = twice[0]
        lists['one row twice'] = twice
    for ld_in in (Tp, Tp + 37):
        hi = rng.integers(0, VC, (R, ld_in)).astype(np.int32)
        hp = rng.uniform(0, 1, (R, ld_in)).astype(np.float32)
        hi[:, :Tp], hp[:, :Tp] = extra[0], extra[1]
        for name, in_rows in lists.items():
            in_rows = in_rows.astype(np.int32)
            w = collapse_want(hi[in_rows, :Tp], hp[in_rows, :Tp], nfr, blank)
            rows = eng.op_ctc_collapse_rows(dev(hi), dev(hp), dev(nfr), in_rows=dev(in_rows), Tp=Tp, blank=blank).cpu().numpy()
            assert np.array_equal(rows, np.concatenate([w[0], w[1][:, None], bits(w[2])[:, None]], 1)), (Tp, B, blank, ld_in, name)


def test_ctc_collapse_refusals(eng):
    """refusals only, nothing launched: a Tp whose max-probs (Tp * 4 bytes of dynamic LDS) pass the kernel's default limit is
    refused by name by masr_ctc_collapse and masr_op_ctc_collapse_rows (masr_transcribe_* and masr_pool_step carry the same
    refusal); the new entry also refuses null pointers, negative sizes and ld_in < Tp.  The buffers have the full size."""
    Tp = 16385
    idx = torch.zeros(1, Tp, dtype=torch.int32, device='cuda')
    mp = torch.zeros(1, Tp, device='cuda')
    n = torch.zeros(1, dtype=torch.int32, device='cuda')
    with pytest.raises(_lib.MasrError, match='masr_ctc_collapse: more than 16384 frames'):
        eng.ctc_collapse(idx, mp, n)
    with pytest.raises(_lib.MasrError, match='masr_op_ctc_collapse_rows: more than 16384 frames'):
        eng.op_ctc_collapse_rows(idx, mp, n)
    with pytest.raises(_lib.MasrError, match='masr_op_ctc_collapse_rows: more than 16384 frames'):
        eng.op_ctc_collapse_rows(idx, mp, n, in_rows=n)
    rows = torch.zeros(1, 66, dtype=torch.int32, device='cuda')
    f = eng.lib.masr_op_ctc_collapse_rows
    for args, msg in [((ptr(None), ptr(mp), ptr(n), ptr(None), 64, 1, 64, 0, ptr(rows)), 'null argument'),
                      ((ptr(idx), ptr(None), ptr(n), ptr(None), 64, 1, 64, 0, ptr(rows)), 'null argument'),
                      ((ptr(idx), ptr(mp), ptr(None), ptr(None), 64, 1, 64, 0, ptr(rows)), 'null argument'),
                      ((ptr(idx), ptr(mp), ptr(n), ptr(None), 64, 1, 64, 0, ptr(None)), 'null argument'),
                      ((ptr(idx), ptr(mp), ptr(n), ptr(None), 64, -1, 64, 0, ptr(rows)), 'must not be negative'),
                      ((ptr(idx), ptr(mp), ptr(n), ptr(None), 64, 1, -1, 0, ptr(rows)), 'must not be negative'),
                      ((ptr(idx), ptr(mp), ptr(n), ptr(n), 63, 1, 64, 0, ptr(rows)), 'ld_in must be at least Tp')]:
        assert f(eng.h, *args, stream()) != 0
        assert msg in eng.lib.masr_last_error().decode()
    assert f(eng.h, ptr(idx), ptr(mp), ptr(n), ptr(None), 64, 0, 64, 0, ptr(rows), stream()) == 0       # B = 0: nothing to do


# ---- d. pruning -----------------------------------------------------------------------------------------------------------------
def topk(eng, probs, top_n, cutoff, blank=None):
    M, V = probs.shape
    idx = torch.full((M, max(top_n, 1)), -7, dtype=torch.int32, device='cuda')
    lp = torch.full((M, max(top_n, 1)), 7.0, device='cuda')
    cnt = torch.full((M,), -7, dtype=torch.int32, device='cuda')
    if blank is None:
        _lib.check(eng.lib.masr_ctc_topk(eng.h, ptr(probs), M, V, top_n, C.c_float(cutoff), ptr(idx), ptr(lp), ptr(cnt), stream()))
        return idx.cpu().numpy(), lp.cpu().numpy(), cnt.cpu().numpy(), None
    blp = torch.full((M,), 7.0, device='cuda')
    _lib.check(eng.lib.masr_ctc_topk_blank(eng.h, ptr(probs), M, V, top_n, C.c_float(cutoff), blank, ptr(idx), ptr(lp), ptr(cnt),
                                           ptr(blp), stream()))
    return idx.cpu().numpy(), lp.cpu().numpy(), cnt.cpu().numpy(), blp.cpu().numpy()


WORST_LOG = {'ulp': 0.0}


def log_distance(got, want64, p, where):
    """largest |got - want64| in float32 ulp of the result (``got``: what the kernel wrote); a new overall maximum is printed with
    its probability, both values and the distance it would have in ulp of the float64 value"""
    got64 = got.astype(np.float64)
    d = np.abs(got64 - want64) / np.maximum(dr.ulp32(got64), 2.0 ** -149)
    i = int(d.argmax())
    if d[i] > WORST_LOG['ulp']:
        WORST_LOG['ulp'] = float(d[i])
        print(f'PRUNE worst so far {where}: p = {float(p[i])!r} log -> {float(got[i])!r}, float64 {float(want64[i])!r}: {d[i]:.3f} ulp of the '
              f'result, {abs(got64[i] - want64[i]) / max(float(dr.ulp32(want64[i:i + 1])[0]), 2.0 ** -149):.3f} ulp of the float64 value', flush=True)
    return float(d[i])


@pytest.mark.parametrize('V', [1, 3, 40, 256, 257, 8192, 8193, 16384])
def test_ctc_topk_against_exact_pruning(eng, V):
    """decode_ref.prune_cases (Dirichlet peaked and flat, dyadic rows whose cumulative sum reaches cutoff 0.5 / 0.75 / 0.875
    exactly, bit-equal probabilities at the thread / lane / wave placements, exact zeros behind a few entries) at top_n 1, 5, 40,
    64 and V + 3, cutoff_prob 1.0, 0.99, 0.875, 0.75, 0.5, M = 300 and M = 1, through masr_ctc_topk and masr_ctc_topk_blank: the
    indices and the counts are exactly those of decode_ref.prune; log-probabilities and blank_logp are within 2 float32 ulp of the
    float64 logarithm, in ulp of the result (HIP documents logf at 1 ulp; the second covers the comparison's own rounding), p[blank] == 0 gives -inf.
    Slots at or behind the count are not looked at.

    Found by this test: indices, counts and the -inf held, but topk_prune_kernel took its logarithms with logf, which was up to
    2.138 float32 ulp from the float64 logarithm (2.004 at V = 3 .. 2.138 at V = 16384; e.g. p = 0.4603322148323059 ->
    -0.7758069634437561 against -0.7758068440071811, p = 1.4212614587449934e-05 -> -11.161382675170898 against -11.161380636478613).
    The kernel now takes log(p + FLT_MIN) and log(p[blank]) in double and rounds once; the candidates' logarithms are taken
    behind the selection rounds, one winner per thread, where thread 0 took them inside every round before."""
    rows = dr.prune_cases(V)
    orders = [dr.sort_order(r) for r in rows]
    drows = dev(rows)
    worst = 0.0
    with np.errstate(divide='ignore'):
        blank_want = np.log(rows.astype(np.float64))
    for top_n in (1, 5, 40, 64, V + 3):
        for cutoff in (1.0, 0.99, 0.875, 0.75, 0.5):
            ref = [dr.prune(rows[r], top_n, cutoff, order=orders[r]) for r in range(len(rows))]
            blank = (top_n + int(cutoff * 8)) % V
            for M in (300, 1):
                for with_blank in (False, True):
                    r1 = 5 * (top_n % 3) + 3 if M == 1 else 0                        # M = 1: a tie row, a dyadic row, ...
                    idx, lp, cnt, blp = topk(eng, drows[r1:r1 + M], top_n, cutoff, blank if with_blank else None)
                    for i in range(M):
                        ri, rl, rc = ref[r1 + i]
                        where = (V, top_n, cutoff, M, with_blank, r1 + i)
                        assert cnt[i] == rc, where
                        assert np.array_equal(idx[i, :rc], ri), where
                        worst = max(worst, log_distance(lp[i, :rc], rl, rows[r1 + i, ri], where))
                    if with_blank:
                        bw = blank_want[r1:r1 + M, blank]
                        zero = rows[r1:r1 + M, blank] == 0
                        assert (blp[zero] == -np.inf).all(), (V, top_n, cutoff, M)
                        if (~zero).any():
                            worst = max(worst, log_distance(blp[~zero], bw[~zero], rows[r1:r1 + M, blank][~zero], (V, top_n, cutoff, M, 'blank')))
            if top_n > V and cutoff == 1.0:
                assert all(rc == V for _, _, rc in ref)
    print(f'PRUNE V={V}: largest log distance {worst:.3f} float32 ulp of the result (all V so far {WORST_LOG["ulp"]:.3f})', flush=True)
    assert worst <= 2.0, f'log-probabilities {worst:.3f} float32 ulp from the float64 logarithm'


def test_ctc_topk_refusals(eng):
    p = torch.full((2, 8), 0.125, device='cuda')
    big = torch.zeros(1, 16385, device='cuda')
    with pytest.raises(_lib.MasrError, match='top_n must be positive'):
        topk(eng, p, 0, 1.0)
    with pytest.raises(_lib.MasrError, match='top_n must be positive'):
        topk(eng, p, -3, 1.0, blank=0)
    with pytest.raises(_lib.MasrError, match='V > 16384'):
        topk(eng, big, 4, 1.0)
    with pytest.raises(_lib.MasrError, match='V > 16384'):
        topk(eng, big, 4, 1.0, blank=0)
    for blank in (-1, 8):
        with pytest.raises(_lib.MasrError, match='blank id out of range'):
            topk(eng, p, 4, 1.0, blank=blank)
