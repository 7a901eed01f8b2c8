"""Plain numpy / Python restatements of the decode tail (csrc/elementwise.hip: argmax_rows_kernel, ctc_collapse_kernel,
topk_prune_kernel; the fused head of csrc/rowgemm.hip) and the designed inputs of tests/test_gpu_decode_edges.py.  A helper module:
no GPU, no torch kernels; tests/test_decode_ref_cpu.py holds it against the oracle/ package.

Every result here is defined exactly -- an index, a count, a sequential float32 sum, a float64 cumulative sum -- so the GPU tests
compare bit for bit.  Where include/masr_hip.h and the reference's decoder are silent (NaN inputs, slots behind a returned count)
nothing is defined here either."""
import numpy as np

FLT_MIN = np.float32(1.17549435e-38)


# ---- references ---------------------------------------------------------------------------------------------------------------
def argmax_first(rows):
    """rows [M, V] float32 -> (first index of each row's maximum [M] int32, the maximum [M] float32): np.argmax's tie rule, which
    the reference's greedy decoder relies on (ctc_greedy_decoder.py:20)"""
    rows = np.asarray(rows, np.float32)
    m = rows.max(axis=-1)
    first = (rows == m[..., None]).argmax(axis=-1)          # argmax of a bool array: the first True
    return first.astype(np.int32), m


def collapse(idx, maxp, n, blank):
    """ctc_greedy_decoder.py:20-30 on the first ``n`` frames (clamped to the row): drop repeats, then blanks; the score is the
    Python-order sequential float32 sum of the max-probs of ALL non-blank frames divided by their count, 0 without any
    -> (tokens list, count, np.float32 score)"""
    n = max(0, min(int(n), len(idx)))
    ids = [int(i) for i in idx[:n]]
    tokens, prev = [], None
    for i in ids:
        if i != prev and i != blank:
            tokens.append(i)
        prev = i
    probs = [np.float32(maxp[t]) for t in range(n) if ids[t] != blank]
    if not probs:
        return tokens, len(tokens), np.float32(0.0)
    acc = np.float32(0.0)
    for p in probs:
        acc = np.float32(acc + p)
    return tokens, len(tokens), np.float32(acc / np.float32(len(probs)))


def sort_order(row):
    """indices of ``row`` by (probability descending, index ascending)"""
    return np.argsort(-np.asarray(row, np.float32), kind='stable')


def prune(row_f32, top_n, cutoff_f32, order=None):
    """get_pruned_log_probs as masr_ctc_topk states it: candidates by (probability descending, index ascending), accumulated in
    float64 in that order; the list ends behind the entry with which cum >= float64(float32(cutoff)) when cutoff < 1, at top_n, or
    at V -> (idx [count] int64, float64 log(float32(p + FLT_MIN)) [count], count).  ``order``: sort_order(row) computed before"""
    row = np.asarray(row_f32, np.float32)
    order = sort_order(row) if order is None else order
    k = min(int(top_n), row.shape[0])
    idx = np.asarray(order[:k], np.int64)
    p = row[idx]
    count = k
    cutoff = np.float32(cutoff_f32)
    if cutoff < np.float32(1.0):
        cum = 0.0
        for i in range(k):
            cum += float(p[i])
            if cum >= float(cutoff):
                count = i + 1
                break
    idx, p = idx[:count], p[:count]
    with np.errstate(divide='ignore'):
        logp = np.log((p + FLT_MIN).astype(np.float32).astype(np.float64))
    return idx, logp, count


def ulp32(x64):
    """one float32 ulp at the float32 nearest to x64 (array)"""
    x = np.abs(np.asarray(x64, np.float64)).astype(np.float32)
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


# ---- designed inputs ------------------------------------------------------------------------------------------------------------
def tie_pairs(V):
    """index pairs (a < b) for bit-equal maxima in the 256-thread row kernels (column j sits in thread j & 255, lane j & 63, wave
    (j >> 6) & 3): distance 256 / 512 / 8192 = one thread, 1 / 37 / 63 = two lanes of a wave, 64 / 129 / 192 = two waves; the
    last pair is (0, V - 1)"""
    pairs = []
    for d in (1, 37, 63, 64, 129, 192, 256, 512, 8192):
        for s in (0, 5, V // 2, V - 1 - d):
            if s >= 0 and s + d < V and (s, s + d) not in pairs:
                pairs.append((s, s + d))
    if V > 1 and (0, V - 1) not in pairs:
        pairs.append((0, V - 1))
    return pairs


def argmax_cases(V, seed=0):
    """rows [N, V] float32 for masr_argmax_rows: a unique maximum at column 0, V - 1, every multiple of 64 (so of 256) below V and the
    column before each; bit-equal maxima at tie_pairs(V) (and one triple); a row whose values are all equal"""
    rng = np.random.default_rng(seed + V)
    cols = sorted({0, V - 1} | {c for k in range(64, V, 64) for c in (k, k - 1)})
    pairs = tie_pairs(V)
    rows = rng.standard_normal((len(cols) + len(pairs) + 2, V)).astype(np.float32)
    r = 0
    for c in cols:
        rows[r, c] = 10.0
        r += 1
    for a, b in pairs:
        rows[r, a] = rows[r, b] = 10.0
        r += 1
    for c in {V // 3, V // 2, V - 1}:             # three (or fewer) equal maxima
        rows[r, c] = 10.0
    rows[r + 1, :] = 0.25
    return rows


def dyadic_row(V, rng):
    """0.5, 0.25, 0.125, ... (at most 24 terms, exact in float32 and in every partial float64 sum) at random columns, zeros elsewhere"""
    row = np.zeros(V, np.float32)
    k = min(V, 24)
    row[rng.permutation(V)[:k]] = np.float32(0.5) ** np.arange(1, k + 1, dtype=np.float32)
    return row


def prune_cases(V, M=300, seed=0):
    """rows [M, V] float32 for masr_ctc_topk, the kinds in turn: Dirichlet peaked / flat, dyadic, bit-equal probabilities at
    tie_pairs(V) above a flat floor, exact zeros behind a few non-zero entries"""
    rng = np.random.default_rng(seed + 7 * V)
    pairs = tie_pairs(V)
    rows = np.zeros((M, V), np.float32)
    for r in range(M):
        kind = r % 5
        if kind == 0:
            rows[r] = rng.dirichlet(np.full(V, 0.1)).astype(np.float32)
        elif kind == 1:
            rows[r] = rng.dirichlet(np.full(V, 5.0)).astype(np.float32)
        elif kind == 2:
            rows[r] = dyadic_row(V, rng)
        elif kind == 3:
            rows[r] = (rng.dirichlet(np.full(V, 5.0)) * 0.5).astype(np.float32)
            if pairs:
                a, b = pairs[(r // 5) % len(pairs)]
                rows[r, a] = rows[r, b] = 0.2
                if r % 2:                         # a third equal entry, and a second tie group below the first
                    rows[r, (a + b) // 2] = 0.2
                    rows[r, V - 1 - a] = rows[r, V - 1 - b] = max(rows[r, V - 1 - a], rows[r, V - 1 - b])
        else:
            nz = rng.permutation(V)[:min(V, 1 + r % 4)]
            rows[r, nz] = rng.dirichlet(np.ones(len(nz))).astype(np.float32)
    return rows


def collapse_cases(Tp, B, V, blank, seed=0):
    """(argmax [B, Tp] int32, max-probs [B, Tp] float32, n_frames [B] int32) for the collapse: utterance b has pattern b % 7 and
    n_frames (0, 1, 63, 64, 65, Tp, Tp + 5)[(b // 7) % 7] -- not clamped: the kernel clamps to Tp.  Patterns (frames past Tp fall
    away): 0 a repeat run over frames 60..67 and another over 124..131 (one token each across the 64-frame rounds); 1 the same
    token at 62 and 64 with a blank at 63, and at 127 and 129 with a blank at 128 (two tokens); 2 different tokens at 63 | 64 and
    127 | 128; 3 all blank; 4 one non-blank token throughout; 5 all frames distinct and non-blank; 6 random.  The max-probs mix
    magnitudes 1e-3 .. 1, so their float32 sum depends on the order."""
    rng = np.random.default_rng(seed + 1000 * Tp + B + blank)
    nb = [t for t in range(V) if t != blank]
    small = np.array(nb[:3] + [blank], np.int32)
    idx = np.zeros((B, Tp), np.int32)
    nfr = np.zeros(B, np.int32)
    T = max(Tp, 132)
    for b in range(B):
        pat = b % 7
        row = small[rng.integers(0, 4, T)]                      # repeats and blanks everywhere
        a, c, d, e = nb[10], nb[11], nb[12], nb[13]
        if pat == 0:
            row[60:68], row[124:132] = a, c
        elif pat == 1:
            row[62], row[63], row[64] = a, blank, a
            row[127], row[128], row[129] = c, blank, c
        elif pat == 2:
            row[63], row[64], row[127], row[128] = a, d, c, e
        elif pat == 3:
            row[:] = blank
        elif pat == 4:
            row[:] = a
        elif pat == 5:
            row = np.array(nb[:T], np.int32)
        idx[b] = row[:Tp]
        nfr[b] = (0, 1, 63, 64, 65, Tp, Tp + 5)[(b // 7) % 7]
    if B == 1:
        nfr[0] = Tp + 5
    maxp = (10.0 ** rng.uniform(-3, 0, (B, Tp))).astype(np.float32)
    return idx, maxp, nfr


# ---- the CTC head with designed logits ------------------------------------------------------------------------------------------
def fused_slot(c):
    """where logit column c lives in the fused head (rowgemm.hip, RG_EPI_CTC): wrow_of(t) = 256 t + 32 wave, the tile's 32 columns
    sit at (r & 3) + 8 (r >> 2) + 4 fh -> (tile t, stripe = wave, half-wave fh, accumulator register r)"""
    x = c % 32
    return c // 256, (c % 256) // 32, (x >> 2) & 1, (x & 3) + 4 * (x >> 3)


def head_placements(V):
    """bit-equal top pairs (a < b) placed by fused_slot: two registers of one half-wave; the two half-waves of one tile, the smaller
    index in either; two tiles of one stripe (= j and j + 256: one thread of the softmax kernel), the last tile ragged; two
    stripes, in one tile and in two; columns 0 and V - 1; both sides of 8192 (the softmax kernel's 32 / 64 values per thread)"""
    last = V - 1
    want = [(0, 1), (1, 9), (1, 5), (4, 9), (32 * (last // 32) + 1, 32 * (last // 32) + 5), (7, 7 + 256), (7, 7 + 512),
            (40, 40 + 256 * ((last - 40) // 256)), (3, 35), (10, 200), (31, 250), (20, 300), (0, last), (8191, 8192), (100, 8292),
            (8000, 8200), (8192 - 256, 8192), (last - 256, last)]
    out = []
    for a, b in want:
        if 0 <= a < b < V and (a, b) not in out:
            out.append((a, b))
    return out


def head_weight(V, seed=0):
    """W [V, 256] float32 whose column k is the designed logit row k (the encoder rows are the rows of the 256 x 256 identity), and
    kinds [256]: 'tie' -- two bit-equal maxima 3.0 over 0.3 * Gaussian noise, at head_placements(V) first and at seeded random
    pairs for the rest; 'equal' -- every logit 0.5; 'pm80' -- one +80 over a floor of -80; 'margin' -- a unique maximum 1.0 above
    the largest of Gaussian noise"""
    rng = np.random.default_rng(seed + 13 * V)
    W = (0.3 * rng.standard_normal((V, 256))).astype(np.float32)
    kinds = []
    place = head_placements(V) if V > 1 else []
    for k in range(256):
        if k < len(place):
            a, b = place[k]
            W[a, k] = W[b, k] = 3.0
            kinds.append('tie')
        elif k == len(place):
            W[:, k] = 0.5
            kinds.append('equal')
        elif k < len(place) + 21:
            c = (0, V - 1)[k % 2] if k < len(place) + 3 else int(rng.integers(0, V))
            W[:, k] = -80.0
            W[c, k] = 80.0
            kinds.append('pm80')
        elif k < len(place) + 61:
            W[:, k] = rng.standard_normal(V).astype(np.float32)
            c = (0, V - 1)[k % 2] if k < len(place) + 23 else int(rng.integers(0, V))
            W[c, k] = np.float32(np.delete(W[:, k], c).max() if V > 1 else 0.0) + np.float32(1.0)
            kinds.append('margin')
        else:
            a, b = (sorted(rng.choice(V, 2, replace=False)) if V > 1 else (0, 0))
            W[a, k] = W[b, k] = 3.0
            kinds.append('tie')
    return W, kinds
