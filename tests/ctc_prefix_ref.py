"""Numpy restatement of the CTC prefix scorer of ``decoder: joint`` (include/masr_hip.h; a helper module: tests import it).

The dtype is a parameter: float64 is the truth, float32 the restatement of the device's arithmetic (the same operations in the
same order, numpy's log / exp for logf / expf).  ``brute_force`` sums over all V^T alignments and is the check of the recursion.

    state of a prefix g over frames 0 .. T - 1: r_n[t], r_b[t] (alignments of g over 0 .. t ending in a non-blank / a blank)
    empty: r_n = -inf, r_b[t] = sum lp[0 .. t][blank], psi = 0
    g . c: phi[t] = r_b[t] if c == last(g) else lse2(r_n[t], r_b[t]);  r_n'[0] = lp[0][c] for the empty g else -inf;  r_b'[0] = -inf;
           r_n'[t] = lse2(r_n'[t-1], phi[t-1]) + lp[t][c];  r_b'[t] = lse2(r_n'[t-1], r_b'[t-1]) + lp[t][blank];
           psi' = r_n'[0], then lse2(psi', phi[t-1] + lp[t][c]) over t >= 1
    eos (id V - 1): psi' = lse2(r_n[T-1], r_b[T-1]);  blank (id 0): -inf"""
import itertools

import numpy as np

BLANK = 0


def log_post(post, dtype=np.float64, is_log=False):
    """[T, V] posteriors as the CTC head leaves them (float32 probabilities) -> their logarithm in ``dtype``; an entry that is not
    > 0 reads as -inf"""
    p = np.asarray(post).astype(dtype)
    if is_log:
        return p
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(p > 0, np.log(np.where(p > 0, p, 1)), -np.inf).astype(dtype)


def lse2(x, y):
    """logaddexp in the dtype of the operands, the way the kernels write it; scalars or arrays"""
    x, y = np.asarray(x), np.asarray(y)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        m = np.maximum(x, y)
        r = m + np.log(np.exp(x - m) + np.exp(y - m))
    return np.where(x == -np.inf, y, np.where(y == -np.inf, x, r)).astype(np.result_type(x, y))


def empty_state(lp):
    """(r_n, r_b) of the empty prefix: the running sum in frame order"""
    T = lp.shape[0]
    rn = np.full(T, -np.inf, lp.dtype)
    rb = np.zeros(T, lp.dtype)
    s = lp.dtype.type(0)
    for t in range(T):
        s = s + lp[t, BLANK]
        rb[t] = s
    return rn, rb


def score(lp, rn, rb, last, cands, is_empty):
    """psi of the prefix with state (r_n, r_b) and last token ``last`` (None: empty) extended by each of ``cands`` -> [M]"""
    T, V = lp.shape
    dt = lp.dtype
    cands = np.asarray(cands, np.int64)
    eos = V - 1
    rep = cands == (-1 if last is None else last)
    psi = lp[0, cands].copy() if is_empty else np.full(len(cands), -np.inf, dt)
    for t in range(1, T):
        phi = np.where(rep, rb[t - 1], lse2(rn[t - 1], rb[t - 1])).astype(dt)
        psi = lse2(psi, phi + lp[t, cands])
    psi = np.where(cands == eos, lse2(rn[T - 1], rb[T - 1]), psi)
    return np.where(cands == BLANK, -np.inf, psi).astype(dt)


def advance(lp, rn, rb, last, c, is_empty):
    """(r_n', r_b') of the prefix extended by ``c`` (neither blank nor eos)"""
    T = lp.shape[0]
    dt = lp.dtype
    ninf = dt.type(-np.inf)
    rn2, rb2 = np.full(T, ninf, dt), np.full(T, ninf, dt)
    rn2[0] = lp[0, c] if is_empty else ninf
    for t in range(1, T):
        phi = rb[t - 1] if c == last else lse2(rn[t - 1], rb[t - 1])
        rn2[t] = lse2(rn2[t - 1], phi) + lp[t, c]
        rb2[t] = lse2(rn2[t - 1], rb2[t - 1]) + lp[t, BLANK]
    return rn2, rb2


def prefix_scores(lp, prefix, cands):
    """the scorer op's outputs for one row: (psi of ``prefix``, psi of ``prefix`` extended by each of ``cands`` [M])"""
    rn, rb = empty_state(lp)
    psi, last = lp.dtype.type(0), None
    for i, c in enumerate(prefix):
        psi = score(lp, rn, rb, last, [c], i == 0)[0]
        rn, rb = advance(lp, rn, rb, last, int(c), i == 0)
        last = int(c)
    return psi, score(lp, rn, rb, last, cands, len(prefix) == 0)


def collapse(path):
    out, prev = [], BLANK
    for s in path:
        if s != BLANK and s != prev:
            out.append(s)
        prev = s
    return out


def brute_force(p, prefix, whole=False):
    """ln of the summed probability of all V^T alignments whose label sequence starts with ``prefix`` (``whole``: IS ``prefix``);
    ``p`` [T, V] probabilities, float64"""
    T, V = p.shape
    prefix, total = list(prefix), 0.0
    for path in itertools.product(range(V), repeat=T):
        lab = collapse(path)
        if (lab == prefix) if whole else (lab[:len(prefix)] == prefix):
            total += float(np.prod([p[t, s] for t, s in enumerate(path)]))
    return np.log(total) if total > 0 else -np.inf
