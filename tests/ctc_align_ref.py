"""CTC forced alignment restated in plain numpy, from the definition (a helper module: tests import it).

Extended labels blank, y1, blank, ..., yL, blank (S = 2 L + 1 states, blank = 0); a state is reached by staying, from s - 1, or -- an
odd state whose token differs from the previous token -- from s - 2; the path starts in state 0 or 1 and ends in state S - 1 or
S - 2.  Log domain, adds and compares in ``dtype`` only (float32: what masr_ctc_align computes, to the bit; float64: the truth of the
budget tests), NEG for "unreachable", never an infinity.  Tie rule: predecessors in the order stay, s - 1, s - 2, a later one only if
strictly greater; at the end state S - 1 wins a tie against S - 2."""
import itertools

import numpy as np

NEG = -1.0e30


def feasible(tokens, n_frames):
    """a path exists iff the frames hold every token and one blank between adjacent equal tokens"""
    tokens = list(tokens)
    return n_frames >= len(tokens) + sum(a == b for a, b in zip(tokens, tokens[1:]))


def align(logp, tokens, dtype=np.float32):
    """``logp`` [T, V] log-probabilities of the VALID frames, ``tokens`` the L ids -> dict(start [L], end [L] int32 (first / last
    frame of each token's state, inclusive), peak [L] (largest log-probability of the token over them), score, status, path [T]
    (the state per frame)); status 1 (no path): start / end -1, peak / score 0"""
    lp = np.asarray(logp, dtype)
    tokens = [int(t) for t in tokens]
    T, L = lp.shape[0], len(tokens)
    S = 2 * L + 1
    none = dict(start=np.full(L, -1, np.int32), end=np.full(L, -1, np.int32), peak=np.zeros(L, dtype), score=dtype(0), status=1,
                path=np.zeros(0, np.int32))
    if not feasible(tokens, T):
        return none
    if T == 0:
        return dict(none, status=0)
    label = [0 if s % 2 == 0 else tokens[s // 2] for s in range(S)]
    neg = dtype(NEG)
    prev = np.full(S, neg, dtype)
    prev[0] = lp[0, 0]
    if S > 1:
        prev[1] = lp[0, label[1]]
    bp = np.zeros((T, S), np.int8)
    label = np.array(label)
    # may_skip[s]: state s may be entered from s - 2 (a token's state whose token differs from the previous token)
    may_skip = np.zeros(S, bool)
    may_skip[3::2] = label[3::2] != label[1:-2:2]
    for t in range(1, T):
        # all states of the frame at once; per state: stay first, then s - 1, then s - 2, each only if strictly greater
        from1 = np.concatenate([[neg], prev[:-1]]).astype(dtype)
        from2 = np.concatenate([[neg, neg], prev[:-2]]).astype(dtype)[:S]
        best, k = prev.copy(), np.zeros(S, np.int8)
        take = from1 > best
        take[0] = False
        best[take], k[take] = from1[take], 1
        take = may_skip & (from2 > best)
        best[take], k[take] = from2[take], 2
        prev = (best + lp[t, label]).astype(dtype)
        bp[t] = k
    s, score = S - 1, prev[S - 1]
    if S >= 2 and prev[S - 2] > score:
        s, score = S - 2, prev[S - 2]
    path = np.zeros(T, np.int32)
    for t in range(T - 1, -1, -1):
        path[t] = s
        s -= int(bp[t, s])
    start, end, peak = np.full(L, -1, np.int32), np.full(L, -1, np.int32), np.zeros(L, dtype)
    for j in range(L):
        frames = np.nonzero(path == 2 * j + 1)[0]
        start[j], end[j] = frames[0], frames[-1]
        peak[j] = lp[frames, tokens[j]].max()
    return dict(start=start, end=end, peak=peak, score=dtype(score), status=0, path=path)


def align_batch(logp, n_frames, tokens, n_tokens, dtype=np.float32):
    """the padded form of masr_ctc_align: [B, T', V], [B], [B, Lmax], [B] -> (start, end [B, Lmax], peak [B, Lmax], score [B],
    status [B]); slots behind n_tokens[b] are -1 / 0"""
    B, Lmax = np.asarray(tokens).shape
    start, end = np.full((B, Lmax), -1, np.int32), np.full((B, Lmax), -1, np.int32)
    peak, score, status = np.zeros((B, Lmax), dtype), np.zeros(B, dtype), np.zeros(B, np.int32)
    for b in range(B):
        L = int(n_tokens[b])
        r = align(np.asarray(logp)[b, :int(n_frames[b])], np.asarray(tokens)[b, :L], dtype)
        start[b, :L], end[b, :L], peak[b, :L], score[b], status[b] = r['start'], r['end'], r['peak'], r['score'], r['status']
    return start, end, peak, score, status


def path_is_valid(path, tokens):
    """``path`` [T] states: starts in 0 / 1, ends in S - 1 / S - 2, moves by the three transitions only"""
    tokens = [int(t) for t in tokens]
    S = 2 * len(tokens) + 1
    path = [int(s) for s in path]
    if not path:
        return len(tokens) == 0
    if path[0] not in (0, 1) or path[-1] not in (S - 1, S - 2) or min(path) < 0 or max(path) >= S:
        return False
    for a, b in zip(path, path[1:]):
        skip = b - a == 2 and b % 2 == 1 and tokens[b // 2] != tokens[b // 2 - 1]
        if not (b - a in (0, 1) or skip):
            return False
    return True


def path_score(logp, path, tokens, dtype=np.float64):
    """log-probability of a state path in ``logp`` [T, V], summed in frame order in ``dtype``"""
    lp = np.asarray(logp, dtype)
    total = dtype(0)
    for t, s in enumerate(path):
        total = dtype(total + lp[t, 0 if s % 2 == 0 else int(tokens[s // 2])])
    return total


def states_from_spans(start, end, n_frames, n_tokens):
    """the state path that per-token (start, end) frames describe: token j's state on its frames, the blank between tokens j - 1
    and j elsewhere (what the kernel's outputs say about its path)"""
    path = np.zeros(int(n_frames), np.int32)
    j = 0
    for t in range(int(n_frames)):
        while j < n_tokens and t > end[j]:
            j += 1
        path[t] = 2 * j + 1 if j < n_tokens and start[j] <= t <= end[j] else 2 * j
    return path


def brute_force(logp, tokens, dtype=np.float64):
    """every frame labelling over the vocabulary that collapses (merge repeats, drop blanks) to ``tokens`` -> (best score or None,
    the set of labellings that reach it); exponential: tiny cases only"""
    lp = np.asarray(logp, dtype)
    T, V = lp.shape
    tokens = [int(t) for t in tokens]
    best, arg = None, set()
    for lab in itertools.product(range(V), repeat=T):
        col = [k for k, _ in itertools.groupby(lab)]
        if [k for k in col if k != 0] != tokens:
            continue
        sc = dtype(0)
        for t, k in enumerate(lab):
            sc = dtype(sc + lp[t, k])
        if best is None or sc > best:
            best, arg = sc, {lab}
        elif sc == best:
            arg.add(lab)
    return best, arg


def labels_of(path, tokens):
    """state path -> frame labelling"""
    return tuple(0 if s % 2 == 0 else int(tokens[s // 2]) for s in path)
