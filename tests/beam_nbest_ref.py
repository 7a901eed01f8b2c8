"""numpy reference of the n-best kernel (csrc/beam_nbest.hip): rank the live set a prefix search left behind, walk N parent chains.

Order = the search's own best pick: higher score first, of BIT-equal scores the smaller last character, of equal (score,
character) the smaller live index.  Scores are compared as order-preserving integers of their bits (so -inf and equal bits are
what they are), never as floats."""
import numpy as np


def score_key(score):
    """float32 array -> uint32 keys: a larger float is a larger key, equal bits are equal keys"""
    u = np.ascontiguousarray(score, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def rank_order(score, ch):
    """live indices, best first"""
    key = score_key(score).astype(np.int64)
    return sorted(range(len(key)), key=lambda i: (-int(key[i]), int(ch[i]), i))


def walk(node, pool_parent, pool_ch, pool_cap):
    """tokens root to leaf of the prefix whose last trie node is ``node``; the walk stops at x <= 0 or x >= pool_cap"""
    out, x = [], int(node)
    while 0 < x < pool_cap:
        out.append(int(pool_ch[x]))
        x = int(pool_parent[x])
    return out[::-1]


def nbest(n_live, node, ch, score, pool_parent, pool_ch, nbest, max_len, tokens_in=None):
    """one utterance -> (tokens [nbest, max_len], len [nbest], score [nbest] float32, count).  Rows past count: len 0, score -inf,
    tokens as ``tokens_in`` gave them (so are positions a row does not write); a chain longer than max_len keeps its full length
    and its first max_len tokens."""
    pool_cap = len(pool_parent)
    toks = np.full((nbest, max_len), -7, np.int32) if tokens_in is None else np.array(tokens_in, np.int32).reshape(nbest, max_len)
    lens = np.zeros(nbest, np.int32)
    out = np.full(nbest, -np.inf, np.float32)
    order = rank_order(np.asarray(score, np.float32)[:n_live], np.asarray(ch)[:n_live])
    count = min(nbest, n_live)
    for r in range(count):
        i = order[r]
        chain = walk(node[i], pool_parent, pool_ch, pool_cap)
        lens[r] = len(chain)
        toks[r, :min(len(chain), max_len)] = chain[:max_len]
        out[r] = np.float32(score[i])
    return toks, lens, out, count
