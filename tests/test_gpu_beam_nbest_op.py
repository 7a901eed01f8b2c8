"""masr_op_beam_nbest (the n-best kernel of csrc/beam_nbest.hip on a host-supplied live set and node pool, LM-free) against the numpy
reference tests/beam_nbest_ref.py: tokens, lengths, score BITS and counts are exact -- the kernel ranks and copies, it computes no
float.

Sizes: n_live at 0, 1, nbest - 1, nbest, the wave edge (63, 64, 65) and the workgroup edge (511, 512); nbest 1, beam and one in
between; chains of length 0 (the root), 1, max_len and max_len + 1; siblings under one parent; exact score ties with different and
with equal last characters, -inf scores, all scores equal; B = 1 and B = 3 with different n_live."""
import ctypes as C

import numpy as np
import pytest

from tests import beam_nbest_ref as ref

MAX_LEN = 12
CAP = 700
SENTINEL = -7


def _pool(rng, B):
    """nodes 1 .. MAX_LEN + 1 are one chain from the root (prefix lengths 1 .. MAX_LEN + 1), the last three share parent 5, the
    rest hang under a random earlier node"""
    parent = np.zeros((B, CAP), np.int32)
    for b in range(B):
        parent[b, 0] = -1
        for x in range(1, CAP):
            parent[b, x] = x - 1 if x <= MAX_LEN + 1 else rng.integers(0, x)
        parent[b, CAP - 3:] = 5
    ch = rng.integers(1, 50, (B, CAP)).astype(np.int32)
    ch[:, 0] = -1
    return parent, ch


def _live(rng, B, beam, n_live, scores):
    node = rng.integers(0, CAP, (B, beam)).astype(np.int32)
    fixed = [0, 1, MAX_LEN, MAX_LEN + 1, CAP - 3, CAP - 2, CAP - 1]         # root, short, full, too long, siblings
    for b in range(B):
        k = min(len(fixed), n_live[b])
        node[b, rng.permutation(n_live[b])[:k]] = fixed[:k]
    ch = rng.integers(0, 4, (B, beam)).astype(np.int32)                       # few characters: (score, character) ties
    if scores == 'distinct':
        sc = -rng.permutation(B * beam).reshape(B, beam).astype(np.float32) / 7
    elif scores == 'ties':
        sc = rng.choice(np.array([-np.inf, -3.25, -1.5, 0.0, -1e-30], np.float32), (B, beam))
    elif scores == 'equal':
        sc = np.full((B, beam), -2.75, np.float32)
    else:
        sc = np.full((B, beam), -np.inf, np.float32)
    return node, ch, np.ascontiguousarray(sc, np.float32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _op(eng_h, n_live, node, ch, sc, parent, pch, beam, nbest, max_len=MAX_LEN):
    from masr_amd import _lib
    B = len(n_live)
    n_live = np.ascontiguousarray(n_live, np.int32)
    rows, width = max(nbest, 1), max(max_len, 1)             # (a refused nbest / max_len still gets real arrays)
    toks = np.full((B, rows, width), SENTINEL, np.int32)
    lens = np.full((B, rows), -1, np.int32)
    out = np.zeros((B, rows), np.float32)
    cnt = np.full(B, -1, np.int32)
    rc = _lib.lib().masr_op_beam_nbest(eng_h, _p(n_live), _p(node), _p(ch), _p(sc), _p(parent), _p(pch), B, beam, parent.shape[1],
                                       nbest, _p(toks), max_len, _p(lens), _p(out), _p(cnt))
    return rc, toks, lens, out, cnt


def _check(eng_h, rng, beam, nbest, n_live, scores):
    B = len(n_live)
    parent, pch = _pool(rng, B)
    node, ch, sc = _live(rng, B, beam, n_live, scores)
    rc, toks, lens, out, cnt = _op(eng_h, n_live, node, ch, sc, parent, pch, beam, nbest)
    from masr_amd._lib import check
    check(rc)
    for b in range(B):
        t_ref, l_ref, s_ref, c_ref = ref.nbest(n_live[b], node[b], ch[b], sc[b], parent[b], pch[b], nbest, MAX_LEN,
                                               np.full((nbest, MAX_LEN), SENTINEL, np.int32))
        what = (beam, nbest, n_live, scores, b)
        assert cnt[b] == c_ref, what
        assert np.array_equal(lens[b], l_ref), what
        assert np.array_equal(out[b].view(np.uint32), s_ref.view(np.uint32)), what
        assert np.array_equal(toks[b], t_ref), what
    return lens, cnt


@pytest.fixture(scope='module')
def eng_h():
    from masr_amd import runtime
    return runtime.aux_engine().h


@pytest.mark.gpu
@pytest.mark.parametrize('nbest', [1, 10, 512])
@pytest.mark.parametrize('scores', ['distinct', 'ties'])
def test_nbest_kernel_at_live_set_sizes(eng_h, nbest, scores):
    rng = np.random.default_rng(1000 + nbest)
    seen = set()
    for n in (0, 1, 9, 10, 63, 64, 65, 511, 512):
        lens, cnt = _check(eng_h, rng, 512, nbest, [n], scores)
        seen.update(lens[0, :cnt[0]].tolist())
    if nbest == 512:                 # the whole live set comes back: the root, the one-token, the full and the overlong chain were read
        assert {0, 1, MAX_LEN, MAX_LEN + 1} <= seen


@pytest.mark.gpu
@pytest.mark.parametrize('beam,nbest', [(1, 1), (7, 3), (64, 64), (65, 64), (300, 300)])
@pytest.mark.parametrize('scores', ['ties', 'equal', 'neginf'])
def test_nbest_kernel_ties_and_infinities(eng_h, beam, nbest, scores):
    rng = np.random.default_rng(beam * 31 + nbest)
    for n in sorted({0, 1, max(nbest - 1, 0), nbest, beam}):
        _check(eng_h, rng, beam, nbest, [n], scores)


@pytest.mark.gpu
@pytest.mark.parametrize('beam,nbest,n_live', [(512, 10, (512, 0, 65)), (20, 20, (3, 20, 19)), (300, 7, (6, 7, 300))])
def test_nbest_kernel_batch_of_three_with_different_live_sets(eng_h, beam, nbest, n_live):
    rng = np.random.default_rng(beam + nbest)
    for scores in ('distinct', 'ties'):
        _check(eng_h, rng, beam, nbest, list(n_live), scores)


def _refused(eng_h, match, beam=8, nbest=3, n_live=(4,), max_len=MAX_LEN, edit=None):
    from masr_amd import _lib
    rng = np.random.default_rng(5)
    B = len(n_live)
    parent, pch = _pool(rng, B)
    node, ch, sc = _live(rng, B, max(beam, 1), [min(max(n, 0), max(beam, 1)) for n in n_live], 'distinct')
    if edit:
        edit(node, parent)
    rc, toks, lens, _, cnt = _op(eng_h, list(n_live), node, ch, sc, parent, pch, beam, nbest, max_len)
    assert rc != 0
    msg = _lib.lib().masr_last_error().decode()
    assert 'masr_op_beam_nbest' in msg and match in msg, msg
    assert (toks == SENTINEL).all() and (cnt == -1).all()         # nothing ran


@pytest.mark.gpu
def test_nbest_op_refuses_bad_indices_by_name(eng_h):
    _refused(eng_h, 'nbest = 0', nbest=0)
    _refused(eng_h, 'nbest = 9', nbest=9)
    _refused(eng_h, 'max_len', max_len=0)
    _refused(eng_h, 'n_live', n_live=(9,))
    _refused(eng_h, 'n_live', n_live=(4, -1))
    _refused(eng_h, 'beam_size', beam=513, nbest=3)

    def node_out(node, parent):
        node[0, 2] = CAP
    _refused(eng_h, 'outside the pool', edit=node_out)

    def node_neg(node, parent):
        node[0, 0] = -1
    _refused(eng_h, 'outside the pool', edit=node_neg)

    def parent_up(node, parent):
        parent[0, 40] = 40
    _refused(eng_h, 'parent of pool node 40', edit=parent_up)
