"""CPU: tests/decode_ref.py -- the exact references of tests/test_gpu_decode_edges.py -- against the oracle/ package: the collapse
against the greedy decoder tests/test_gpu_parity.py::test_ctc_collapse_against_oracle uses, the pruning against the pruning step
of the prefix search tests/test_beam_search.py compares with; on random Dirichlet rows and on the designed rows of the GPU tests."""
import numpy as np
import pytest

from oracle import beam_search as obs, decoders as od
from tests import decode_ref as dr


def test_argmax_first_takes_the_first_maximum():
    rows = np.array([[1, 3, 3, 2], [5, 5, 5, 5], [-2, -1, -1, -3], [0, 0, 0, 7]], np.float32)
    idx, m = dr.argmax_first(rows)
    assert idx.tolist() == [1, 0, 1, 3] and m.tolist() == [3, 5, -1, 7]
    for V in (1, 2, 65, 257, 8193):
        rows = dr.argmax_cases(V)
        idx, m = dr.argmax_first(rows)
        assert np.array_equal(idx, rows.argmax(-1)) and np.array_equal(m, rows.max(-1))
        assert idx[-1] == 0                                        # the all-equal row
        for (a, b), r in zip(dr.tie_pairs(V), range(len(rows) - 2 - len(dr.tie_pairs(V)), len(rows) - 2)):
            assert rows[r, a] == rows[r, b] == rows[r].max() and idx[r] == a


def as_probs(idx, maxp, V):
    """a probability matrix whose argmax / max are (idx, maxp): what greedy_decoder reads"""
    p = np.zeros((len(idx), V), np.float32)
    p[np.arange(len(idx)), idx] = maxp
    return p


@pytest.mark.parametrize('blank', [0, 255])
@pytest.mark.parametrize('Tp', [1, 63, 64, 65, 129, 200])
def test_collapse_against_the_oracle_greedy_decoder(Tp, blank):
    V = 256
    vocab = [chr(0x4e00 + i) for i in range(V)]
    idx, maxp, nfr = dr.collapse_cases(Tp, 70, V, blank)
    for b in range(70):
        n = min(int(nfr[b]), Tp)
        tokens, count, score = dr.collapse(idx[b], maxp[b], nfr[b], blank)
        s_ref, t_ref = od.greedy_decoder(as_probs(idx[b, :n], maxp[b, :n], V), vocab, blank) if n else (0, '')
        assert ''.join(vocab[i] for i in tokens) == t_ref and count == len(tokens)
        assert float(score) * 100.0 == s_ref
        assert score.dtype == np.float32
    if Tp == 200:                                                  # the designed patterns say what they are meant to say
        a, c, d, e = ([t for t in range(V) if t != blank][10:14])
        full = {b % 7: dr.collapse(idx[b], maxp[b], Tp, blank)[0] for b in range(7)}
        assert full[0].count(a) == 1 and full[0].count(c) == 1
        assert full[1].count(a) == 2 and full[1].count(c) == 2
        assert [full[2].count(t) for t in (a, d, c, e)] == [1, 1, 1, 1]
        assert full[3] == [] and full[4] == [a] and len(full[5]) == Tp
        assert dr.collapse(idx[3], maxp[3], Tp, blank)[2] == 0


def test_collapse_score_is_the_sequential_float32_sum():
    p = np.array([1.0, 1e-3, 1e-3, 1e-3, 0.5, 3e-3] * 20, np.float32)
    idx = np.ones(len(p), np.int32)
    _, _, score = dr.collapse(idx, p, len(p), 0)
    acc = np.float32(0)
    for v in p:
        acc = np.float32(acc + v)
    assert score == np.float32(acc / np.float32(len(p)))
    rev = np.float32(0)
    for v in np.sort(p):
        rev = np.float32(rev + v)
    assert rev != acc                                              # the order matters for values of these magnitudes


@pytest.mark.parametrize('V', [1, 3, 40, 257, 8193])
def test_prune_against_the_oracle_pruning_step(V):
    rows = dr.prune_cases(V, M=25 if V > 1000 else 60)
    for r, row in enumerate(rows):
        order = dr.sort_order(row)
        for top_n in (1, 5, 40, 64, V + 3):
            for cutoff in (1.0, 0.99, 0.875, 0.75, 0.5):
                idx, logp, count = dr.prune(row, top_n, cutoff, order=order)
                ref = obs.pruned_log_probs(row, float(np.float32(cutoff)), top_n)
                assert count == len(ref) == len(idx), (r, top_n, cutoff)
                assert idx.tolist() == [i for i, _ in ref], (r, top_n, cutoff)
                lp_ref = np.array([float(lp) for _, lp in ref])
                assert (np.abs(logp - lp_ref) <= dr.ulp32(logp)).all()     # the oracle adds FLT_MIN in float64 and rounds the log
                assert count >= 1 and (top_n <= V or cutoff < 1 or count == V)


def test_prune_reaches_a_dyadic_cutoff_exactly():
    rng = np.random.default_rng(1)
    for V in (3, 40, 8193):
        row = dr.dyadic_row(V, rng)
        assert dr.prune(row, 40, 0.5)[2] == 1 and dr.prune(row, 40, 0.75)[2] == 2 and dr.prune(row, 40, 0.875)[2] == 3
        assert dr.prune(row, 2, 0.875)[2] == 2
        idx, logp, count = dr.prune(row, V + 1, 1.0)
        assert count == V and (np.diff(row[idx].astype(np.float64)) <= 0).all()
        zeros = row[idx] == 0
        assert (np.diff(idx[zeros]) > 0).all() and (logp[zeros] == np.log(np.float64(dr.FLT_MIN))).all()


def test_head_designs():
    for V in (5, 257, 8193):
        W, kinds = dr.head_weight(V)
        assert W.shape == (V, 256) and len(kinds) == 256 and {'tie', 'equal', 'pm80', 'margin'} <= set(kinds)
        idx, m = dr.argmax_first(W.T)
        for k, kind in enumerate(kinds):
            top = np.nonzero(W[:, k] == m[k])[0]
            assert idx[k] == top[0]
            assert len(top) == {'tie': 2, 'equal': V, 'pm80': 1, 'margin': 1}[kind]
    # the placements say what their names say
    assert dr.fused_slot(1)[2] == 0 and dr.fused_slot(5)[2] == 1 and dr.fused_slot(4)[2] == 1 and dr.fused_slot(9)[2] == 0
    assert dr.fused_slot(7)[1:] == dr.fused_slot(7 + 256)[1:] and dr.fused_slot(7)[0] != dr.fused_slot(7 + 256)[0]
    assert dr.fused_slot(3)[1] != dr.fused_slot(35)[1] and dr.fused_slot(3)[0] == dr.fused_slot(35)[0]
    assert sorted(dr.fused_slot(c)[2:] for c in range(32)) == sorted((h, r) for h in (0, 1) for r in range(16))
