"""CPU: ``serving.window_plan`` -- the decoding windows of a lock-step step (predict.py:283-306) -- at the edges the loop has, and
``masr_pool_window_plan`` -- the same rule as the C step's room check and lock-step loop apply it (csrc/pool_plan.h) -- held to it."""
import ctypes as C

import pytest

from masr_amd.serving import CONTEXT, OVERLAP, STRIDE, WINDOW, window_plan

EDGES = [
    (66, False, []),
    (67, False, [(0, 67)]),
    (130, False, [(0, 67)]),
    (131, False, [(0, 67), (64, 131)]),
    (6, True, []),
    (7, True, [(0, 7)]),
    (70, True, [(0, 67)]),
    (71, True, [(0, 67), (64, 71)]),
]


@pytest.mark.parametrize('n_frames,is_end,expected', EDGES)
def test_window_plan_at_the_edges(n_frames, is_end, expected):
    assert (WINDOW, STRIDE, CONTEXT, OVERLAP) == (67, 64, 7, 3)
    assert window_plan(n_frames, is_end) == expected


@pytest.fixture(scope='module')
def c_window_plan(built_lib):
    """(n_frames, is_end, cap) -> (the full count, the pairs written): the buffer holds ``cap`` pairs and a guard pair of -1
    behind them, which the call must leave alone; ``cap=None``: asked again with room for the full count"""
    from masr_amd import _lib

    def plan(n_frames, is_end, cap=None):
        n = C.c_int32(-1)
        if cap is None:
            _lib.check(_lib.lib().masr_pool_window_plan(n_frames, int(is_end), None, 0, C.byref(n)))
            cap = n.value
        buf = (C.c_int32 * (2 * cap + 2))(*([-1] * (2 * cap + 2)))
        _lib.check(_lib.lib().masr_pool_window_plan(n_frames, int(is_end), buf, cap, C.byref(n)))
        written = [v for v in buf if v != -1]
        assert list(buf[len(written):]) == [-1] * (2 * cap + 2 - len(written)) and len(written) % 2 == 0
        return n.value, list(zip(written[0::2], written[1::2]))
    return plan


@pytest.mark.parametrize('n_frames,is_end,expected', EDGES)
def test_c_window_plan_at_the_edges(c_window_plan, n_frames, is_end, expected):
    assert c_window_plan(n_frames, is_end) == (len(expected), expected)


def test_c_window_plan_is_the_python_rule_pair_for_pair(c_window_plan):
    for n in range(401):
        for is_end in (False, True):
            want = window_plan(n, is_end)
            assert c_window_plan(n, is_end) == (len(want), want), (n, is_end)


def test_c_window_plan_counts_everything_and_writes_at_most_cap_pairs(c_window_plan):
    want = window_plan(400, True)
    assert len(want) == 7
    assert c_window_plan(400, True, cap=0) == (7, [])                # the count, nothing written
    for cap in (1, 3, 6):
        assert c_window_plan(400, True, cap=cap) == (7, want[:cap])  # exactly cap pairs
    assert c_window_plan(400, True, cap=9) == (7, want)
    for n in (-1, -67, -2 ** 31):
        assert c_window_plan(n, False) == (0, []) and c_window_plan(n, True) == (0, [])


def test_windows_start_a_stride_apart_and_the_last_one_reaches_the_end():
    """every n in 0 .. 400, both flags: consecutive windows start STRIDE apart from 0 and none is longer than WINDOW; a stream
    that goes on gets full windows only.  At the end of a stream with the context's frames the last window ends at n -- except
    where a full window leaves at most OVERLAP frames behind it, which open no window of their own (n = 70: [(0, 67)], the table
    above): there it ends that many frames short of n, never more."""
    short = []
    for n in range(401):
        for is_end in (False, True):
            plan = window_plan(n, is_end)
            assert [a for a, _ in plan] == [k * STRIDE for k in range(len(plan))]
            assert all(0 < b - a <= WINDOW and b <= n for a, b in plan)
            if not is_end:
                assert all(b - a == WINDOW for a, b in plan) and len(plan) == (0 if n < WINDOW else (n - WINDOW) // STRIDE + 1)
        if n >= CONTEXT:
            last = window_plan(n, True)[-1]
            if last[1] != n:
                assert last[1] - last[0] == WINDOW and 0 < n - last[1] <= OVERLAP
                short.append(n)
        else:
            assert window_plan(n, True) == []
    # exactly the n whose tail behind the last full window is 1 .. OVERLAP frames: too few for the context of another window
    assert short == [n for n in range(CONTEXT, 401) if WINDOW < n - (n - CONTEXT) // STRIDE * STRIDE]
    assert short[:4] == [68, 69, 70, 132]
