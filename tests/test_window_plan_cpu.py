"""CPU: ``serving.window_plan`` -- the decoding windows of a lock-step step (predict.py:283-306) -- at the edges the loop has."""
import pytest

from masr_amd.serving import CONTEXT, OVERLAP, STRIDE, WINDOW, window_plan


@pytest.mark.parametrize('n_frames,is_end,expected', [
    (66, False, []),
    (67, False, [(0, 67)]),
    (130, False, [(0, 67)]),
    (131, False, [(0, 67), (64, 131)]),
    (6, True, []),
    (7, True, [(0, 7)]),
    (70, True, [(0, 67)]),
    (71, True, [(0, 67), (64, 71)]),
])
def test_window_plan_at_the_edges(n_frames, is_end, expected):
    assert (WINDOW, STRIDE, CONTEXT, OVERLAP) == (67, 64, 7, 3)
    assert window_plan(n_frames, is_end) == expected


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
