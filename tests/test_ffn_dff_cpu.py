"""CPU: what tests/test_gpu_ffn_dff.py (the fused FFN kernels at d_ff other than 2048) stands on.

* the budget rule of tests/budget.py sees a lost chunk: a float32 ORACLE forward in which one FFN of one layer has lost its last
  128 hidden units (the last 32 at d_ff = 128) goes through ``budget.evaluate`` in the place of the candidate and must be
  rejected on ``enc`` and on ``probs``, at every width the GPU module runs -- at d_ff = 2176 the lost chunk is 1 / 17 of one
  of four FFNs -- while the undamaged float32 forward with another thread count must pass;
* the Python restatement of the launch plan (tests/ffn_plan.py) gives the plans the GPU cases are built for, and is
  consistent over every accepted width and row-block count;
* ``masr_create`` refuses d_ff = 0, negative and non-multiples of 128 before it touches a device."""
import ctypes

import pytest
import torch

from tests import budget
from tests.ffn_plan import lose_last_chunk, plan, slices

WIDTHS = (128, 384, 640, 2176)


def case_a_batch():
    """B = 3, T = 203 ragged with lens[0] = T: T' = 50, M = 150 (the batch of case A in the GPU module)"""
    from tests.test_gpu_f64_budget import batch
    return batch(3, 203, 3203)


@pytest.mark.parametrize('d_ff', WIDTHS)
def test_the_budget_rule_rejects_a_lost_chunk(d_ff):
    from masr_amd.utils import synthetic
    from oracle import f64
    keep = torch.get_num_threads()
    torch.set_num_threads(min(16, keep))
    try:
        feats, lens = case_a_batch()
        sd = synthetic.conformer_state_dict(0, 512, d_ff=d_ff, num_blocks=2)
        r32, r64 = f64.both('conformer', sd, feats, lens)
        mask = budget.valid_mask(r64['enc'].shape, lens)
        assert r64['enc'].shape[1] == 50
        torch.set_num_threads(1)                                    # a legitimately different float32 summation order
        other = f64.forward('conformer', sd, feats, lens)
        torch.set_num_threads(min(16, keep))
        for k in ('enc', 'probs'):
            f = budget.evaluate(r64[k], r32[k], other[k], mask)
            print(budget.line(f'd_ff {d_ff} undamaged, one thread {k}', f), flush=True)
            assert f['ok'], budget.line(f'd_ff {d_ff} undamaged {k}', f)
        for prefix in ('encoder.encoders.1.feed_forward', 'encoder.encoders.0.feed_forward_macaron'):
            bad = f64.forward('conformer', lose_last_chunk(sd, prefix, d_ff), feats, lens)
            for k in ('enc', 'probs'):
                f = budget.evaluate(r64[k], r32[k], bad[k], mask)
                print(budget.line(f'd_ff {d_ff} {prefix} without its last chunk {k}', f), flush=True)
                assert not f['ok'] and f['ratio_max'] > budget.C and f['ratio_rms'] > budget.C, (prefix, k, f)
    finally:
        torch.set_num_threads(keep)


# (d_ff, M) -> (nsplit, cpb, ny), chunks per slice: every plan tests/test_gpu_ffn_dff.py names
PLANS = [
    # case A / C / E: 3 x 203 frames, M = 150, 5 row blocks
    (128, 150, (1, 1, 1), (1,)), (384, 150, (3, 1, 3), (1, 1, 1)), (640, 150, (5, 1, 5), (1,) * 5),
    (1024, 150, (8, 1, 8), (1,) * 8), (2176, 150, (17, 1, 17), (1,) * 17),
    # case B
    (640, 1250, (3, 2, 3), (2, 2, 1)), (384, 1250, (3, 1, 3), (1, 1, 1)),
    (640, 1500, (2, 3, 2), (3, 2)), (384, 1500, (2, 2, 2), (2, 1)),
    (2176, 2250, (3, 6, 3), (6, 6, 5)), (640, 2250, (3, 2, 3), (2, 2, 1)),
    (2176, 300, (12, 2, 9), (2,) * 8 + (1,)),
    # case D: 1, 3 and 40 lock-step streams of 16 frames
    (128, 16, (1, 1, 1), (1,)), (640, 16, (5, 1, 5), (1,) * 5), (2176, 16, (17, 1, 17), (1,) * 17),
    (640, 48, (5, 1, 5), (1,) * 5), (2176, 48, (17, 1, 17), (1,) * 17),
    (128, 640, (1, 1, 1), (1,)), (640, 640, (5, 1, 5), (1,) * 5), (2176, 640, (6, 3, 6), (3, 3, 3, 3, 3, 2)),
    # Squeezeformer, separate launches: expansion factors 1 and 3 at M = 150 and at 75 behind the time reduction
    (256, 150, (2, 1, 2), (1, 1)), (768, 150, (6, 1, 6), (1,) * 6), (256, 75, (2, 1, 2), (1, 1)), (768, 75, (6, 1, 6), (1,) * 6),
    # the shipped width: 16 chunks, and the full kernel from 129 row blocks on and with key 13 = 0
    (2048, 150, (16, 1, 16), (1,) * 16), (2048, 4080, (2, 8, 2), (8, 8)), (2048, 4114, (1, 16, 1), (16,)),
]


@pytest.mark.parametrize('d_ff,M,want,per_slice', PLANS)
def test_plan_of_the_gpu_cases(d_ff, M, want, per_slice):
    assert plan(d_ff, M) == want
    assert slices(d_ff, M) == per_slice and sum(per_slice) == d_ff // 128
    assert plan(d_ff, M, split_blocks=0) == (1, d_ff // 128, 1)      # key 13 = 0: always the full kernel


def test_plan_is_consistent_at_every_width_and_row_block_count():
    """every slice owns at least one chunk, no more slices than asked for, and the slices cover the chunks exactly"""
    for d_ff in range(128, 4097, 128):
        nchunk = d_ff // 128
        for rowblocks in range(1, 192):
            for M in (32 * rowblocks - 31, 32 * rowblocks):
                nsplit, cpb, ny = plan(d_ff, M)
                assert 1 <= ny <= nsplit <= nchunk, (d_ff, M)
                assert (ny - 1) * cpb < nchunk <= ny * cpb, (d_ff, M)
                assert nsplit * ((M + 31) // 32) <= 256, (d_ff, M)       # the ffpart workspace and the grid stay small
                s = slices(d_ff, M)
                assert len(s) == ny and min(s) >= 1 and sum(s) == nchunk, (d_ff, M)
        assert plan(d_ff, 32 * 192) == (1, nchunk, 1)


@pytest.mark.parametrize('kind,kernel', [(0, 15), (1, 31), (2, 15)], ids=['conformer', 'squeezeformer', 'efficient_conformer'])
@pytest.mark.parametrize('d_ff', [0, -128, 2000])
def test_masr_create_refuses_d_ff(built_lib, kind, kernel, d_ff):
    """0 % 128 == 0 and -128 % 128 == 0: both passed the old remainder test, and ffn() would then have launched the fused kernels
    with no chunks.  The check sits in front of the first device call, so the refusal needs no GPU."""
    from masr_amd import _lib
    cfg = _lib.MasrConfig(model_kind=kind, d_model=256, heads=4, d_ff=d_ff, num_blocks=2, cnn_kernel=kernel, n_mels=80,
                          vocab_size=512, causal=1, max_pos=5000, device_id=0)
    if kind == 1:
        cfg.reserved[0], cfg.reserved[1] = -1, -1
    if kind == 2:
        cfg.reserved[0], cfg.reserved[1], cfg.reserved[2] = 3, 4, 3
    h = ctypes.c_void_p()
    rc = _lib.lib().masr_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = _lib.lib().masr_last_error().decode()
    assert rc != 0 and not h.value
    assert 'd_ff' in msg and 'positive multiple of 128' in msg and str(d_ff) in msg, msg
