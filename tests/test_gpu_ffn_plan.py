"""GPU: the engine launches what masr_ffn_plan says (csrc/ffn_plan.h).  For each engine the FFN calls of one encode_full are
written down here by hand -- which call offers which stage, at how many rows -- the library's plan is asked for each of them, and
the launch counts that masr_profile_select / masr_profile_read report for the three FFN classes (2 plain, 6 with the QKV tail, 7
with the conv-module head) must be the plan's.  The same run stays inside the budget of tests/budget.py against the references
of tests/test_gpu_ffn_dff.py (small synthetic checkpoints, the few-row batch B = 3, T = 203: M = 150)."""
import collections

import pytest

from tests.test_gpu_f64_budget import dev, settle
from tests.test_gpu_ffn_dff import DEPTH, FEW, engines, frames_out, reference, run_full      # noqa: F401 (engines: fixture)

pytestmark = pytest.mark.gpu

K_NO_CHAIN, K_NO_TAIL, K_NO_HEAD, K_SMALL_BLOCKS, K_SPLIT_BLOCKS, K_FEW_ROWS, K_FFN16 = 5, 8, 9, 12, 13, 29, 39
M0 = FEW[0] * frames_out(FEW[1])
KINDS = (2, 6, 7)


def knob(keys, key):
    from masr_amd import _lib
    return keys.get(key, {k: default for k, _, default, _ in _lib.debug_key_table()}[key])


def predicted(d_ff, keys, calls):
    """launches per profile class for ``calls`` = [(M, ask keywords of _lib.ffn_plan)]"""
    from masr_amd import _lib
    got = collections.Counter(_lib.ffn_plan(d_ff, M, keys, **ask).prof for M, ask in calls)
    return {k: got.get(k, 0) for k in KINDS}


def measured(e, kind, d_ff, streaming, keys):
    """launches per profile class of one encode_full under ``keys`` (one run per class: the engine times one class at a time)"""
    import torch
    from masr_amd._lib import debug_keys
    feats, lens = reference(kind, d_ff, streaming, *FEW)[:2]
    out = {}
    with debug_keys(e, keys):
        for k in KINDS:
            e.profile_select(k)
            e.profile_read(True)
            e.encode_full(dev(feats), dev(lens, torch.int32), -1)
            out[k] = e.profile_read(True)[1]
        e.profile_select(0)
    return out


def conformer_calls(e, keys):
    """masr_encode_full: per layer the first FFN offers the QKV tail; the second offers the conv-module head unless the layer is on
    the few-rows path (there only with key 30) or key 5 holds the chain kernel off"""
    few = knob(keys, K_FEW_ROWS) and (M0 + 31) // 32 < min(knob(keys, K_SMALL_BLOCKS), knob(keys, K_SPLIT_BLOCKS))
    second = {} if few or knob(keys, K_NO_CHAIN) else dict(head_ktaps=e.cnn_kernel)
    return [(M0, dict(tail_n=768)), (M0, second)] * e.num_blocks


CONFORMER_KEYS = {
    'defaults': {},
    'full': {K_SPLIT_BLOCKS: 0},
    'full-32row': {K_SPLIT_BLOCKS: 0, K_FFN16: 0},
    'full-no-stages': {K_SPLIT_BLOCKS: 0, K_NO_TAIL: 1, K_NO_HEAD: 1},
}


@pytest.mark.parametrize('name', list(CONFORMER_KEYS))
@pytest.mark.parametrize('d_ff', [640, 2048])
def test_conformer_launches_are_the_plan(engines, d_ff, name):
    from masr_amd import _lib
    assert M0 == 150
    keys = CONFORMER_KEYS[name]
    eng = engines('conformer', d_ff)
    e = eng[0]
    calls = conformer_calls(e, keys)
    want = predicted(d_ff, keys, calls)
    n = 2 * DEPTH['conformer']
    assert want == {'defaults': {2: n, 6: 0, 7: 0}, 'full': {2: 0, 6: n // 2, 7: n // 2}, 'full-32row': {2: 0, 6: n // 2, 7: n // 2},
                    'full-no-stages': {2: n, 6: 0, 7: 0}}[name]
    first = _lib.ffn_plan(d_ff, M0, keys, tail_n=768)
    assert (first.kernel, first.nsplit, first.cpb) == {'defaults': ('PC', d_ff // 128, 1), 'full': ('ROWS16', 1, d_ff // 128),
                                                       'full-32row': ('PC', 1, d_ff // 128), 'full-no-stages': ('ROWS16', 1, d_ff // 128)}[name]
    try:
        got = measured(e, 'conformer', d_ff, True, keys)
        print(f'conformer d_ff {d_ff} {name}: launches {got}, plan {want}', flush=True)
        assert got == want
        res, _, _ = run_full(f'plan conformer d_ff {d_ff} {name}', eng, 'conformer', d_ff, True, *FEW, keys)
        settle(res)
    finally:
        _lib.check(_lib.lib().masr_debug_reset(e.h))


@pytest.mark.parametrize('name,keys', [('defaults', {}), ('full', {K_SPLIT_BLOCKS: 0})])
def test_efficient_conformer_launches_are_the_plan(engines, name, keys):
    """depth 5: grouped layers 0 ... 3 (planar QKV tail), the stride layer 3 (M = 150 -> 75 inside it), layer 4 behind it with 7
    taps.  A layer offers the head only where the caller's own condition takes the fused launches (ffn_plan.h
    ffn_full_row_blocks; never the stride layer)."""
    from masr_amd import _lib
    d_ff, L, stride = 640, DEPTH['efficient_conformer'], 3
    eng = engines('efficient_conformer', d_ff)
    e = eng[0]
    calls, M = [], M0
    for i in range(L):
        K = e.cnn_kernel // 2 if i > stride else e.cnn_kernel
        calls.append((M, dict(tail_n=768, tail_planar=int(i <= stride))))
        fused = i != stride and (M + 31) // 32 >= knob(keys, K_SPLIT_BLOCKS) and K in (15, 7)
        if i == stride:
            M = FEW[0] * ((frames_out(FEW[1]) + 1) // 2)
        calls.append((M, dict(head_ktaps=K) if fused else {}))
    assert M == 75 and e.cnn_kernel == 15
    want = predicted(d_ff, keys, calls)
    assert want == {'defaults': {2: 2 * L, 6: 0, 7: 0}, 'full': {2: 1, 6: L, 7: L - 1}}[name]
    try:
        got = measured(e, 'efficient_conformer', d_ff, True, keys)
        print(f'efficient_conformer d_ff {d_ff} {name}: launches {got}, plan {want}', flush=True)
        assert got == want
        res, _, _ = run_full(f'plan efficient_conformer d_ff {d_ff} {name}', eng, 'efficient_conformer', d_ff, True, *FEW, keys)
        settle(res)
    finally:
        _lib.check(_lib.lib().masr_debug_reset(e.h))


def test_squeezeformer_launches_are_the_plan(engines):
    """depth 4, time reduction behind layer 1 and recovery at layer 3 (M = 150, 75 in between): two affine-prologue FFNs per layer,
    d_ff-split with the post-LayerNorm on the reduction -- the plain class whatever the plan"""
    from masr_amd import _lib
    d_ff, L = 768, DEPTH['squeezeformer']
    eng = engines('squeezeformer', d_ff, False)
    e = eng[0]
    calls = [(75 if 1 <= i < 3 else M0, dict(affine=1)) for i in range(L) for _ in range(2)]
    want = predicted(d_ff, {}, calls)
    assert want == {2: 2 * L, 6: 0, 7: 0}
    assert all(_lib.ffn_plan(d_ff, M, affine=1)[:4] == ('PC', 6, 1, 6) for M, _ in calls)
    try:
        got = measured(e, 'squeezeformer', d_ff, False, {})
        print(f'squeezeformer d_ff {d_ff}: launches {got}, plan {want}', flush=True)
        assert got == want
        res, _, _ = run_full(f'plan squeezeformer d_ff {d_ff}', eng, 'squeezeformer', d_ff, False, *FEW)
        settle(res)
    finally:
        _lib.check(_lib.lib().masr_debug_reset(e.h))
