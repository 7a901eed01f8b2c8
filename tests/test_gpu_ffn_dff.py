"""GPU: the fused FFN family (ffn_pc.hip ffn_pc_kernel / ffn16_kernel, ffn_reduce.hip, the sqz_layer.hip stage kernels, their
weight packers) at d_ff OTHER than 2048, under the budget rule of tests/budget.py exactly as tests/test_gpu_f64_budget.py
applies it: every output against the oracle in float64, at most C = 8 times as far from it as the float32 CPU oracle (max and
rms, valid frames).  No tolerance of its own.

Every other module builds its engines with ``linear_units: 2048`` (16 chunks of 128), which never reaches: the full kernel on
few rows (d_ff = 128: one chunk, every prefetch of "the next chunk" clamped from the first slab on), slices of uneven length
(3, 5, 17 chunks), fewer slices launched than asked for (ny != nsplit: the reduction must add ny partials), more than 16 slices
(the remainder loop of ffn_reduce_kernel behind two full rounds of eight), packed copies and buffer ranges of another size, and
the Squeezeformer stage kernel at its lower edge (d_ff = 256).

Each case names the launch plan (nsplit, cpb, ny) it is built for and asserts it with the restatement in tests/ffn_plan.py;
tests/test_ffn_dff_cpu.py shows that the rule rejects a forward that loses one 128-unit chunk of one FFN at these widths (ratios
>= 1.7e4 against the bar of 8), so a kernel that drops or double-counts one slice cannot pass here.

Shapes: the few-row batch is B = 3, T = 203 (T' = 50, M = 150 = 5 row blocks of 32; 150 = 9 x 16 + 6, so the last 16-row block
is partial).  References are computed once per (checkpoint, batch) and shared by the cases that use them.

Every case prints its figures before it asserts (``BUDGET ...``); with ``MASR_BUDGET_TABLE=<path>`` they are also written there
as a markdown table (docs/LAB_NOTES.md keeps the one measured when this module was added)."""
import os
import time

import numpy as np
import pytest
import torch

from tests import budget
from tests.ffn_plan import plan, slices
from tests.test_gpu_f64_budget import EFF_CONF, SQZ_CONF, WINDOWS, batch, dev, settle

pytestmark = pytest.mark.gpu

V = 512
ROWS = []                                    # (case, output, figures) of this run
FEW = (3, 203)                               # the few-row batch: M = 150
DEPTH = {'conformer': 2, 'efficient_conformer': 5, 'squeezeformer': 4}      # hand-over between layers / stride layer 3 / 1 -> 3
RATE = {'conformer': 4, 'efficient_conformer': 8, 'squeezeformer': 4}


def held(case, key, y64, y32, y, mask=None):
    f = budget.evaluate(y64, y32, y, mask)
    ROWS.append((case, key, f))
    print(budget.line(f'{case} {key}', f), flush=True)
    return f


@pytest.fixture(scope='module', autouse=True)
def table():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    t0 = time.time()
    yield
    print(f'd_ff module: {time.time() - t0:.0f} s wall, {len(ROWS)} figures', flush=True)
    path = os.environ.get('MASR_BUDGET_TABLE')
    if path:
        with open(path, 'w') as f:
            f.write('| case | output | max err | ref max err | ratio max | ratio rms | C |\n|---|---|---|---|---|---|---|\n')
            for case, key, r in ROWS:
                f.write(f'| {case} | {key} | {r["max"]:.2e} | {r["max_ref"]:.2e} | {r["ratio_max"]:.2f} | {r["ratio_rms"]:.2f} | '
                        f'{r["c"]:g} |\n')
            f.write(f'\nwall time of the module: {time.time() - t0:.0f} s\n')


# ---- checkpoints, engines, references -----------------------------------------------------------------------------------------
def model(kind, d_ff, streaming):
    """(state dict, HipEngine keywords, oracle keywords); squeezeformer: d_ff = 256 x feed_forward_expansion_factor"""
    from masr_amd.utils import synthetic
    depth = DEPTH[kind]
    if kind == 'conformer':
        sd = synthetic.conformer_state_dict(0, V, d_ff=d_ff, num_blocks=depth)
        conf, okw = {'num_blocks': depth, 'linear_units': d_ff}, {'streaming': streaming}
    elif kind == 'efficient_conformer':
        sd = synthetic.efficient_conformer_state_dict(0, V, d_ff=d_ff, num_blocks=depth)
        conf, okw = dict(EFF_CONF, num_blocks=depth, linear_units=d_ff), {'streaming': streaming}
    else:
        assert d_ff % 256 == 0
        sd = synthetic.squeezeformer_state_dict(0, V, ff_factor=d_ff // 256, num_blocks=depth, streaming=streaming)
        conf = dict(SQZ_CONF, num_blocks=depth, feed_forward_expansion_factor=d_ff // 256, reduce_idx=1, recover_idx=3)
        okw = {'reduce_idx': 1, 'recover_idx': 3, 'causal': streaming}
    return sd, dict(encoder_conf=conf, vocab_size=V, streaming=streaming, use_model=kind), okw


@pytest.fixture(scope='module')
def engines():
    """one engine per (family, d_ff, streaming), built on first use and closed at the end -> (engine, state dict, oracle keywords)"""
    from masr_amd.engine import HipEngine
    cache = {}

    def get(kind, d_ff, streaming=True):
        key = (kind, d_ff, streaming)
        if key not in cache:
            sd, ekw, okw = model(*key)
            e = HipEngine(sd, **ekw)
            assert e.cfg.d_ff == d_ff
            cache[key] = (e, sd, okw)
        return cache[key]
    yield get
    for e in cache.values():
        e[0].close()


_REFS = {}


def reference(kind, d_ff, streaming, B, T):
    """float32 and float64 oracle forward of one checkpoint on one batch, computed once -> (feats, lens, r32, r64, valid mask)"""
    from oracle import f64
    key = (kind, d_ff, streaming, B, T)
    if key not in _REFS:
        sd, _, okw = model(kind, d_ff, streaming)
        feats, lens = batch(B, T, 1000 * B + T)
        assert int(lens[0]) == T and (B == 1 or int(lens.min()) < T)          # ragged, the first utterance full length
        r32, r64 = f64.both(kind, sd, feats, lens, **okw)
        assert torch.isfinite(r32['probs']).all()
        _REFS[key] = (feats, lens, r32, r64, budget.valid_mask(r64['enc'].shape, lens, RATE[kind]))
    return _REFS[key]


_CHUNK_REFS = {}


def chunk_reference(kind, d_ff, windows):
    from oracle import f64
    from oracle.make_golden import golden_inputs
    key = (kind, d_ff, len(windows))
    if key not in _CHUNK_REFS:
        feats, _ = golden_inputs()
        sd, _, _ = model(kind, d_ff, True)
        _CHUNK_REFS[key] = (feats[:1],) + f64.both_chunks(kind, sd, feats[:1], windows)
    return _CHUNK_REFS[key]


def run_full(case, eng, kind, d_ff, streaming, B, T, keys=None):
    """encode_full + ctc_probs under masr_debug_set ``keys`` against the shared reference -> (figures, enc, probs on the host)"""
    from masr_amd._lib import debug_keys
    e = eng[0]
    feats, lens, r32, r64, mask = reference(kind, d_ff, streaming, B, T)
    with debug_keys(e, keys or {}):
        enc = e.encode_full(dev(feats), dev(lens, torch.int32), -1)
        probs = e.ctc_probs(enc)
        enc, probs = enc.cpu(), probs.cpu()
    assert tuple(enc.shape) == tuple(r64['enc'].shape)
    return [(case, k, held(case, k, r64[k], r32[k], g, mask)) for k, g in (('enc', enc), ('probs', probs))], enc, probs


def frames_out(T):
    return ((T - 1) // 2 - 1) // 2           # conv2d subsampling


# ---- A. few rows offline: one slice per chunk, 1 ... 17 slices ----------------------------------------------------------------
@pytest.mark.parametrize('streaming', [True, False], ids=['streaming', 'full_context'])
@pytest.mark.parametrize('d_ff,nsplit', [(128, 1), (384, 3), (640, 5), (1024, 8), (2176, 17)])
def test_few_rows_offline(engines, d_ff, nsplit, streaming):
    """M = 150, 5 row blocks: nsplit = min(d_ff / 128, 128 / 5 = 25) = d_ff / 128, one chunk per slice.  128: the cap is 1, the
    full kernel runs where 2048 always splits; 384 / 640: a remainder loop only; 1024: exactly one round of eight in the
    reduction; 2176: 8 + 8 + 1."""
    B, T = FEW
    M = B * frames_out(T)
    assert M == 150 and plan(d_ff, M) == (nsplit, 1, nsplit) and nsplit == d_ff // 128
    res, _, _ = run_full(f'A conformer d_ff {d_ff} {"streaming" if streaming else "full-context"} B=3 T=203 nsplit {nsplit}',
                         engines('conformer', d_ff, streaming), 'conformer', d_ff, streaming, B, T)
    settle(res)


# ---- B. uneven slices ---------------------------------------------------------------------------------------------------------
UNEVEN = [  # B, T, d_ff -> M, row blocks, (nsplit, cpb, ny), chunks per slice
    (5, 1003, 640, 1250, 40, (3, 2, 3), (2, 2, 1)),
    (5, 1003, 384, 1250, 40, (3, 1, 3), (1, 1, 1)),
    (6, 1003, 640, 1500, 47, (2, 3, 2), (3, 2)),
    (6, 1003, 384, 1500, 47, (2, 2, 2), (2, 1)),
    (9, 1003, 2176, 2250, 71, (3, 6, 3), (6, 6, 5)),               # 64 row blocks and more: the budget of slices is 256 / row blocks
    (9, 1003, 640, 2250, 71, (3, 2, 3), (2, 2, 1)),
    (3, 403, 2176, 300, 10, (12, 2, 9), (2,) * 8 + (1,)),          # ny != nsplit: nine partials where twelve were asked for
]


@pytest.mark.parametrize('B,T,d_ff,M,rowblocks,want,per_slice', UNEVEN, ids=[f'{c[0]}x{c[1]}-dff{c[2]}' for c in UNEVEN])
def test_uneven_slices(engines, B, T, d_ff, M, rowblocks, want, per_slice):
    assert B * frames_out(T) == M and (M + 31) // 32 == rowblocks
    assert plan(d_ff, M) == want and slices(d_ff, M) == per_slice
    res, _, _ = run_full(f'B conformer d_ff {d_ff} B={B} T={T} plan {want} slices {per_slice}', engines('conformer', d_ff), 'conformer',
                         d_ff, True, B, T)
    settle(res)


# ---- C. the full kernels (tail and head stages) at these widths on few rows -----------------------------------------------------
@pytest.mark.parametrize('streaming', [True, False], ids=['streaming', 'full_context'])
@pytest.mark.parametrize('d_ff', [128, 384, 640, 2176])
def test_full_kernels_on_few_rows(engines, d_ff, streaming):
    """key 13 (ffn_split_blocks) = 0: no split, so the few-row batch runs the full launches with the QKV tail and the conv-module
    head stage -- the 16-row kernel (key 39 = 1, the default) and the 32-row kernel (key 39 = 0), each with packed copies of its
    own order.  Both under the rule, and bit-identical to each other as tests/test_gpu_ffn16.py requires at 2048.

    d_ff = 128: the split cut-over must be a no-op, because the cap of the default plan is already 1.  Key 13 also gates the
    latency-cut layer kernels of few row blocks (few_rows = row blocks < min(key 12, key 13) in encode_full), which replace the
    out-projection / conv-module launches around the FFN and are not bit-identical to them at any width
    (tests/test_gpu_few_rows.py holds the two within 2e-5), so the comparison is made with that path held off (key 29 = 0) on
    both sides: then key 13 = 192 against key 13 = 0 differ in nothing but the FFN plan, and must agree to the bit.  The
    unswitched default run is case A; its difference from the key 13 = 0 run is printed (measured when the test was written:
    2.9e-6 on the streaming build's ``enc``, 1.7e-6 on the full-context build's; both runs 1.0 - 1.3 x the reference's error)."""
    B, T = FEW
    assert plan(d_ff, 150, split_blocks=0) == (1, d_ff // 128, 1)
    eng = engines('conformer', d_ff, streaming)
    name = f'C conformer d_ff {d_ff} {"streaming" if streaming else "full-context"} B=3 T=203 full kernel'
    r16, enc16, probs16 = run_full(f'{name} 16-row', eng, 'conformer', d_ff, streaming, B, T, {'ffn_split_blocks': 0, 'ffn16': 1})
    r32, enc32, probs32 = run_full(f'{name} 32-row', eng, 'conformer', d_ff, streaming, B, T, {'ffn_split_blocks': 0, 'ffn16': 0})
    res = r16 + r32
    assert torch.equal(enc16, enc32), f'max |16-row - 32-row| = {(enc16 - enc32).abs().max().item():.3e}'
    assert torch.equal(probs16, probs32)
    if d_ff == 128:
        assert plan(128, 150) == (1, 1, 1)
        rd, encd, probsd = run_full(f'{name} default keys', eng, 'conformer', d_ff, streaming, B, T)
        print(f'{name}: max |default - key 13 = 0| = {(encd - enc16).abs().max().item():.3e} (includes the few-row layer kernels)', flush=True)
        rl, encl, probsl = run_full(f'{name} key 29 = 0', eng, 'conformer', d_ff, streaming, B, T, {'few_rows_path': 0})
        rf, encf, probsf = run_full(f'{name} keys 29 = 0, 13 = 0', eng, 'conformer', d_ff, streaming, B, T,
                                    {'few_rows_path': 0, 'ffn_split_blocks': 0})
        res += rd + rl + rf
        assert torch.equal(encl, encf), f'max |key 13 = 192 - key 13 = 0| = {(encl - encf).abs().max().item():.3e}'
        assert torch.equal(probsl, probsf)
        assert torch.equal(encf, enc16) and torch.equal(probsf, probs16)      # key 29 is moot once key 13 = 0
    settle(res)


# ---- D. chunk steps -------------------------------------------------------------------------------------------------------------
def chunk_steps(e, feats, n, windows, export=False):
    """n lock-step streams fed with the same features -> probabilities [n, T', V] (+ the first stream's exported caches)"""
    x = dev(feats.expand(n, -1, -1))
    sids = [e.stream_open(400) for _ in range(n)]
    try:
        outs = [e.encode_chunk(sids, x[:, cur:cur + k].contiguous())[0] for cur, k in windows]
        caches = e.stream_export_cache(sids[0]) if export else None
    finally:
        for s in sids:
            e.stream_close(s)
    return torch.cat(outs, dim=1).cpu(), caches


@pytest.mark.parametrize('d_ff', [128, 640, 2176])
def test_chunk_steps(engines, d_ff):
    """five 67-frame windows (16 rows per stream and step) and a short last chunk (2 rows):
      1 stream:   M = 16, 1 row block,   nsplit = nchunk (1, 5, 17)
      3 streams:  M = 48, 2 row blocks,  nsplit = nchunk
      40 streams: M = 640, 20 row blocks, nsplit = min(nchunk, 6): 640 -> cpb 1, ny 5; 2176 -> cpb 3, ny 6 (3, 3, 3, 3, 3, 2)
    probabilities of every window and every stream; the single stream's exported caches after the last window"""
    nchunk = d_ff // 128
    assert plan(d_ff, 16) == (nchunk, 1, nchunk) and plan(d_ff, 48) == (nchunk, 1, nchunk)
    assert plan(d_ff, 640) == {128: (1, 1, 1), 640: (5, 1, 5), 2176: (6, 3, 6)}[d_ff]
    assert d_ff != 2176 or slices(d_ff, 640) == (3, 3, 3, 3, 3, 2)
    e = engines('conformer', d_ff)[0]
    feats, (p32, a32, c32), (p64, a64, c64) = chunk_reference('conformer', d_ff, WINDOWS)
    res = []
    for n in (1, 3, 40):
        case = f'D conformer d_ff {d_ff} chunks {n} streams plan {plan(d_ff, 16 * n)}'
        got, caches = chunk_steps(e, feats, n, WINDOWS, export=n == 1)
        assert got.shape == (n,) + tuple(p64.shape)
        res.append((case, 'probs', held(case, 'probs', p64.expand(n, -1, -1), p32.expand(n, -1, -1), got)))
        if caches:
            att, cnn = caches
            assert att.shape == a64.shape and cnn.shape == c64.shape
            res += [(case, 'att_cache', held(case, 'att_cache', a64, a32, att)), (case, 'cnn_cache', held(case, 'cnn_cache', c64, c32, cnn))]
    settle(res)


# ---- E. the other families ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d_ff', [640, 128])
def test_efficient_conformer(engines, d_ff):
    """the few-row batch (T' = 25 behind the stride layer: M = 150, then 75) and one chunk-step run of the five windows"""
    B, T = FEW
    nchunk = d_ff // 128
    assert plan(d_ff, 150) == (nchunk, 1, nchunk) and plan(d_ff, 75) == (nchunk, 1, nchunk)
    eng = engines('efficient_conformer', d_ff)
    name = f'E efficient_conformer d_ff {d_ff}'
    res, enc, _ = run_full(f'{name} B=3 T=203', eng, 'efficient_conformer', d_ff, True, B, T)
    assert enc.shape[1] == 25
    wins = WINDOWS[:5]
    feats, (p32, _, _), (p64, _, _) = chunk_reference('efficient_conformer', d_ff, wins)
    sid = eng[0].stream_open(0)
    try:
        got = torch.cat([eng[0].encode_chunk([sid], dev(feats[:, cur:cur + k]))[0][0] for cur, k in wins])
    finally:
        eng[0].stream_close(sid)
    assert got.shape == p64.shape
    res.append((name, 'probs', held(f'{name} chunks', 'probs', p64, p32, got)))
    settle(res)


@pytest.mark.parametrize('factor', [1, 3])
def test_squeezeformer_fused_and_separate(engines, factor):
    """streaming: False, depth 4 with the time reduction behind layer 1 and the recovery at layer 3 (M = 150, 75 in between).
    key 36 (sqz_fused_blocks) = 1: the sqz_layer.hip stage kernels at every resolution -- d_ff = 256 is exactly their lower edge
    (2 x 128: launch_sqz_stage refuses less); key 36 = 0: the separate launches, whose FFN at so few row blocks is the
    d_ff-split kernel with the affine prologue (2 and 6 one-chunk slices) and the post-LayerNorm on the reduction.  Both
    under the rule.

    Bit-identity, as test_squeezeformer_fused_layer_is_bit_identical_to_the_separate_launches requires at 2048: that test runs
    405 / 203 row blocks, where the separate launches are the full FFN kernel and the row-block projections, i.e. the stage
    kernels' own summation order.  At 5 row blocks the separate launches split d_ff (partial sums added by the reduction) and
    split K in the projections (rowgemm_small.hip) -- other orders, so the two differ in the last bits whatever d_ff is
    (measured at d_ff = 256, valid frames: both 1.1 - 1.2 x the reference's error, not equal).  The identity is therefore
    asserted with the separate launches held on the order the stage kernels restate (key 13 = 0: full FFN kernel, key 6 = 0:
    no K-split projection) and the padded frames computed on both sides (key 38 = 0), the same keys on both sides but key 36."""
    B, T = FEW
    d_ff = 256 * factor
    assert plan(d_ff, 150) == (2 * factor, 1, 2 * factor) and plan(d_ff, 75) == (2 * factor, 1, 2 * factor)
    eng = engines('squeezeformer', d_ff, False)
    name = f'E squeezeformer d_ff {d_ff} B=3 T=203'
    mask = reference('squeezeformer', d_ff, False, B, T)[4]
    rf, encf, _ = run_full(f'{name} fused stages', eng, 'squeezeformer', d_ff, False, B, T, {'sqz_fused_blocks': 1})
    rs, encs, _ = run_full(f'{name} separate launches (d_ff split)', eng, 'squeezeformer', d_ff, False, B, T, {'sqz_fused_blocks': 0})
    print(f'{name}: max |fused - separate, default order| on valid frames = '
          f'{np.abs(encf.numpy()[mask] - encs.numpy()[mask]).max():.3e}', flush=True)
    same = {'ffn_split_blocks': 0, 'rowgemm_small': 0, 'skip_padding': 0}
    rfp, encfp, probsfp = run_full(f'{name} fused stages, keys 13 = 6 = 38 = 0', eng, 'squeezeformer', d_ff, False, B, T,
                                   dict(same, sqz_fused_blocks=1))
    rsp, encsp, probssp = run_full(f'{name} separate launches, keys 13 = 6 = 38 = 0', eng, 'squeezeformer', d_ff, False, B, T,
                                   dict(same, sqz_fused_blocks=0))
    print(f'{name}: max |fused - separate, same order| = {(encfp - encsp).abs().max().item():.3e}', flush=True)
    assert torch.equal(encfp, encsp), f'max |fused - separate| = {(encfp - encsp).abs().max().item():.3e}'
    assert torch.equal(probsfp, probssp)
    settle(rf + rs + rfp + rsp)


# ---- refusal ----------------------------------------------------------------------------------------------------------------------
def test_engine_refuses_linear_units_0():
    from masr_amd import _lib
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sd = synthetic.conformer_state_dict(0, V, d_ff=128, num_blocks=1)
    with pytest.raises(_lib.MasrError, match=r'd_ff \(linear_units\) must be a positive multiple of 128, got 0'):
        HipEngine(sd, encoder_conf={'num_blocks': 1, 'linear_units': 0}, vocab_size=V)
