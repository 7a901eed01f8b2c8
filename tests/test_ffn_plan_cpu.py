"""CPU: masr_ffn_plan -- the function ffn() in masr_amd/csrc/engine_layers.hip chooses its kernel with (csrc/ffn_plan.h), evaluated by
the library on the switch defaults plus overrides -- against three independent statements:

  1. the split rule of tests/ffn_plan.py, over every accepted d_ff up to 4096, 1 ... 300 row blocks and four cut-overs;
  2. a table of kernels written by hand from ffn() as it stood before the plan was a function of its own;
  3. the conditions under which ffn()'s callers used to restate the plan: the one that moved into it is shown equal over the
     sweep, the two that are NOT equal to it are kept in the C++ (ffn_plan.h ffn_full_row_blocks / few_row_blocks) and the test
     states where they part from it (docs/LAB_NOTES.md records the open question).

No GPU, no engine: the query reads and writes no process state."""
import pytest

from tests.ffn_plan import plan

K_NO_TAIL, K_NO_HEAD, K_SMALL_BLOCKS, K_SPLIT_BLOCKS, K_X3, K_PACKED, K_DUAL, K_FEW_ROWS, K_SPLIT_HEAD, K_COOP, K_FFN16 = (
    8, 9, 12, 13, 20, 23, 24, 29, 30, 35, 39)
D_FFS = range(128, 4097, 128)
ROW_BLOCKS = range(1, 301)
SPLIT_BLOCKS = (0, 64, 192, 1000)
SPLIT_M, FULL = 150, {K_SPLIT_BLOCKS: 0}          # the split call: M = 150 under the defaults; the full call: the same with key 13 = 0


@pytest.fixture(scope='module')
def ffn_plan(built_lib):
    from masr_amd import _lib
    return _lib.ffn_plan


def rows_of(rb):
    return 32 * rb, 32 * rb - 31


# ---- 1. split rule ----------------------------------------------------------------------------------------------------------------
def test_split_rule_is_the_python_restatement(ffn_plan):
    n = 0
    for d_ff in D_FFS:
        for rb in ROW_BLOCKS:
            for M in rows_of(rb):
                for sb in SPLIT_BLOCKS:
                    p = ffn_plan(d_ff, M, {K_SPLIT_BLOCKS: sb})
                    want = plan(d_ff, M, split_blocks=sb)
                    assert (p.nsplit, p.cpb, p.ny) == want, (d_ff, M, sb)
                    if p.nsplit == 1:
                        assert (p.nsplit, p.cpb, p.ny) == (1, d_ff // 128, 1)
                    n += 1
    assert n == 32 * 300 * 2 * 4


def test_the_query_touches_no_process_state_and_refuses_bad_input(ffn_plan):
    from masr_amd import _lib
    before = ffn_plan(2048, SPLIT_M)
    assert ffn_plan(2048, SPLIT_M, FULL).nsplit == 1
    assert ffn_plan(2048, SPLIT_M) == before and before.nsplit == 16          # the override did not stick
    for bad in ((0, 150), (-128, 150), (100, 150), (2048, 0)):
        with pytest.raises(_lib.MasrError):
            ffn_plan(*bad)
    with pytest.raises(_lib.MasrError, match='key 3'):
        ffn_plan(2048, 150, {3: 1})


# ---- 2. kernel table ----------------------------------------------------------------------------------------------------------------
TAIL = dict(tail_n=768)
HEAD15, HEAD7_BN, HEAD31 = dict(head_ktaps=15), dict(head_ktaps=7, head_norm=1), dict(head_ktaps=31)


def test_kernel_table_defaults(ffn_plan):
    for d_ff in (640, 2048):
        p = ffn_plan(d_ff, SPLIT_M, FULL, **TAIL)
        assert (p.kernel, p.tail_in_kernel, p.head_in_kernel, p.packed, p.prof) == ('ROWS16', 1, 0, 1, 6)
        p = ffn_plan(d_ff, SPLIT_M, FULL, **HEAD15)
        assert (p.kernel, p.tail_in_kernel, p.head_in_kernel, p.prof) == ('ROWS16', 0, 1, 7)
        p = ffn_plan(d_ff, SPLIT_M, FULL, **HEAD7_BN)
        assert (p.kernel, p.head_in_kernel) == ('ROWS16', 1)
        for ask in ({}, TAIL, HEAD15):                                  # the split call carries neither stage
            p = ffn_plan(d_ff, SPLIT_M, **ask)
            assert (p.kernel, p.nsplit, p.tail_in_kernel, p.head_in_kernel, p.split_head, p.prof) == ('PC', d_ff // 128, 0, 0, 0, 2)
        for keys in ({}, FULL):                                         # affine (Squeezeformer): never the 16-row kernel
            assert ffn_plan(d_ff, SPLIT_M, keys, affine=1).kernel == 'PC'


def test_kernel_table_switches(ffn_plan):
    d_ff = 2048
    p = ffn_plan(d_ff, SPLIT_M, {**FULL, K_FFN16: 0}, **TAIL)
    assert (p.kernel, p.packed, p.tail_in_kernel) == ('PC', 1, 1)
    for keys in (FULL, {}):
        p = ffn_plan(d_ff, SPLIT_M, {**keys, K_PACKED: 0}, **TAIL)
        assert (p.kernel, p.packed) == ('PC', 0)
    assert ffn_plan(d_ff, SPLIT_M, {K_PACKED: 1}).packed == 0           # key 23 = 1: the full launches only
    assert ffn_plan(d_ff, SPLIT_M, {K_PACKED: 2}).packed == 1
    p = ffn_plan(d_ff, SPLIT_M, {**FULL, K_NO_TAIL: 1}, **TAIL)
    assert (p.kernel, p.tail_in_kernel, p.prof) == ('ROWS16', 0, 2)
    p = ffn_plan(d_ff, SPLIT_M, {**FULL, K_NO_HEAD: 1}, **HEAD15)
    assert (p.kernel, p.head_in_kernel, p.prof) == ('ROWS16', 0, 2)
    for keys in ({}, FULL, {**FULL, K_FFN16: 0}, {**FULL, K_DUAL: 1}, {K_SPLIT_HEAD: 1, K_PACKED: 2}):
        assert ffn_plan(d_ff, SPLIT_M, keys, **HEAD31).head_in_kernel == 0      # 31 taps: never in a kernel


def test_kernel_table_experimental_kernels(ffn_plan):
    dual = {**FULL, K_DUAL: 1}
    for d_ff in (512, 2048):
        p = ffn_plan(d_ff, SPLIT_M, dual, **TAIL)
        assert (p.kernel, p.tail_in_kernel) == ('DUAL', 1)
        assert ffn_plan(d_ff, SPLIT_M, dual, **HEAD15).kernel == 'DUAL'
    for d_ff in (256, 640, 384):                                        # d_ff % 256 != 0 or d_ff < 512
        assert ffn_plan(d_ff, SPLIT_M, dual, **TAIL).kernel == 'ROWS16'
    assert ffn_plan(2048, SPLIT_M, dual, tail_n=512).kernel == 'ROWS16'
    assert ffn_plan(2048, SPLIT_M, dual, **HEAD7_BN).kernel == 'ROWS16'
    assert ffn_plan(2048, SPLIT_M, {K_DUAL: 1}, **TAIL).kernel == 'PC'  # the split call
    # a planar tail (the Efficient Conformer's grouped layers) is ffn_pc.hip's: with key 24 = 1 the caller passed no tail at all,
    # so the two-chain kernel ran the block alone and the projection stayed its own launch
    p = ffn_plan(2048, SPLIT_M, dual, tail_planar=1, **TAIL)
    assert (p.kernel, p.tail_in_kernel) == ('DUAL', 0)
    p = ffn_plan(2048, SPLIT_M, FULL, tail_planar=1, **TAIL)
    assert (p.kernel, p.tail_in_kernel) == ('ROWS16', 1)

    for d_ff in (640, 2048):                                            # key 35: one chunk per slice only
        M = 150 if d_ff == 640 else 32 * 8                              # nsplit = min(nchunk, 128 / row blocks)
        p = ffn_plan(d_ff, M, {K_COOP: 1})
        assert p.nsplit == d_ff // 128 and p.kernel == 'COOP'
    assert ffn_plan(2048, 32 * 10, {K_COOP: 1}).kernel == 'PC'          # 12 slices of 16 chunks
    assert ffn_plan(2048, SPLIT_M, {**FULL, K_COOP: 1}).kernel == 'ROWS16'

    assert ffn_plan(2048, SPLIT_M, {**FULL, K_X3: 2}).kernel == 'X3'
    p = ffn_plan(2048, SPLIT_M, {**FULL, K_X3: 2}, **TAIL)
    assert (p.kernel, p.tail_in_kernel, p.prof) == ('X3', 0, 2)
    assert ffn_plan(2048, SPLIT_M, {**FULL, K_X3: 2}, affine=1).kernel == 'PC'
    assert ffn_plan(2048, SPLIT_M, {K_X3: 2}).kernel == 'PC'            # the split call
    assert ffn_plan(2048, SPLIT_M, {**FULL, K_X3: 1}).kernel == 'ROWS16'        # bit 2 only

    p = ffn_plan(2048, SPLIT_M, {K_SPLIT_HEAD: 1, K_PACKED: 2}, **HEAD15)
    assert (p.kernel, p.nsplit, p.split_head, p.head_in_kernel, p.packed, p.prof) == ('PC', 16, 1, 1, 1, 7)
    assert ffn_plan(2048, SPLIT_M, {K_SPLIT_HEAD: 1, K_PACKED: 1}, **HEAD15).split_head == 0
    assert ffn_plan(2048, SPLIT_M, {K_SPLIT_HEAD: 1, K_PACKED: 2}, head_ktaps=7).split_head == 0
    assert ffn_plan(2048, SPLIT_M, {K_SPLIT_HEAD: 1, K_PACKED: 2, K_COOP: 1}, **HEAD15).kernel == 'PC'     # the head keeps ffn_pc.hip


# ---- 3. the callers' conditions ---------------------------------------------------------------------------------------------------
def test_planar_tail_condition_moved_into_the_plan(ffn_plan):
    """encode_full_efficient passed its grouped layers' planar tail iff ``efficient_fused and not ffn_dual`` (old); now it
    passes it iff ``efficient_fused`` and the plan drops it under ffn_dual (new).  efficient_fused gates the caller on both
    sides; what is left is: [no tail at all under key 24] == [planar tail offered under key 24], plan for plan."""
    for d_ff in D_FFS:
        for rb in ROW_BLOCKS:
            for M in rows_of(rb):
                for sb in SPLIT_BLOCKS:
                    for dual in (0, 1):
                        keys = {K_SPLIT_BLOCKS: sb, K_DUAL: dual}
                        old = ffn_plan(d_ff, M, keys, tail_n=768 if not dual else 0, tail_planar=0 if dual else 1)
                        new = ffn_plan(d_ff, M, keys, tail_n=768, tail_planar=1)
                        assert old == new, (d_ff, M, keys)


def differing_row_blocks(ffn_plan, caller, d_ff, keys=None):
    """row-block counts of the sweep at which a caller's 'this call runs split' disagrees with the plan's nsplit > 1"""
    return [rb for rb in ROW_BLOCKS if any(caller((M + 31) // 32) != (ffn_plan(d_ff, M, keys).nsplit > 1) for M in rows_of(rb))]


def test_efficient_conformer_fused_condition_is_not_the_plan(ffn_plan):
    """encode_full_efficient's ``fused`` asks for (M + 31) // 32 >= ffn_split_blocks (ffn_plan.h ffn_full_row_blocks), "enough
    row blocks for the full launch".  The plan runs the full kernel from 129 row blocks on (256 // rowblocks == 1), and at
    d_ff = 128 always: at 129 ... 191 row blocks (every d_ff) the layers keep their separate launches around a full FFN kernel."""
    def split(rb, sb=192):
        return not rb >= sb
    for d_ff in (256, 640, 2048, 4096):
        diff = differing_row_blocks(ffn_plan, split, d_ff)
        assert (diff[0], diff[-1], len(diff)) == (129, 191, 63)
    diff = differing_row_blocks(ffn_plan, split, 128)
    assert (diff[0], diff[-1], len(diff)) == (1, 191, 191)
    assert differing_row_blocks(ffn_plan, lambda rb: split(rb, 64), 2048, {K_SPLIT_BLOCKS: 64}) == []


def test_encode_full_few_rows_condition_is_not_the_plan(ffn_plan):
    """masr_encode_full's ``few_rows`` is few_rows_path and (M + 31) // 32 < min(rowgemm_small_blocks, ffn_split_blocks)
    (ffn_plan.h few_row_blocks): it also follows the K-split projection's cut-over (key 12 = 112), so at 112 ... 128 row blocks the
    FFN runs split although the layer is not on the few-rows path."""
    def few_rows(rb, small=112, sb=192, path=1):
        return bool(path) and rb < min(small, sb)
    for d_ff in (256, 2048):
        diff = differing_row_blocks(ffn_plan, few_rows, d_ff)
        assert (diff[0], diff[-1], len(diff)) == (112, 128, 17)
    diff = differing_row_blocks(ffn_plan, lambda rb: few_rows(rb, small=200), 2048, {K_SMALL_BLOCKS: 200})
    assert (diff[0], diff[-1], len(diff)) == (129, 191, 63)          # key 12 above key 13: few rows, full FFN kernel
    diff = differing_row_blocks(ffn_plan, lambda rb: few_rows(rb, path=0), 2048, {K_FEW_ROWS: 0})
    assert (diff[0], diff[-1]) == (1, 128)
