"""The launch plan of the fused FFN family, restated in Python (a plain helper module: tests import it).

``ffn_plan()`` in masr_amd/csrc/ffn_plan.h splits d_ff across workgroups when a call has few 32-row blocks, and ``ffn_slices()``
there turns that wish into slices of whole 128-unit chunks (this module is the independent statement: tests/test_ffn_plan_cpu.py
holds the library's ``masr_ffn_plan`` to it):

    rowblocks = ceil(M / 32)                                                       nchunk = d_ff / 128
    nsplit    = min(nchunk, max(1, (rowblocks < 64 ? 128 : 256) / rowblocks))      if rowblocks < ffn_split_blocks (key 13), else 1
    cpb       = ceil(nchunk / nsplit)          chunks per slice
    ny        = ceil(nchunk / cpb)             slices launched = partial sums that ffn_reduce_kernel adds

The tests of d_ff off 2048 assert with it which plan each of their shapes is meant to reach, so that a later change of the
cut-overs makes them say so instead of silently testing something else."""
PC_CH = 128                  # hidden units per chunk (ffn_pc.hip PC_CH, sqz_layer.hip SQ_CH)
SPLIT_BLOCKS = 192           # default of masr_debug_set key 13 (knobs.h ffn_split_blocks)


def plan(d_ff, M, split_blocks=SPLIT_BLOCKS):
    """(nsplit, cpb, ny) of one FFN call on M rows; nsplit = 1 is the full kernel (one slice owning every chunk)"""
    assert d_ff > 0 and d_ff % PC_CH == 0 and M > 0
    nchunk, rowblocks = d_ff // PC_CH, (M + 31) // 32
    nsplit = 1
    if rowblocks < split_blocks:
        nsplit = min(nchunk, max(1, (128 if rowblocks < 64 else 256) // rowblocks))
    if nsplit == 1:
        return 1, nchunk, 1
    cpb = (nchunk + nsplit - 1) // nsplit
    return nsplit, cpb, (nchunk + cpb - 1) // cpb


def slices(d_ff, M, split_blocks=SPLIT_BLOCKS):
    """chunks owned by each launched slice, e.g. (2, 2, 1)"""
    _, cpb, ny = plan(d_ff, M, split_blocks)
    nchunk = d_ff // PC_CH
    return tuple(min(cpb, nchunk - y * cpb) for y in range(ny))


def lose_last_chunk(sd, prefix, d_ff):
    """a copy of a checkpoint in which the FFN under ``prefix`` has lost its last 128 hidden units (the last 32 at d_ff = 128, where
    128 would be the whole block): what a kernel that drops its last slice, or a packer that stops one chunk early, computes"""
    n = 32 if d_ff == PC_CH else PC_CH
    out = dict(sd)
    for k in ('.w_1.weight', '.w_1.bias'):
        t = sd[prefix + k].clone()
        assert t.shape[0] == d_ff
        t[d_ff - n:] = 0
        out[prefix + k] = t
    return out
