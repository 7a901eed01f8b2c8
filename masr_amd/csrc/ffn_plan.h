// Which kernel of the fused FFN family one ffn() call launches (engine_layers.hip), as a pure function of the sizes, of what the call
// asks for and of the masr_debug_set switches.  Host only (no HIP include): ffn() evaluates it on knobs(), masr_ffn_plan
// (include/masr_hip.h) on a copy of the defaults with overrides, and tests/test_ffn_plan_cpu.py holds it to tests/ffn_plan.py.
#pragma once
#include <algorithm>

#include "knobs.h"

namespace masr {

enum FfnKernel {
    FFN_X3 = 0,       // ffn_x3.hip: the split-bf16 kernel (experimental)
    FFN_COOP = 1,     // ffn_coop.hip + the split reduction: one-chunk slices, all eight waves on both products (experimental)
    FFN_DUAL = 2,     // ffn_dual.hip: two accumulator chains per wave (experimental)
    FFN_ROWS16 = 3,   // ffn_pc.hip ffn16_kernel: 16-row blocks, two workgroups per CU, packed weights of its own order
    FFN_PC = 4,       // ffn_pc.hip ffn_pc_kernel: 32-row blocks; full or d_ff-split, packed weights or LDS slabs
};

// what a call asks for beyond the block itself (FfnArgs of common.h, reduced to what the choice depends on)
struct FfnAsk {
    int affine = 0;        // affine prologue instead of the LayerNorm (Squeezeformer)
    int tail_n = 0;        // weight rows of the tail stage; 0 = no tail
    int tail_planar = 0;   // the tail writes planar q | k | v (FfnTail::plane_stride > 0)
    int head_ktaps = 0;    // depthwise taps of the head stage; 0 = no head
    int head_norm = 0;     // FfnHead::norm
};

struct FfnPlan {
    int kernel;            // FfnKernel
    int nsplit;            // d_ff slices wished for; 1 = the full kernel
    int cpb, ny;           // chunks of 128 hidden units per slice, slices launched (ffn_slices)
    int packed;            // the kernel reads fragment-ordered weight copies
    int tail_in_kernel;    // the tail / head stage is asked of the kernel; the launcher's return code says whether it ran, and
    int head_in_kernel;    // what the kernel does not run, ffn() or its caller launches
    int split_head;        // the head stage rides on the d_ff-split launch
    int prof;              // masr_profile_select kind of the launch: 2 plain, 6 with tail, 7 with head
};

inline int ffn_row_blocks(int M) { return (M + 31) / 32; }

// nsplit slices wished for -> whole chunks per slice and slices launched (every slice owns at least one chunk)
struct FfnSlices {
    int cpb, ny;
};
inline FfnSlices ffn_slices(int dff, int nsplit) {
    const int nchunk = dff / 128;
    const int cpb = (nchunk + nsplit - 1) / nsplit;
    return {cpb, (nchunk + cpb - 1) / cpb};
}

// d_ff a positive multiple of 128, M > 0.  The switches it reads are, under the names every launcher reads them by:
// knobs().ffn_split_blocks (key 13), knobs().bf16x3 (20, bit 2), knobs().no_ffn_tail (8), knobs().no_ffn_head (9),
// knobs().split_head (30), knobs().ffn_packed (23), knobs().ffn_coop (35), knobs().ffn16 (39), knobs().ffn_dual (24).
inline FfnPlan ffn_plan(const Knobs& k, int d, int dff, int M, const FfnAsk& ask) {
    const bool tail = ask.tail_n > 0, head = ask.head_ktaps > 0;
    const int affine = ask.affine;
    // few rows (streaming chunk steps): split d_ff across workgroups so that >= ~128 CUs work on the block
    int nsplit = 1;
    const int rowblocks = ffn_row_blocks(M);
    if (rowblocks < k.ffn_split_blocks) nsplit = std::min(dff / 128, std::max(1, (rowblocks < 64 ? 128 : 256) / rowblocks));
    // exploratory, bit 2 of key 20: the fused split-bf16 FFN (ffn_x3.hip).  (An unfused version -- LayerNorm, then two split-bf16
    // GEMMs with the hidden tensor in HBM -- measured 44 + 82 + 6 us against the 144 us of the fused exact-fp32 kernel at
    // B = 32 x 10 s: the 65 MB round trip of the hidden tensor ate what the bf16 pipe saved.)
    const bool x3 = (k.bf16x3 & 2) && nsplit == 1 && !affine && d == 256 && dff % 128 == 0;
    // (a planar tail -- the Efficient Conformer's grouped layers -- is ffn_pc.hip's only: with the two-chain kernel switched on the
    // projection stays its own launch)
    const bool want_tail = tail && nsplit == 1 && !k.no_ffn_tail && !x3 && !(ask.tail_planar && k.ffn_dual);
    // (few rows: the head stage rides on the d_ff-split launch, every slice repeating it on the row block's rows -- key 30)
    const bool split_head = head && nsplit > 1 && k.split_head && !affine && !x3 && ask.head_ktaps == 15 && d == 256 && k.ffn_packed >= 2;
    const bool want_head = head && ((nsplit == 1 && !want_tail && !k.no_ffn_head && !affine && !x3 &&
                                     (ask.head_ktaps == 15 || ask.head_ktaps == 7)) || split_head);
    // few rows, one chunk of 128 hidden units per workgroup: the kernel in which all eight waves work on both products (key 35)
    const bool coop = k.ffn_coop && nsplit > 1 && nsplit == dff / 128 && !want_head && !x3 && d == 256;
    // full launches stream PACKED weight copies straight into registers (ffn_pc.hip VAR == 2; built on first use, + 4 MB per FFN)
    const bool packed = k.ffn_packed && (nsplit == 1 || k.ffn_packed >= 2) && d == 256;      // (key 23 = 2: the d_ff-split launches of small M too)
    // 16-row blocks, two workgroups per CU (ffn_pc.hip ffn16_kernel): every full-d_ff launch of packed weights it covers
    const bool use16 = packed && nsplit == 1 && k.ffn16 && !affine && dff % 128 == 0 && !(want_tail && ask.tail_n % 256) &&
                       !(want_head && ask.head_ktaps != 15 && ask.head_ktaps != 7);
    // two accumulator chains per wave (ffn_dual.hip): same arithmetic in the same order, its own packing order
    // (its head stage carries the LayerNorm variant only)
    const bool dual = packed && nsplit == 1 && k.ffn_dual && dff % 256 == 0 && dff >= 512 && !(want_tail && ask.tail_n != 768) &&
                      !(affine && (want_tail || want_head)) && !(want_head && ask.head_norm);
    FfnPlan p{};
    p.kernel = x3 ? FFN_X3 : coop ? FFN_COOP : dual ? FFN_DUAL : use16 ? FFN_ROWS16 : FFN_PC;
    p.nsplit = nsplit;
    const FfnSlices sl = ffn_slices(dff, nsplit);
    p.cpb = sl.cpb; p.ny = sl.ny;
    p.packed = packed;
    p.tail_in_kernel = want_tail; p.head_in_kernel = want_head; p.split_head = split_head;
    p.prof = want_tail ? 6 : want_head ? 7 : 2;
    return p;
}

// Two conditions of ffn()'s callers that read like "the FFN of this call runs split" and are NOT the plan's nsplit > 1
// (docs/LAB_NOTES.md 20, an open question); kept as they are, written once.
// encode_full_efficient: row blocks from which a layer takes the Conformer's fused launches
inline bool ffn_full_row_blocks(const Knobs& k, int M) { return ffn_row_blocks(M) >= k.ffn_split_blocks; }
// masr_encode_full: few row blocks -- the latency-cut kernels of the chunk steps instead of the row-block chain kernel (key 29)
inline bool few_row_blocks(const Knobs& k, int M) {
    return k.few_rows_path && ffn_row_blocks(M) < std::min(k.rowgemm_small_blocks, k.ffn_split_blocks);
}

}  // namespace masr
