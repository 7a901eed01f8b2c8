// The process-wide masr_debug_set switches: one struct of ints, one table of (key, name, field).  Host only (no HIP include).
// A launcher reads knobs().field at launch time; production = the in-class defaults, which are written nowhere else.  Keys 2, 16
// and 38 are not here: they are fields of masr_engine (engine_state.h).
#pragma once

namespace masr {

struct Knobs {
    int ffn_variant = 0;          // key 1: diagnostic ablations of the fused FFN kernel (0 = production); 81 = the kernel without weight loads (MFMA-only floor)
    int no_chain = 0;             // key 5: 1 = separate out-projection and pointwise_conv1 kernels (A/B)
    int rowgemm_small = 1;        // key 6 (diagnostics): 0 = no K-split projection kernel
    int attention_fewq = 1;       // key 7 (diagnostics): 0 = always the query-tiled kernel
    int no_ffn_tail = 0;          // key 8: 1 = the QKV projection as its own launch after the first FFN (A/B)
    int no_ffn_head = 0;          // key 9: 1 = depthwise conv and pointwise_conv2 as their own launches before the second FFN (A/B)
    // key 12 (tuning)
    // row blocks (of 32 rows) below which the K-split kernel takes the projection: 4x more, 4x shorter workgroups fill the chip
    // where a 32-row x N workgroup per row block leaves CUs idle (128 lock-step streams = 64 row blocks: chunk call 5.75 -> 5.34 ms;
    // tools/chunk_step_ab.py).  At 124 row blocks (16 x 10 s; the Efficient Conformer's half-rate layers at 32 x 10 s) the row-block
    // kernel is ahead again: 4.56 -> 4.42 ms per forward, 6.11 -> 6.04 ms per Efficient-Conformer pass (tools/offline_size_ab.py,
    // tools/efficient_size_ab.py); 93 row blocks are indifferent
    int rowgemm_small_blocks = 112;
    // row blocks below which the FFN splits d_ff across workgroups (masr_debug_set key 13): up to 191 row blocks the split (256 /
    // rowblocks ways) + its reduction beat one full-d_ff workgroup per row block on a quarter to three quarters of the CUs
    // (128 streams: chunk call 5.34 -> 3.16 ms, 256 streams 6.52 -> 4.99 ms; tools/chunk_step_ab.py)
    int ffn_split_blocks = 192;
    int attention_fold = 1;       // key 14 (diagnostics): 0 = two-term score contraction in attention_kernel
    int embed_split = 1;          // key 15: 0 = the offline embed projection never splits K
    // waves per workgroup of the conv2 implicit GEMM on 128x128 tiles: 8 (default) or 4 (masr_debug_set key 17).  In one kernel
    // trace with both shapes alternating (tools/gemm_waves_trace.py): 1 467 vs 1 486 us on average, 1 437 vs 1 480 us at best.
    int gemm_waves = 8;
    // key 18 (diagnostics): 0 = conv1 writes its output with plain stores
    // the 636 MB of conv1 output (B = 32 x 10 s) are written once and read back from HBM by conv2 whatever the caches do: streaming
    // (non-temporal) stores, 135.3 -> 125.6 us in one kernel trace with both forms alternating, conv2 behind it unchanged
    int conv1_nt = 1;
    int hot_weights = 0;          // key 19 (timing experiment only): every chunk-step layer runs on layer 0's weights
    // masr_debug_set key 20 -- EXPLORATORY precision mode, never the contract path: the big offline GEMMs (conv2, embed projection,
    // the two FFN GEMMs, unfused) run as split-bf16 products on the bf16 matrix pipe (gemm_bf16x3.hip)
    int bf16x3 = 0;
    int gemm_bf16x3_waves = 8;    // key 21: waves per workgroup of the split-bf16 conv2 launch (8 | 4)
    int ffn_x3_rotation = 1;      // key 22: 0 = no per-workgroup chunk rotation in the split-bf16 FFN
    int ffn_packed = 2;           // key 23: 0 = the full FFN launches stream their weights through the wave-private LDS slabs (A/B)
    int ffn_dual = 0;             // key 24: 0 = the full FFN launches run ffn_pc.hip (one accumulator chain per wave) instead of ffn_dual.hip (A/B)
    int rowgemm_packed = 1;       // key 25: 0 = the offline out-proj + pw1 chain and the CTC head stream their weights through LDS slabs (A/B)
    int attention_grouped_fold = 1;   // key 26: 0 = the two-wave, two-term grouped kernel (A/B)
    int ctc_fused_blocks = 160;   // key 27: row blocks from which the fused CTC head (rowgemm EPI_CTC) runs
    int attention_fewq_wgs = 48;  // key 28: offline launches with fewer attention_kernel workgroups than this take the key-split kernel
    int few_rows_path = 1;        // key 29: 0 = offline Conformer layers of few row blocks keep the row-block chain kernel (A/B)
    // masr_debug_set key 30: 1 = few rows: [depthwise conv -> LN -> SiLU -> pointwise_conv2 + residual] as the head stage of the d_ff-split
    // FFN launch (every slice repeats it on its row block's rows; slice 0 publishes them).  Built in round 4 because round 3 priced
    // it at -3.4 us per layer; MEASURED (tools/chunk_lat.py, MASR_AB=30:0,30:1,30:0,30:1, one process, one box): 16 streams 1.177 /
    // 1.162 ms per chunk call without it, 1.199 / 1.170 ms with it; 128 streams 3.011 / 3.017 vs 3.037 / 3.042 ms -- the 128
    // dependent MFMAs + the window loads it adds to EVERY slice's critical path cost what the removed 11 us launch (whose columns
    // spread over 32 workgroups) cost.  Off by default; identical frame decisions either way.
    int split_head = 0;
    int efficient_fused = 1;      // key 31: 0 = Efficient-Conformer layers keep separate out-proj / pw1 / dwconv / pw2 launches (A/B)
    int beam_lm_cache = 1;        // key 32: 0 = the GPU prefix search probes the scorer once per (prefix, candidate) pair (A/B)
    int conv2_mid_fill = 50;      // key 33 (diagnostics): 128 streams: 3.26 -> 3.19 ms per chunk call (tools/chunk_lat.py MASR_AB=33:0,33:50)
    // masr_debug_set key 34: 1 = offline Conformer layers run attention AND the [out-proj -> LN -> pw1 -> GLU] chain as ONE launch
    // (attention.hip attn_chain_kernel: 32 queries x all four heads per workgroup, context rows in LDS).  Built in round 4 (verdict
    // item 6, priced at -0.13 ms per step in round 3), bit-identical to the two launches -- and MEASURED no faster: 58.3 us per launch
    // against 25.9 + 32.7 us (rocprofv3, one trace), 6.428 vs 6.412 ms per 32 x 10 s pass (tools/attn_chain_ab.py): a workgroup that
    // owns 32 queries of all four heads stages four heads' K' / V tiles per 64 MFMAs per wave where attention_kernel's 128 queries of
    // one head stage one -- the saved prologue / epilogue / att round trip is paid back in staging.  Off by default.
    int attn_chain = 0;
    // masr_debug_set key 35: 1 = one-chunk d_ff slices of few rows (<= 8 row blocks) run ffn_coop.hip -- all eight waves on both products
    // (GEMM 1 as 16 x 16 x 4 tiles without a K split, GEMM 2 as 32 x 32 x 2), every weight fragment from packed copies, all loads in
    // flight before the LayerNorm -- instead of the producer / consumer kernel, whose two roles run one after the other when a
    // workgroup owns ONE chunk.  Built in round 4 on the estimate of 2 x 1.7 us of matrix pipe saved per launch; MEASURED slower:
    // 16 streams 1.167 / 1.195 ms per chunk call against 1.135 / 1.109 ms (tools/chunk_lat.py MASR_AB=35:0,35:1,35:0,35:1; with the
    // weights read from the row-major matrices: 1.33 ms -- 16 / 32 cache lines per load instruction).  The launch is bound by its
    // dependent memory round trips (rows written by another XCD, LayerNorm, LDS exchange, partial store), not by the 256 MFMAs.  Off.
    int ffn_coop = 0;
    // masr_debug_set key 36: row blocks from which a full-context Squeezeformer layer runs as attention + the two fused stage kernels of
    // sqz_layer.hip (0 = never: the twelve separate launches, kept for A/B and the bit-identity test).  128 since round 6: the half-rate
    // layers of BASELINE configs[2]'s second pass (144 row blocks, 100 of them valid) are 0.4 ms per call faster fused, on one lane
    // and on two (17.5 -> 17.0 / 19.2 -> 18.8 ms); passes of ~120 half-rate row blocks (32 x 10 s) stay on the d_ff-split launches
    // (fused from 96: 21.2 against 18.9 ms per call of three such passes, round 5)
    int sqz_fused_blocks = 128;
    int beam_narrow = 1;          // key 37: 0 = every frame of the GPU prefix search on the wide (1024-thread) step (A/B, tests)
    int ffn16 = 1;                // key 39: 0 = the full packed FFN launches run the 32-row kernel instead of the 16-row one (A/B)
    int conv2_rows = 1;           // key 40: 0 = the offline conv2 runs on 128x128 tiles instead of full-width 64-row blocks (A/B)
    int conv1_fused = 1;          // key 41: 0 = conv1 runs as its own launch in front of the row-block conv2 (A/B)
    int embed_rows = 1;           // key 42: 0 = the offline embed projection's K quarters run on 128x128 tiles (A/B)
    // masr_debug_set key 43: hidden units per workgroup of the matrix-core form.  8 = the product's choice (4 units at rnn_size <= 512,
    // where 8 leave most CUs without a workgroup: measured 10 - 16 % per step, docs/LAB_NOTES.md 18; 8 units above), 16 = 16 units at
    // rnn_size 1024, -8 = 8 units at every size (the A/B side of the small sizes; the same bits).  The raw value: gru.hip reads any
    // value but 16 and -8 as 8, lstm.hip asks only whether it is -8
    int rnn_mfma_units = 8;
};

struct KnobInfo {
    int key;
    const char* name;
    int Knobs::*field;
    bool experimental;      // the product build (MASR_EXPERIMENTS = 0) refuses a non-zero value: the kernel is not compiled in
};

Knobs& knobs();
const KnobInfo* knob_info(int index);      // row `index` of the table; nullptr past the last row
const KnobInfo* knob_find(int key);        // nullptr: no process-wide switch has this key
int knob_default(const KnobInfo& k);
bool knob_set(int key, int value, Knobs& into = knobs());      // false: unknown key (into: a copy of the table, for queries)
void knobs_reset();                        // every switch back to its default

}  // namespace masr
