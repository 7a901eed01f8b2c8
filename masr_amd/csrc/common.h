// Shared declarations for the MI355X (gfx950) MASR inference kernels.
// Everything here is internal to libmasr_hip.so; the public C ABI is include/masr_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knobs.h"
#include "lm_scorer.h"

struct masr_resample_feed;      // include/masr_hip.h
struct masr_resample_rate;

// MASR_EXPERIMENTS = 1 (MASR_BUILD_EXPERIMENTS=1 at build time): the measured-and-rejected kernels of earlier rounds are compiled
// in and reachable through their masr_debug_set keys (ffn_dual.hip, ffn_coop.hip, ffn_x3.hip, gemm_bf16x3.hip, attn_chain_kernel,
// the head stage on d_ff-split launches).  The default build holds the product kernels only; those keys then fail loudly.
#ifndef MASR_EXPERIMENTS
#define MASR_EXPERIMENTS 0
#endif

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace masr {

// Opt-in to more than 64 KB of dynamic LDS for a kernel, checked and per device: `st` is the call site's table of the sizes
// already granted on each device ordinal (one process may drive several GPUs).  A failing hipFuncSetAttribute is not silent: it is
// recorded with note_launch_error() and the C ABI entry point that issued the launch returns it (engine_state.h, LAUNCHCHK).
struct LdsAttr {
    size_t granted[32] = {};
};
void ensure_dynamic_lds(const void* fn, size_t bytes, LdsAttr& st);
void note_launch_error(const char* what, hipError_t e);

#ifdef __HIPCC__
// Sum over the 64 lanes of a wave, result in every lane.  DPP row shifts / row broadcasts (a scan whose last lane holds the
// total) + one readlane: ~10 VALU instructions.  __shfl_xor lowers to ds_bpermute_b32, i.e. six dependent LDS round trips
// (~600 cycles) per sum -- measurable in the LayerNorm prologues of the latency-bound streaming kernels.
// (sequence, frame) of row `row0 + lr` of a [b][T] row space, from (b0, t0) = divmod(row0, T) computed once per block: a carry
// loop instead of an integer division per row (a division by a run-time divisor is ~40 instructions; the row-local stages did
// 16-32 of them per lane)
struct SeqRow {
    int b, t;
};
__device__ __forceinline__ SeqRow seq_row(int b0, int t0, int T, int lr) {
    SeqRow r{b0, t0 + lr};
    while (r.t >= T) {
        r.t -= T;
        ++r.b;
    }
    return r;
}

__device__ __forceinline__ float wave_sum_dpp(float v) {
#define MASR_DPP_F(x, ctrl, rows) \
    __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (x)), (ctrl), (rows), 0xf, false))
    v += MASR_DPP_F(v, 0x111, 0xf);   // row_shr:1
    v += MASR_DPP_F(v, 0x112, 0xf);   // row_shr:2
    v += MASR_DPP_F(v, 0x114, 0xf);   // row_shr:4
    v += MASR_DPP_F(v, 0x118, 0xf);   // row_shr:8
    v += MASR_DPP_F(v, 0x142, 0xa);   // row_bcast:15 -> rows 1, 3
    v += MASR_DPP_F(v, 0x143, 0xc);   // row_bcast:31 -> rows 2, 3
#undef MASR_DPP_F
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// The activations behind ACT_SILU (GemmAct), on the device math library's erff / tanhf / expf (1-2 ulp), never the fast
// intrinsics.  ACT as a template argument: the row kernels of wide.hip; act_f(act, v): the GEMM epilogues, where act is uniform
// over the launch and the switch is a scalar branch.  ACT_SILU is the expression of silu_f (gemm_f32.hip) and of the wide
// depthwise kernels, so that a swish launch keeps its bits.
template <int ACT>
__device__ __forceinline__ float act_f(float v) {
    static_assert(ACT >= 0 && ACT <= 6, "GemmAct");
    if (ACT == 1) return fmaxf(v, 0.f);
    if (ACT == 2) return v / (1.0f + expf(-v));
    if (ACT == 3) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
    if (ACT == 4) return tanhf(v);
    if (ACT == 5) return fminf(fmaxf(v, -1.0f), 1.0f);
    if (ACT == 6) return v > 0.f ? 1.0507009873554805f * v : 1.7580993408473766f * (expf(v) - 1.0f);   // scale * alpha
    return v;
}
__device__ __forceinline__ float act_f(int act, float v) {
    switch (act) {
    case 1: return act_f<1>(v);
    case 2: return act_f<2>(v);
    case 3: return act_f<3>(v);
    case 4: return act_f<4>(v);
    case 5: return act_f<5>(v);
    case 6: return act_f<6>(v);
    default: return v;
    }
}
#endif


// ---- subsampling front-end geometry (encoder_conf.input_layer, masr_config.reserved[3]) ----------------------------
// 0 = conv2d (Conv2dSubsampling4), 1 = conv2d6, 2 = conv2d8 (reference conformer/subsampling.py:65-211).  Every conv has no
// padding: conv1 is 3x3 stride 2, then 3x3 stride 2 (conv2d), 5x5 stride 3 (conv2d6) or 3x3 stride 2 twice (conv2d8).  The
// subsampled mask keeps input frame rate * t (x_mask[:-2:2][:-2:2], [:-2:2][:-4:3], [:-2:2] x 3), so encoder frame t of an
// utterance of len feature frames is valid iff rate * t < len.
enum InputLayer { IL_CONV2D = 0, IL_CONV2D6 = 1, IL_CONV2D8 = 2 };
__host__ __device__ inline int sub_rate(int il) { return il == IL_CONV2D6 ? 6 : il == IL_CONV2D8 ? 8 : 4; }
__host__ __device__ inline int sub_min_frames(int il) { return il == IL_CONV2D6 ? 11 : il == IL_CONV2D8 ? 15 : 7; }
// size of one spatial axis (time or frequency) behind the convs after the first: n1 = (n - 1) / 2 comes out of conv1
__host__ __device__ inline int sub_after_conv1(int il, int n1) {
    return il == IL_CONV2D6 ? (n1 - 2) / 3 : il == IL_CONV2D8 ? ((n1 - 1) / 2 - 1) / 2 : (n1 - 1) / 2;
}
// encoder frames T' for T feature frames (0 below the minimum)
__host__ __device__ inline int sub_frames(int il, int T) { return T < sub_min_frames(il) ? 0 : sub_after_conv1(il, (T - 1) / 2); }
// frequency bins behind the last conv (80 mel bins: 19 / 12 / 9)
__host__ __device__ inline int sub_bins(int il, int F) { return sub_after_conv1(il, (F - 1) / 2); }

// ---- GEMM: C[M,N] = epilogue(A[M,K] * W[N,K]^T) on v_mfma_f32_32x32x2_f32 ----------------
enum GemmAct { ACT_NONE = 0, ACT_RELU = 1, ACT_SILU = 2, ACT_GELU = 3, ACT_TANH = 4, ACT_HARDTANH = 5, ACT_SELU = 6 };
inline bool gemm_act_valid(int act) { return act >= ACT_NONE && act <= ACT_SELU; }
// encoder_conf.activation_type of the Conformer (masr_config.reserved[4]; model_utils/utils/common.py get_activation): the hidden
// activation of both feed-forward modules and the one behind the conv module's norm.  Torch's defaults: erf-exact GELU, Hardtanh
// on [-1, 1], SELU with scale 1.0507009873554805 and alpha 1.6732632423543772.
enum EncAct { ENC_ACT_SWISH = 0, ENC_ACT_RELU = 1, ENC_ACT_GELU = 2, ENC_ACT_TANH = 3, ENC_ACT_HARDTANH = 4, ENC_ACT_SELU = 5 };
// the GemmAct of an EncAct (ACT_NONE for a value outside the enum: masr_create refuses those)
inline int gemm_act_of(int enc_act) {
    constexpr int t[6] = {ACT_SILU, ACT_RELU, ACT_GELU, ACT_TANH, ACT_HARDTANH, ACT_SELU};
    return enc_act >= 0 && enc_act < 6 ? t[enc_act] : ACT_NONE;
}
enum GemmAMode { A_PLAIN = 0, A_CONV2 = 1, A_CONV5 = 2, A_ROWS = 3 };     // A_CONV5: the 5x5 stride-3 gather of conv2d6 (A_CONV2 geometry);
                                                                          // A_ROWS: row m of A is row GemmArgs::rows[m] of a row pool
enum GemmEpi { EPI_STD = 0, EPI_GLU = 1, EPI_SPLITK = 2, EPI_ACT = 3 };   // EPI_ACT: EPI_STD + GemmAct 3 .. 6 (launch_gemm picks it by a.act);
                                                                // EPI_GLU is NOT implemented by launch_gemm (gemm_f32.hip has no GLU
                                                                // epilogue; the number is kept so that EPI_SPLITK keeps its value): the
                                                                // row-block kernels carry RG_EPI_GLU, the wide path runs launch_glu_wide

struct GemmArgs {
    const float* A;      // [M, lda] row-major (A_PLAIN), conv activations [B,T1,F1,C] (A_CONV2 / A_CONV5) or a row pool [n_rows, lda] (A_ROWS)
    const float* W;      // [N, K] row-major (K contiguous) -- torch Linear.weight layout
    const float* bias;   // [N] or nullptr
    float* C;            // [M, ldc]
    const float* R;      // residual [M, ldr] or nullptr (may alias C)
    const int* lens;     // optional per-sequence feature lengths for row masking (see mask_tp)
    int M, N, K;
    int lda, ldc, ldr;
    int act;             // GemmAct (EPI_STD only; launch_gemm_bf16x3 takes none / relu / silu and leaves the rest to launch_gemm)
    float alpha;         // out = R + alpha * act(acc + bias)
    int mask_tp;         // >0: row r -> (b = r / mask_tp, t = r % mask_tp); rows with 4*t >= lens[b] give act(..)=0
    int bias_after_alpha; // 1: out = R + alpha*act(acc) + bias  (Squeezeformer input_proj: scaling precedes the Linear)
    // A_CONV2 / A_CONV5 geometry: row m -> (b, t2, f2) with m = (b*T2 + t2)*F2 + f2 ; k -> (c / 32, kh, kw, c % 32)
    int T1, F1, T2, F2, Cc;
    int nsplit, ksplit;  // EPI_SPLITK: number of K ranges (gridDim.y) and BK-slabs per range
    // skip_rps > 0 (with lens): row r belongs to sequence r / skip_rps at frame (r % skip_rps) / skip_div; a tile whose rows all lie in
    // ONE sequence at frames with 4 * frame >= lens[sequence] (padding) is not computed -- its output rows keep what they held
    int skip_rps, skip_div;
    // A_CONV2, N = 256: launch_pack_conv2_rows copy of W -- launch_gemm then runs the full-width row-block kernel where it would run
    // 128x128 tiles (nullptr: never)
    const float* Wp;
    // conv2_rows_kernel only, with Wp: conv1 computed inside the A gather (masr_debug_set key 41) from the features
    // feats [B, Tin, Fin] through CMVN (mean, istd) and the conv1 weights c1w [9][256], c1b [256]; A is not read (nullptr: from A)
    const float *feats, *mean, *istd, *c1w, *c1b;
    int Tin, Fin;
    // A_ROWS: row m of the A operand is A + rows[m] * lda (64-bit: the pool may exceed 2^31 bytes), rows [M] int64 on the device.  An
    // entry outside [0, n_rows) -- the -1 padding of a row table -- is a row of zeros and is never dereferenced.  EPI_STD only; the
    // tile shapes are A_PLAIN's at the same (M, N), and every output element sees A_PLAIN's MFMA chain on the gathered dense copy
    const int64_t* rows;
    int64_t n_rows;
};

void launch_gemm(const GemmArgs& a, int amode, int epi, hipStream_t s);
void launch_pack_conv2_rows(const float* w, float* p, int K, hipStream_t s);    // W [256, K] -> GemmArgs::Wp layout
bool gemm_conv2_rows(const GemmArgs& a);    // launch_gemm(a, A_CONV2, EPI_STD) runs conv2_rows_kernel (needs a.Wp)
// deep-K, few-row GEMM: split K over workgroups into `partial` [nsplit][M][N], then reduce + epilogue into a.C
void launch_gemm_splitk(const GemmArgs& a, float* partial, int nsplit, hipStream_t s, int amode = A_PLAIN);
struct FfnArgs;
// exploratory split-bf16 variant (gemm_bf16x3.hip; masr_debug_set key 20): standard epilogue only; false = not taken
#if MASR_EXPERIMENTS
bool launch_gemm_bf16x3(const GemmArgs& a, int amode, hipStream_t s);
// fused split-bf16 FFN (ffn_x3.hip): weights packed once per FFN (hi / lo pieces in fragment order)
size_t ffn_x3_packed_elems(int dff);
void launch_pack_ffn_x3(const float* w1, const float* w2, unsigned short* p1, unsigned short* p2, int dff, hipStream_t s);
bool launch_ffn_x3(const FfnArgs& a, hipStream_t s);      // w1 / w2: the packed (hi, lo) bf16 copies; false = sizes not covered
#else
inline bool launch_gemm_bf16x3(const GemmArgs&, int, hipStream_t) { return false; }
inline size_t ffn_x3_packed_elems(int) { return 0; }
inline void launch_pack_ffn_x3(const float*, const float*, unsigned short*, unsigned short*, int, hipStream_t) {}
inline bool launch_ffn_x3(const FfnArgs&, hipStream_t) { return false; }
#endif

// ---- elementwise / reductions ------------------------------------------------------------
// LayerNorm over rows of width 256.  If seq_t > 0 the output row is remapped to
// b*(seq_t+pad)+pad+t (conv-module padded layout) and rows with 4*t >= lens[b] are zeroed.
void launch_layernorm(const float* x, const float* w, const float* b, float* y, int M, float eps,
                      int seq_t, int pad, const int* lens, hipStream_t s);
// CMVN + Conv2d(1->C,3x3,s2) + ReLU, output channels-last [B,T1,F1,C]
void launch_conv1(const float* feats, const float* mean, const float* istd, const float* w9c, const float* bias,
                  float* out, int B, int T, int F, int C, hipStream_t s);
// depthwise causal conv (k taps) + LayerNorm(C=256) + SiLU on padded layout [nseq, pad+Tq, 256] -> [nseq*Tq, 256]
// k = 15 / 7 / 31: the kernels instantiated on the tap count; every other k in [1, 32]: dwconv_ln_silu_taps_kernel (tap count at
// run time).  false: no kernel for k taps, nothing was launched -- the caller reports it
bool launch_dwconv_ln_silu(const float* g, const float* wkc, const float* bias, const float* lnw, const float* lnb,
                           float* out, int nseq, int Tq, int ktaps, float eps, hipStream_t s, const float* gconst = nullptr);
// same with an eval-mode BatchNorm folded into a per-channel scale/shift instead of the LayerNorm
void launch_glu_const(const float* bias512, float* out256, hipStream_t s);
void launch_queue_spin(long long ticks, hipStream_t s);      // holds the stream's hardware queue for `ticks` x 10 ns
void launch_queue_nop(hipStream_t s);
bool launch_dwconv_bn_silu(const float* g, const float* wkc, const float* bias, const float* scale, const float* shift,
                           float* out, int nseq, int Tq, int ktaps, hipStream_t s, const float* gconst = nullptr);
// Efficient-Conformer stride layer: depthwise causal conv with stride 2 (+ LayerNorm + SiLU) on the padded layout
// [nseq][ktaps-1 + Tin][256] -> [nseq * ceil(Tin/2), 256]; and the AvgPool1d(2, ceil_mode) residual path
void launch_dwconv_stride2_ln_silu(const float* g, const float* wkc, const float* bias, const float* lnw,
                                   const float* lnb, float* out, int nseq, int Tin, int ktaps, float eps, hipStream_t s);
// same with an eval-mode BatchNorm folded into a per-channel scale/shift instead of the LayerNorm (cnn_module_norm: batch_norm)
void launch_dwconv_stride2_bn_silu(const float* g, const float* wkc, const float* bias, const float* scale,
                                   const float* shift, float* out, int nseq, int Tin, int ktaps, hipStream_t s);
void launch_avgpool2(const float* x, float* out, int B, int T, hipStream_t s);
// Squeezeformer TimeReductionLayer1D depthwise part: k=5, stride 2, padding 3, pad-masked input -> [B, ceil(T/2), 256]
void launch_time_reduce_dw(const float* x, const float* w5c, const float* bias, const int* lens, float* out, int B, int T,
                           int mstride, hipStream_t s);
// Squeezeformer recover: x[b,t,:] = saved[b,t,:] + y[b, t/2, :]
void launch_recover_add(const float* saved, const float* y, float* x, int B, int T, int L, hipStream_t s);
// softmax over V per row (in place) + argmax / max prob
void launch_softmax_argmax(float* logits, int M, int V, int ldv, int write_probs, int* idx, float* maxp, hipStream_t s);
// CTC collapse per utterance.  The kernel stages the non-blank max-probs of an utterance in Tp * 4 bytes of dynamic LDS and
// nothing raises its limit above the default 64 KB (ensure_dynamic_lds): every caller refuses Tp > CTC_COLLAPSE_MAX_FRAMES by
// name (ctc_collapse_refusal) before it launches
constexpr int CTC_COLLAPSE_MAX_FRAMES = 16384;
constexpr char ctc_collapse_refusal[] = "more than 16384 frames per utterance are not supported by the CTC collapse kernel (it stages Tp max-probs in 64 KB of dynamic LDS)";
void launch_ctc_collapse(const int* idx, const float* maxp, const int* nframes, int B, int Tp, int blank,
                         int* tokens, int* ntok, float* score, hipStream_t s);
struct PoolSeg {            // masr_pool_step: one contiguous run of rows to copy (rows of `width` floats)
    long src, dst;
    int n, pad_;
};
void launch_ctc_collapse_hist(const int* idx, const float* maxp, const int* nframes, const int* in_rows, int ld_in, int B, int Tp,
                              int blank, int* rows, hipStream_t s);
void launch_copy_segments(const float* src, float* dst, const float* src2, float* dst2, const PoolSeg* seg, int nseg,
                          int max_rows, int width, hipStream_t s);
void launch_ctc_collapse_rows(const int* idx, const float* maxp, const int* nframes, int B, int Tp, int blank, int* rows,
                              hipStream_t s);
void launch_topk_prune(const float* probs, int M, int V, int top_n, float cutoff_prob, int* out_idx, float* out_logp,
                       int* out_cnt, int blank, float* out_blank_lp, hipStream_t s);
void launch_argmax_rows(const float* probs, int M, int V, int* idx, float* maxp, hipStream_t s);
void launch_frame_counts(const int* nsamp, int B, int* nfr, int* nenc, int halve, hipStream_t s, int input_layer = IL_CONV2D);
// lens [B] feature frames -> out [B] = 4 * ceil(lens / rate): the conv2d-unit lengths of a rate-6 / rate-8 front-end
void launch_sub_lens(const int* lens, int B, int rate, int* out, hipStream_t s);
void launch_export_att(const float* cache, float* out, int L, int H, int cap, int t, int dk, hipStream_t s, int rate = 1,
                       int shift = 0);   // rate 2: half-rate cache, entry (j + shift) / 2 (the reference repeat-interleaves)
struct PlaneCopy { const float* src_k; const float* src_v; float* dst_k; float* dst_v; };
void launch_kv_append_planar(const PlaneCopy* pc, int n, int Tq, hipStream_t s);
void launch_export_cnn_layer(const float* cache, float* out, int used, int total, int d, hipStream_t s);
void launch_export_att_planar(const float* kplane, const float* vplane, float* out, int H, int t, int dk, hipStream_t s);
void launch_affine_rows(const float* x, const float* w, const float* b, float* y, int M, int seq_t, int pad, hipStream_t s);
void launch_export_cnn(const float* cache, float* out, int L, int pad, int d, hipStream_t s);

// ---- row-block GEMM for the K = 256 projections (rowgemm.hip) -------------------------------------
struct AttSeq;
enum RowGemmPro { RG_PRO_PLAIN = 0, RG_PRO_LN = 1, RG_PRO_LN_PAD = 2, RG_PRO_AFFINE = 3,
                  RG_PRO_HIST = 4, RG_PRO_DWCONV = 5 };      // small-M kernel only (rowgemm_small.hip): fused streaming conv-module fronts
enum RowGemmEpi { RG_EPI_STORE = 0, RG_EPI_RESID = 1, RG_EPI_GLU = 2, RG_EPI_CTC = 3, RG_EPI_CHAIN = 4 };
struct RowGemmArgs {
    const float* A;       // [rows, lda] source rows (K = 256)
    const float* lnw;     // LayerNorm weight / bias (PRO_LN*)
    const float* lnb;
    const float* W;       // [N, 256]
    const float* Wp;      // optional: the same weights in fragment order (launch_pack_rows_pc, N rounded up to 256); the offline CHAIN /
                          // CTC launches then read them with buffer loads straight into MFMA operand registers (no LDS slab staging)
    const float* bias;    // [N]
    float* C;             // output [M, ldc]
    const float* R;       // residual [M, ldr] (EPI_RESID; may alias C)
    float* R2;            // EPI_CHAIN: where the updated residual stream x + out-proj goes (may alias R); C = GLU output
    const int* lens;      // per-sequence feature lengths (pad masks), or nullptr
    int* out_idx;         // EPI_CTC: per-row argmax
    float* out_maxp;      // EPI_CTC: per-row softmax probability of the argmax
    int M, N;             // output rows / weight rows
    int lda, ldc, ldr;
    float eps, alpha;
    int seq_t, pad;       // PRO_LN_PAD: output rows index [nseq][pad + seq_t], source rows [nseq][seq_t]
    int mask_tp;          // EPI_RESID: >0 -> row r = (b, t) with t = r % mask_tp masked when mstride*t >= lens[b]
    int mstride;          // feature frames per encoder frame for the pad masks (4; 8 after Squeezeformer time reduction)
    int out_seq_t;        // >0: output row (b, t) is stored at b*(out_seq_t + out_pad_tot) + out_pad_l + t
    int out_pad_l, out_pad_tot;
    int plane_cols;       // EPI_STORE: >0 -> column c goes to plane c / plane_cols (planar q | k | v buffers)
    long plane_stride;    //            floats between planes
    int a_seq_t, a_seq_stride;   // PRO_PLAIN: >0 -> source row of (b, t) = b * a_seq_stride + t, with (b, t) = divmod(row, a_seq_t)
    float* const* cache_rd;      // PRO_HIST: per-stream cnn cache (read half / written half of the double buffer); A = x rows,
    float* const* cache_wr;      //           seq_t new rows + pad history rows per stream, M = n * (seq_t + pad)
    int hist_affine;             //           1: new rows = lnw * x + lnb (Squeezeformer, convolution.py:109-110) instead of LayerNorm
    const float* dw_w;           // PRO_DWCONV: depthwise weights [pad + 1][256] and bias [256]; A = GLU rows in the padded layout
    const float* dw_b;           //             [n][pad + seq_t][256], lnw / lnb = the conv module's LayerNorm, M = n * seq_t
    const float* gconst;         //             offline causal conv: the pad history rows of every sequence are not materialised -- they
                                 //             all hold this constant row glu(bias) [256] (nullptr: read them like any other row)
    const AttSeq* kv_seqs;       // EPI_STORE, small-M kernel: columns >= 256 (k | v of the fused QKV projection) of row (b, t) =
    int kv_tq;                   //   divmod(row, kv_tq) go to stream b's key/value cache instead of C (replaces launch_kv_append)
};
bool launch_rowgemm(const RowGemmArgs& a, int pro, int epi, hipStream_t s);   // false: not applicable, nothing launched (HIST / DWCONV)
bool launch_rowgemm_small(const RowGemmArgs& a, int pro, int epi, hipStream_t s);   // rowgemm_small.hip; false = not applicable

// Fused FFN block, in place: x <- x + scale * (W2 . silu(W1 . LN(x) + b1) + b2)   (ffn_pc.hip and its kin; FfnArgs below)
// post: LayerNorm that follows the block in the layer; it is fused into the split-mode reduction of small M
struct FfnPostLn {
    const float* lnw;
    const float* lnb;
    float* y;          // destination rows (may alias x); nullptr: no LayerNorm behind the block
    float eps = 1e-5f;
};
// tail: a row-local stage appended to the full (non-split) kernel: out[M, N] = LayerNorm(x_new; lnw, lnb) . W[N, 256]^T + bias
// (the fused QKV projection that follows the first macaron FFN).  Return value 2 = done by the kernel.
struct FfnTail {
    const float* lnw;
    const float* lnb;
    const float* W;
    const float* bias;
    float* out;
    int N, ldo;
    const float* pre_lnw;      // optional: x <- LayerNorm(x; pre_lnw, pre_lnb) first, written back (the previous layer's norm_final,
    const float* pre_lnb;      // encoder.py:160-161, riding on this launch instead of its own)
    // planar output (the Efficient Conformer's grouped attention: q | k | v planes [nseq][seq_t + pad_t][256], the time padding
    // rows stay zero): plane_stride > 0 -> column tile c / 256 goes to plane c / 256, row (b, t) = divmod(row, seq_t) to row
    // b * (seq_t + pad_t) + t of that plane (ffn_pc.hip only)
    long plane_stride;
    int seq_t, pad_t;
};
// head: the rest of the conv module in front of the block, on the workgroup's own 32 rows, before the block's LayerNorm:
//   x <- x + mask(pointwise_conv2(SiLU(LayerNorm(depthwise_conv(glu)))))       (convolution.py:120-131, encoder.py:137-148)
// norm = 1 (cnn_module_norm: batch_norm): the eval-mode BatchNorm1d folded into a per-channel scale / shift instead of the LayerNorm
// the depthwise conv reads the GLU rows of the padded layout [nseq][pad + seq_t][256] (ktaps - 1 = pad history rows in front,
// gconst: constant history rows that are not materialised).  Return value bit 2 (4) = done by the kernel.
struct FfnHead {
    const float* glu;          // nullptr: no head stage
    const float* dw_w;         // [ktaps][256]
    const float* dw_b;
    const float* lnw;          // the conv module's LayerNorm (norm = 1: the folded BatchNorm's scale / shift)
    const float* lnb;
    const float* gconst;       // [256] or nullptr
    const float* W;            // pointwise_conv2 [256, 256]
    const float* bias;
    const int* lens;           // feature lengths for the pad mask, or nullptr
    int seq_t, ktaps, mstride;
    float* xout;               // d_ff-split launches (few rows) only: where the rows updated by the head stage go -- every d_ff
                               // slice of a row block runs the head on the SAME old rows of x, so x itself must stay untouched
                               // until the split reduction, which then reads xout and writes x
    int norm;                  // 0 = LayerNorm, 1 = folded BatchNorm: y = silu(conv * lnw[c] + lnb[c]), no row statistics
};
// One FFN call, from ffn()'s call sites (the engine's family files; ffn() itself: engine_layers.hip) to the launchers.  ffn_plan.h chooses the launcher; ffn() hands it the weights
// in that kernel's order (w1 / w2, tail.W, head.W) and only the stages the kernel is to run
struct FfnArgs {
    float* x = nullptr;           // rows [M, 256], updated in place (ffn(): the engine's residual stream)
    int M = 0, dff = 0;           // rows / hidden units (ffn(): the model's d_ff)
    const float* lnw = nullptr;   // the block's LayerNorm (affine = 1: per-channel scale / bias instead, Squeezeformer)
    const float* lnb = nullptr;
    const float* w1 = nullptr;    // [dff, 256]
    const float* b1 = nullptr;
    const float* w2 = nullptr;    // [256, dff]
    const float* b2 = nullptr;
    float scale = 0.5f;           // x <- x + scale * block(x)
    int affine = 0;
    float eps = 1e-5f;
    FfnPostLn post{};             // the LayerNorm that follows the block; y == nullptr: none
    FfnTail tail{};               // W == nullptr: none
    FfnHead head{};               // glu == nullptr: none
    float* partial = nullptr;     // split mode: [nsplit][M][256] partial sums
    int nsplit = 1;               //             d_ff slices wished for (1: the full kernel)
    bool packed = false;          // w1 / w2 are launch_pack_ffn_pc's copies (launch_ffn_fused)
};
// the fused block (ffn_pc.hip through ffn_reduce.hip): returns 1 when the post LayerNorm was applied (split-d_ff path), 2 when the
// tail stage ran, 4 when the head stage ran (| 1 on a split launch), 0 when the caller still has to run whichever it asked for
int launch_ffn_fused(const FfnArgs& a, hipStream_t s);
void launch_pack_ffn_pc(const float* w1, const float* w2, float* p1, float* p2, int dff, hipStream_t s);
void launch_pack_rows_pc(const float* w, float* p, int N, hipStream_t s, int n_src = -1);   // weights [n_src, 256] -> N % 256 == 0 packed rows (rows >= n_src zero)
// 16-row fused FFN stages (ffn_pc.hip ffn16_kernel, two workgroups per CU): full-d_ff launches only, packed weights of its own order
int launch_ffn16(const FfnArgs& a, hipStream_t s);
void launch_pack_ffn16(const float* w1, const float* w2, float* p1, float* p2, int dff, hipStream_t s);
void launch_pack_rows16(const float* w, float* p, int N, hipStream_t s, int n_src = -1);
// sqz_layer.hip: one Squeezeformer (post-LN) half-layer per launch on the workgroup's own 32 rows --
//   stage 0 "mid": x <- LN_a(x + att . head_w^T + head_b);  x <- LN_b(x + FFN(ffn_s * x + ffn_b));
//                  glu_out <- GLU(pw1(mask(tail_s * x + tail_sb)))        (tail_n = 512, padded layout of the depthwise conv)
//   stage 1 "end": x <- LN_a(x + mask(pw2(SiLU(BN(dwconv(glu))))));  out <- LN_b(x + FFN(ffn_s * x + ffn_b));
//                  tail_out <- Wqkv . (tail_s * out + tail_sb) + bqkv     (tail_n = 768; tail_w == nullptr: no tail)
// head_w / tail_w: packed rows (launch_pack_rows_pc), w1 / w2: packed FFN weights (launch_pack_ffn_pc)
struct SqzStageArgs {
    float* x;                  // residual stream [M, 256], updated in place
    float* out;                // where the stage's last LayerNorm goes (x, or the encoder output for the last layer)
    const float* att;          // stage 0: attention output rows [M, 256]
    const float* head_w;       // stage 0: Wo; stage 1: pointwise_conv2
    const float* head_b;
    const float *ln_a_w, *ln_a_b, *ln_b_w, *ln_b_b;
    const float *ffn_s, *ffn_b, *w1, *b1, *w2, *b2;
    const float *tail_w, *tail_b, *tail_s, *tail_sb;
    float* tail_out;           // stage 1: qkv [M, 768]
    float* glu_out;            // stage 0: [nseq][glu_pad_tot + seq_t][256], real rows at glu_pad_l
    const float* glu;          // stage 1: the same buffer
    const float *dw_w, *dw_b, *bn_scale, *bn_shift, *gconst;
    const float* gpad;         // stage 1 with skip_pad, symmetric conv: glu(pointwise_conv1 bias) [256], the GLU row of a padded frame
    const int* lens;           // feature lengths for the pad mask, or nullptr
    int M, dff, seq_t, mstride, ktaps, tail_n, glu_pad_l, glu_pad_tot;
    float eps;
    int skip_pad;              // 1 (with lens): a row block of padded frames only is not computed (x, glu, qkv rows keep what they held)
};
bool launch_sqz_stage(const SqzStageArgs& a, int stage, hipStream_t s);
// ffn_dual.hip: the same block with two independent accumulator chains per wave (chunks of 256 hidden units); p1 / p2 from
// launch_pack_ffn_dual, tail->W from launch_pack_rows_dual (N = 768), head->W from launch_pack_rows_pc.
// Returns 0 / 2 (tail done) / 4 (head done), -1 when the sizes are not covered
#if MASR_EXPERIMENTS
int launch_ffn_dual(const FfnArgs& a, hipStream_t s);
void launch_pack_ffn_dual(const float* w1, const float* w2, float* p1, float* p2, int dff, hipStream_t s);
void launch_pack_rows_dual(const float* w, float* p, hipStream_t s);
#else
inline int launch_ffn_dual(const FfnArgs&, hipStream_t) { return -1; }
inline void launch_pack_ffn_dual(const float*, const float*, float*, float*, int, hipStream_t) {}
inline void launch_pack_rows_dual(const float*, float*, hipStream_t) {}
#endif

// one-chunk FFN slices for few rows (ffn_coop.hip): all eight waves on both products; w1p = launch_pack_ffn_coop_w1's copy, w2p =
// ffn_pc.hip's packed W2, partial [dff / 128][M][256]
#if MASR_EXPERIMENTS
void launch_pack_ffn_coop_w1(const float* w1, float* p, int dff, hipStream_t s);
void launch_ffn_coop(const FfnArgs& a, hipStream_t s);      // the caller runs the reduction
#else
inline void launch_pack_ffn_coop_w1(const float*, float*, int, hipStream_t) {}
inline void launch_ffn_coop(const FfnArgs&, hipStream_t) {}
#endif
// x <- xin + scale * (sum of a.nsplit partial sums + b2), then a.post (xin: the rows a head stage of the split launch updated;
// nullptr: x)
void launch_ffn_reduce(const FfnArgs& a, hipStream_t s, const float* xin = nullptr);

// Fragment-ordered weight copies, one layout per packing routine: the engine keeps every copy it has built under
// (layout, device pointer of the source weights) -- engine_encoder.h packed_of()
enum PackLayout {
    PACK_FFN_PC,        // launch_pack_ffn_pc: W1 | W2 of an FFN, keyed by W1
    PACK_ROWS_PC,       // launch_pack_rows_pc: [N, 256] rows, N rounded up to a multiple of 256
    PACK_FFN16,         // launch_pack_ffn16: W1 | W2 in the 16-row kernel's order, keyed by W1
    PACK_ROWS16,        // launch_pack_rows16
    PACK_CONV2_ROWS,    // launch_pack_conv2_rows: subsampling conv / embed projection weights [256, K]
    PACK_FFN_DUAL,      // launch_pack_ffn_dual: W1 | W2 in the two-chain order, keyed by W1
    PACK_ROWS_DUAL,     // launch_pack_rows_dual: the 768-row QKV tail of the two-chain kernel
    PACK_FFN_COOP_W1,   // launch_pack_ffn_coop_w1: W1 as 16 x 16 x 4 fragments (W2: the PACK_FFN_PC copy)
    PACK_FFN_X3,        // launch_pack_ffn_x3: (hi, lo) bf16 pieces of W1 | W2, keyed by W1
};

// ---- CTC prefix beam search on the GPU (beam_gpu.hip) ---------------------------------------------
struct BeamGpuArgs {
    const int* cidx;       // [B * T_stride, K]
    const float* clp;      // [B * T_stride, K]
    const int* ccount;     // [B * T_stride]
    const float* blank_lp; // [B * T_stride] ln p(blank) of every frame: input of the decoder's min_cutoff rule (nullptr: rule off)
    const int* frames;     // [B] frames to consume per utterance (nullptr: T_stride)
    int T_stride, K, beam, blank, max_len;
    int* pool_parent;      // [B][pool_cap]
    int* pool_ch;          // [B][pool_cap]
    int pool_cap;
    int* state_i;          // [B][2 + 3 * beam]: n_live, pool_count, node[], ch[], lm m|oov[]     (persistent streams)
    unsigned long long* state_h;   // [B][3 * beam]: string identity of the prefix and of its parent, packed LM context
    float* state_f;        // [B][7 * beam]:     b[], nb[], score[], LM backoffs [4][]
    int init;              // 1: start from the empty prefix; 0: continue from state_*
    int* tokens;           // [B][max_len]
    int* len;              // [B]
    float* score;          // [B]
    long long* prof;       // optional [8] cycle counters of workgroup 0 (phase breakdown), or nullptr
    // external scorer (lm_scorer.h): a new prefix p + c adds alpha * ln P_LM(c | last words of p) + beta to its score
    int use_lm;
    LmView lm;             // table / known in the memory of the launch device
    float alpha, beta;
    int lm_cache;          // 1: one scorer probe per (distinct effective context, candidate) and frame; 0: one per (prefix, candidate)
    int narrow;            // 1: frames of <= 1024 extension entries run on the narrow step (beam_gpu.hip); 0: every frame on the wide step
};
// per-utterance search state in HBM: [3 * beam] u64 | [2 + 3 * beam] int | [7 * beam] float
inline size_t beam_state_bytes(int beam) { return (size_t)3 * beam * 8 + (size_t)(2 + 3 * beam) * 4 + (size_t)7 * beam * 4 + 8; }
inline void beam_state_carve(void* base, int B, int beam, unsigned long long** h, int** i, float** f) {
    *h = reinterpret_cast<unsigned long long*>(base);                       // [B][3 * beam]
    *i = reinterpret_cast<int*>(*h + (size_t)B * 3 * beam);                 // [B][2 + 3 * beam]
    *f = reinterpret_cast<float*>(*i + (size_t)B * (2 + 3 * (size_t)beam)); // [B][7 * beam]
}
size_t beam_gpu_lds_bytes(int beam, int K, bool use_lm);
int launch_beam_search(const BeamGpuArgs& a, int B, hipStream_t s);   // 1: sizes not supported

// ---- the N best prefixes of a finished search (beam_nbest.hip): reads the live set launch_beam_search persisted ----
struct BeamNbestArgs {
    const int* state_i;        // [B][2 + 3 * beam] of the search (n_live, -, node[], ch[], -)
    const float* state_f;      // [B][7 * beam]     of the search (score[] at 2 * beam)
    const int* pool_parent;    // [B][pool_cap]
    const int* pool_ch;        // [B][pool_cap]
    int pool_cap, beam, nbest, max_len;
    int* tokens;               // [B][nbest][max_len]
    int* len;                  // [B][nbest]
    float* score;              // [B][nbest]
    int* count;                // [B] = min(nbest, n_live)
    int use_lm;                // 1: the reported scores are the decoder's approx_ctc (the ranking stays on the search score)
    LmView lm;
    float alpha, beta;
};
int launch_beam_nbest(const BeamNbestArgs& a, int B, hipStream_t s);  // 1: sizes not supported

// ---- DeepSpeech2 (lstm.hip, gru.hip) ------------------------------------------------------
// step launchers: H = every multiple of 256 in [256, 2048]; 1 (and nothing launched) for any other H
int launch_lstm_step(const float* gx, const float* whh, const float* h_prev, float* h_next, float* c, float* out,
                     const int* lens, int B, int T, int H, int step, int ndir, hipStream_t s);
void launch_layernorm_generic(const float* x, const float* w, const float* b, float* y, int M, int N, float eps,
                              hipStream_t s);
void launch_ds2_lens(const int* lens, int B, int Tq, int* out, hipStream_t s);
// use_gru: True (gru.hip): gx [B*T][ndir*3H] holds W_ih x + b_ih + [b_hr, b_hz, 0]; bhn [ndir][H]
int launch_gru_step(const float* gx, const float* whh, const float* bhn, const float* h_prev, float* h_next, float* out,
                    const int* lens, int B, int T, int H, int step, int ndir, hipStream_t s);

// ---- attention ---------------------------------------------------------------------------
struct AttSeq {            // one per sequence, device memory
    const float* q;        // first query row of this sequence (row stride q_stride)
    const float* k;        // first key row   (row stride kv_stride)
    const float* v;        // first value row (row stride kv_stride)
    float* out;            // first output row (row stride heads * 64: launch_attention's row_w)
    int nq, nk;            // number of query rows / key rows
    int klen;              // keys j >= klen are masked (padding)
    int pos0;              // positional index of key 0
    int q_abs0;            // absolute index of query 0 (for the chunk mask)
    int pad_;
};
// attention + [out-projection + residual -> LayerNorm -> pointwise_conv1 -> GLU] of an offline Conformer layer as ONE launch
// (attention.hip attn_chain_kernel; d_model 256, 4 heads of 64): the arguments of launch_attention + those of the EPI_CHAIN rowgemm
struct AttnChainArgs {
    const AttSeq* seqs;        // [nseq]; q / k / v rows of sequence b, nq = nk = frames of the padded batch
    int nseq, nqb;             // nqb (query blocks of 32 per sequence) is filled in by the launcher
    int q_stride, kv_stride, chunk_size, pos_stride;
    const float* ptab;         // [max_pos, 256] positional keys of the layer
    const float* bias_u;       // [4][64]
    const float* bias_v;
    const float* Wp;           // [Wo; W_pw1] packed in fragment order (launch_pack_rows_pc, 768 rows)
    const float* bias;         // [768]  bo | b_pw1 (value | gate)
    const float* lnw;          // the conv module's LayerNorm
    const float* lnb;
    const float* R;            // residual stream in  [nseq * seq_t, 256]
    float* R2;                 // residual stream out (may alias R)
    float* C;                  // GLU output, padded layout [nseq][out_pad_tot + seq_t][256], real rows at out_pad_l
    const int* lens;           // feature lengths for the pad mask, or nullptr
    int seq_t, mstride, out_pad_l, out_pad_tot;
    float eps;
};
#if MASR_EXPERIMENTS
bool launch_attn_chain(const AttnChainArgs& a, int max_nq, hipStream_t s);
#else
inline bool launch_attn_chain(const AttnChainArgs&, int, hipStream_t) { return false; }
#endif
// encoder_conf.pos_enc_layer_type of the Conformer (masr_config.reserved[2]; conformer/encoder.py:239-281)
enum PosEnc { POS_ENC_REL = 0, POS_ENC_ABS = 1, POS_ENC_NONE = 2 };
// which instantiations launch_attention runs: with the relative-position term, or the plain q . k^T / sqrt(d_k) of
// MultiHeadedAttention (abs_pos and no_pos alike: they differ in the embedding only)
enum AttPos { ATT_REL_POS = 0, ATT_NO_POS = 1 };
// row_w = heads * 64: the row stride of AttSeq::out and of ptab [max_pos, row_w] (256; the wide Conformer path: 512)
// pos_mode ATT_NO_POS: ptab / bias_u / bias_v are not read (may be null), pos_stride still scales the chunk mask
void launch_attention(const AttSeq* seqs, int nseq, int max_nq, int heads, int q_stride, int kv_stride,
                      const float* ptab /*[max_pos,row_w]*/, const float* bias_u, const float* bias_v,
                      int chunk_size, int pos_stride, hipStream_t s, int row_w, int pos_mode);
// x [nseq * Tq, d] += pe[offs[b] + t] (abs_pos embedding; offs == nullptr: offset 0); rows at or past n_pos are not touched
void launch_add_pos_rows(float* x, const float* pe, const int* offs, int nseq, int Tq, int d, int n_pos, hipStream_t s);
void launch_attention_grouped(const AttSeq* seqs, int nseq, int max_nq, int heads, int group, const float* ptab,
                              int t_true, const float* bias_u, const float* bias_v, hipStream_t s, int chunk_size = 0);
void launch_attseq_grouped(AttSeq* seqs, const float* q, const float* k, const float* v, float* out, const int* lens,
                           int B, int Tg, int group, int mstride, hipStream_t s);
void launch_kv_append(const AttSeq* seqs, const float* qkv, int n, int Tq, hipStream_t s);
void launch_cnn_cache_move(float* const* caches, float* lnpad, int n, int Tq, int pad, int dir, hipStream_t s);
// streaming conv-module front in one launch: history rows <- cache_rd, new rows <- LayerNorm / affine of x, cache_wr <- last pad rows
void launch_conv_hist(const float* x, const float* w, const float* b, float* const* cache_rd, float* const* cache_wr,
                      float* lnpad, int n, int Tq, int pad, int affine, float eps, hipStream_t s);
void launch_attseq_full(AttSeq* seqs, const float* qkv, float* out, const int* lens, int B, int Tp, int mstride,
                        hipStream_t s, int valid_only = 0);     // valid_only: nq = nk = klen (padded queries / keys are not touched)

// ---- width-generic Conformer path (wide.hip): counterparts of the 256-only row kernels, rows of width d ------------------------
// wide_supported(d): the widths the templated kernels are instantiated for (256, 512).  The bool launchers are those templated on the
// width: false, with nothing launched, for any other d.  The void launchers (conv1, glu(bias), sequence descriptors) run plain
// kernels that take d at run time and serve any width.
bool wide_supported(int d);
// launch_layernorm at width d (same remap into the padded layout and pad masking)
bool launch_layernorm_wide(const float* x, const float* w, const float* b, float* y, int M, int d, float eps, int seq_t, int pad,
                           const int* lens, hipStream_t s);
// launch_conv1 for more than 256 output channels
void launch_conv1_wide(const float* feats, const float* mean, const float* istd, const float* w9c, const float* bias, float* out,
                       int B, int T, int F, int C, hipStream_t s);
// out [M, d] = value * sigmoid(gate) of in [M, 2 d] (value | gate: a pointwise_conv1 output with its bias added)
bool launch_glu_wide(const float* in, float* out, int M, int d, hipStream_t s);
void launch_glu_const_wide(const float* bias2d, float* out, int d, hipStream_t s);      // launch_glu_const at width d
// depthwise conv (1 <= ktaps <= 32) + LayerNorm(d) + act (a GemmAct from ACT_RELU to ACT_SELU): g [nseq][in_pad + Tq][d] (in_pad materialised history rows) -> out [nseq * Tq, d];
// tap j of output frame t reads input frame t + j - pad_l; frames in front of the materialised rows read gconst [d] (nullptr:
// zero), frames behind the sequence read zero
bool launch_dwconv_ln_silu_wide(const float* g, const float* wkc, const float* bias, const float* lnw, const float* lnb, float* out,
                                int nseq, int Tq, int d, int ktaps, int in_pad, int pad_l, float eps, const float* gconst, int act,
                                hipStream_t s);
// launch_conv_hist (LayerNorm variant) at width d
bool launch_conv_hist_wide(const float* x, const float* w, const float* b, float* const* cache_rd, float* const* cache_wr,
                           float* lnpad, int n, int Tq, int pad, int d, float eps, hipStream_t s);
bool launch_kv_append_wide(const AttSeq* seqs, const float* qkv, int n, int Tq, int d, hipStream_t s);   // qkv [n * Tq, 3 d]
// launch_attseq_full over a [B * Tp, 3 d] q | k | v buffer and [B * Tp, d] output rows (conv2d rate: 4 feature frames per frame)
void launch_attseq_full_wide(AttSeq* seqs, const float* qkv, float* out, const int* lens, int B, int Tp, int d, hipStream_t s);

// ---- attention decoder of the second pass (decoder.hip) ------------------------------------------------------------
// Row space [S = B * N sequences][Lmax + 1 positions]; hyp [S, Lmax] int32 token ids, lens [S] their lengths (clamped to [0, Lmax]
// in the kernels).  reverse = 1: the right-to-left decoder's view of the same table.
// x [S * (Lmax + 1), d] <- emb[token] * sqrt(d) + pe[position]; rows past a hypothesis' length are zeroed
void launch_dec_embed(const int* hyp, const int* lens, const float* emb, const float* pe, float* x, int S, int Lmax, int d, int V,
                      int reverse, hipStream_t s);
// few-query attention over heads of 64: causal = 1 over the sequence's own rows (k / v rows of the same row space), causal = 0 over
// the Tp encoder frames of utterance s / N (k / v rows [B * Tp]), keys j < key_lens[s / N]
void launch_dec_attention(const float* q, int q_stride, const float* k, const float* v, int kv_stride, float* out, int out_stride,
                          const int* hyp_lens, const int* key_lens, int S, int N, int Lmax, int Tp, int heads, int causal,
                          hipStream_t s);
// out [S] = sum over positions 0 .. L of log_softmax(logits [row, V])[target]; rowlp [S * (Lmax + 1)] scratch
void launch_dec_scores(const float* logits, const int* hyp, const int* lens, float* rowlp, float* out, int S, int Lmax, int V,
                       int reverse, hipStream_t s);

// ---- attention decoder, one autoregressive step (decoder_step.hip; decoder: attention) ----
// Row s = b * N + n; step i handles position p = i - 1.  tok / anc [S, Lcap] int32: the tokens after sos and, per position j < p,
// the rank whose cache slot holds the hypothesis' position j.
// x [S, d] = emb[last token] * sqrt(d) + pe[p]  (last token: sos = V - 1 at p = 0, else tok[s][p - 1])
void launch_step_embed(const int* tok, const float* emb, const float* pe, float* x, int S, int p, int Lcap, int d, int V,
                       hipStream_t s);
// one query per (hypothesis, head of 64), the keys split over the lanes of a wave.  anc given: self-attention over positions
// 0 .. p of the cache kv [Lrun][S][2 d] (key p is the row's own slot); anc null: source attention over the key_lens[s / N] frames of
// kv [B * Tp][2 d]
void launch_step_attention(const float* q, int q_stride, const float* kv, float* out, const int* anc, const int* key_lens, int S,
                           int N, int Tp, int Lcap, int p, int d, int heads, hipStream_t s);
// log_softmax + top n of each logits row (larger first, bit-equal values: the smaller id first) -> top_v / top_i [S, n]; full
// [S, V] log-probabilities when given; only_pos [S] given: a row writes at p == only_pos[row] alone
void launch_step_topn(const float* logits, int S, int V, int n, float* top_v, int* top_i, float* full, const int* only_pos, int p,
                      hipStream_t s);
struct StepMerge {           // the merge kernel's argument
    const float* top_v;      // [S, N]
    const int* top_i;        // [S, N]
    const float* score_cur;  // [S]
    float* score_next;
    const int* tok_cur;      // [S, Lcap]
    int* tok_next;
    const int* anc_cur;      // [S, Lcap]
    int* anc_next;
    const int* enc_lens;     // [B]
    int* done;               // [B] 0 / 1
    int* active;             // [1] utterances not done
    int N, Lcap, Tp, V, p, max_len, max_pos;
};
// beam merge of step p + 1, per utterance (finished-row masking, N x N top N with ties to the smaller flat index, tables through
// the parent index, the count of utterances still running in *active)
void launch_step_merge(const StepMerge& m, int B, hipStream_t s);
void launch_step_init(float* score, int* done, int* active, const int* enc_lens, int B, int N, int Tp, int Lcap, int max_len,
                      int max_pos, hipStream_t s);
void launch_step_result(const int* tok, const float* score, const int* enc_lens, int* tokens_out, int* lens_out, float* scores_out,
                        int S, int N, int Lcap, int Tp, int V, int steps, int max_len, int max_pos, hipStream_t s);

// ---- joint CTC / attention search (decoder_joint.hip; decoder: joint) ----
// The CTC prefix state of row s: r [S][2][Tp] float32 = r_n | r_b over the frames of its utterance, two such buffers (read `cur`,
// write `next`).  Row s belongs to utterance row_utt[s] (given: the scorer op) or s / N; blank = id 0, eos = V - 1.
struct PrefixRows {
    const float* post;       // [B, Tp, V] posteriors (input_is_log = 0: probabilities, the kernels take the logarithm)
    const int* enc_lens;     // [B] valid frames (clamped to [0, Tp])
    const int* row_utt;      // [S] or nullptr
    const int* done;         // [B] or nullptr: rows of a finished utterance are skipped
    int S, N, V, Tp, input_is_log;
};
// r <- the empty prefix: r_n = -inf, r_b[t] = sum of lp[0 .. t][blank]
void launch_prefix_init(const PrefixRows& pr, float* r, hipStream_t s);
// psi_out [S, M] = log CTC prefix probability of row s extended by cand [S, M] (lane m = candidate m); tok [S, Lcap] holds the
// row's p tokens.  only_pos [S] given: a row writes at p == only_pos[row] alone.  Rows whose last token is eos are skipped.
void launch_prefix_score(const PrefixRows& pr, const int* cand, int M, const int* tok, int Lcap, int p, const int* only_pos,
                         const float* r_cur, float* psi_out, hipStream_t s);
// r_next[s] <- r_cur[parent of s] extended by tok_next[s][p], parent = rank anc_next[s][p] of the row's utterance; a row that ends
// in eos is left alone.  row_len [S] given (the scorer op): rows with p >= row_len[s] copy their own state.
void launch_prefix_advance(const PrefixRows& pr, const int* tok_next, const int* anc_next, int Lcap, int p, const int* row_len,
                           const float* r_cur, float* r_next, hipStream_t s);
struct JointMerge {          // the joint merge kernel's argument
    const float* top_v;      // [S, M] attention log-probabilities of the candidates
    const int* top_i;        // [S, M]
    const float* psi_cand;   // [S, M] or nullptr (ctc_weight 0)
    const float* lm_cand;    // [S, M] or nullptr (lm_weight 0): lm(g, c) of the candidates
    const float *key_cur, *att_cur, *psi_cur, *lm_cur;      // [S] J, A, psi, Lm
    float *key_next, *att_next, *psi_next, *lm_next;
    const int* n_cur;        // [S] tokens other than eos
    int* n_next;
    const int* tok_cur;      // [S, Lcap]
    int* tok_next;
    const int* anc_cur;      // [S, Lcap]
    int* anc_next;
    const int* enc_lens;     // [B]
    int* done;               // [B] 0 / 1
    int* active;             // [1] utterances not done
    int N, M, Lcap, Tp, V, p, max_len, max_pos;
    float ctc_weight, lm_weight, length_bonus;
};
// beam merge of step p + 1 by J = (((1 - ctc_weight) A + ctc_weight psi) + lm_weight Lm) + length_bonus n (the psi / Lm term left
// out where its candidate table is null): N of the N x M candidates per utterance, ties to the smaller flat index parent * M +
// candidate; A, psi, Lm, n, tokens and ancestors carried through the parent index
void launch_joint_merge(const JointMerge& m, int B, hipStream_t s);
// att [S] = [0, -inf, ...] per utterance, psi = 0, Lm = 0, n = 0
void launch_joint_init(float* att, float* psi, float* lm, int* n, int S, int N, hipStream_t s);
// lm_out [S, M] = ln P(cand [S, M] | the row's tokens) of the n-gram model `lm` (a device view), bit-equal to
// masr_lm_cond_log_prob; one wave per row, lane m = candidate m.  tok [S, Lcap] holds p tokens per row, or row_len [S] of them
// when that is given (the op; no row counts as finished then).  done [B] or nullptr: rows s / N of a finished utterance are
// skipped, and so are rows whose last token is eos.  Returns non-zero for a model order outside 1 .. 5.
int launch_joint_lm_score(const LmView& lm, const int* cand, int M, const int* tok, int Lcap, int p, const int* row_len,
                          const int* done, int S, int N, int V, float* lm_out, hipStream_t s);

// ---- features ------------------------------------------------------------------------------
size_t fbank_gain_scratch_floats(int B);   // size of gain_scratch ([B] gains + partial sums)
// use_db: 0 = no dB normalisation, 1 = gains computed on the device, 2 = gains supplied in gain_scratch[0 .. B)
// tables of the fbank front-end (engine_frontend.hip build_fbank_tables): povey window [400]; mel weights transposed [16 taps][80] (tap i of
// filter m = bin mel_lo[m] + i, zero past the filter's last bin); W512^k (k <= 256) for the real-split pass; twr4 [3 passes][3][64]:
// the twiddles of the radix-4 passes Ns = 4, 16, 64 per lane
struct FbankTables {
    const float *window, *melwt, *tw512, *twr4;
    const int* mel_lo;
};
void launch_fbank(const void* pcm, int sample_format /*0 int16, 1 float32*/, const int* nsamp, int B, int n_max,
                  int use_db, float target_db, const FbankTables& tb, float* feats, int T_max, float* gain_scratch,
                  int16_t* norm_out, hipStream_t s);
void launch_mean_square(const void* pcm, int sample_format, const int* nsamp, int B, int n_max, float* gain_scratch,
                        float* ms_out, hipStream_t s);
void launch_mfcc(const float* fbank, long rows, int n_ceps, const float* dct /*[80][n_ceps]*/, const float* lifter, float* out,
                 hipStream_t s);
void launch_linear_spec(const void* pcm, int sample_format, const int* nsamp, int B, int n_max, int use_db, const float* gain,
                        const double* win /*[320]*/, const double* tw /*[320][2]*/, double scale, float* feats /*[B][T_max][161]*/,
                        int T_max, hipStream_t s);
void launch_linear_frame_counts(const int* nsamp, int B, int* nfr, hipStream_t s);
// resample.hip: rows of one source rate -> float32 rows at ratio x that rate, scattered into dst [.., dst_stride] and zero-filled
// behind their own length.  rows_dev [R][3] int32 = samples in | samples out | destination row; table [nwin][2] double = (win[k],
// dwin[k]) pairs, nullptr = the rows are at the target rate already (converted and copied)
void launch_resample_rows(const void* src, int sample_format /*0 int16, 1 float32*/, long src_stride, const int* rows_dev, int R,
                          double ratio, const double* table, int nwin, int num_table, float* dst, long dst_stride, hipStream_t s);
// resample.hip: the off-rate feeds of a streaming step in ONE launch over tiles_dev [n_tiles][2] = (feed, first output); every feed
// writes dst[dst_row][dst_offset .. + n_out) only.  Descriptors: masr_hip.h; lds_floats: the dynamic LDS that stages a tile's inputs
void launch_resample_feeds(const void* src, const ::masr_resample_feed* feeds_dev, int n_feeds, const ::masr_resample_rate* rates_dev,
                           const int* tiles_dev, long n_tiles, int lds_floats, float* dst, long dst_stride, hipStream_t s);

}  // namespace masr
