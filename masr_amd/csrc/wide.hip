// Row kernels of the width-generic Conformer path (output_size 512 / attention_heads 8, and output_size 256 with an
// activation_type other than swish): the counterparts of the 256-only kernels of elementwise.hip / attention.hip.  Every kernel
// performs the arithmetic steps of its 256 counterpart in the same order.
// * Templated on the row width D (a multiple of 256; instantiated for 256 and 512): LayerNorm, GLU, depthwise conv + LayerNorm +
//   activation (a second template argument: the GemmAct behind the norm), the streaming conv front and kv_append.  Bandwidth-bound: one wave per row, D / 256 float4 per lane (lane l holds columns
//   256 i + 4 l .. + 3), DPP wave reductions.  Their launchers return bool: false, with nothing launched, for a width they are
//   not instantiated for -- the engine turns that into an error, never into another code path.
// * Plain kernels that take the width at run time and so serve any d (void launchers, nothing to refuse): conv1 for more
//   channels than threads, glu(bias) and the full-context sequence descriptors.
#include "common.h"

namespace masr {

namespace {

template <int D>
struct RowVec {
    static constexpr int V = D / 256;
    f32x4 v[V];
};

template <int D>
__device__ __forceinline__ RowVec<D> load_row(const float* p, int lane) {
    RowVec<D> r;
#pragma unroll
    for (int i = 0; i < RowVec<D>::V; ++i) r.v[i] = *reinterpret_cast<const f32x4*>(p + i * 256 + lane * 4);
    return r;
}
template <int D>
__device__ __forceinline__ void store_row(float* p, int lane, const RowVec<D>& r) {
#pragma unroll
    for (int i = 0; i < RowVec<D>::V; ++i) *reinterpret_cast<f32x4*>(p + i * 256 + lane * 4) = r.v[i];
}
template <int D>
__device__ __forceinline__ RowVec<D> zero_row() {
    RowVec<D> r;
#pragma unroll
    for (int i = 0; i < RowVec<D>::V; ++i) r.v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    return r;
}

// LayerNorm of one row held by one wave: two-pass variance in registers, eps inside the square root (layernorm256_kernel)
template <int D>
__device__ __forceinline__ RowVec<D> layernorm_row(const RowVec<D>& x, const float* __restrict__ w, const float* __restrict__ b,
                                                   float eps, int lane) {
    constexpr int V = RowVec<D>::V;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) sum += x.v[i][0] + x.v[i][1] + x.v[i][2] + x.v[i][3];
    const float mean = wave_sum_dpp(sum) * (1.0f / D);
    RowVec<D> dv;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) dv.v[i][k] = x.v[i][k] - mean;
        sq += dv.v[i][0] * dv.v[i][0] + dv.v[i][1] * dv.v[i][1] + dv.v[i][2] * dv.v[i][2] + dv.v[i][3] * dv.v[i][3];
    }
    const float var = wave_sum_dpp(sq) * (1.0f / D);
    const float rstd = 1.0f / sqrtf(var + eps);
    const RowVec<D> ww = load_row<D>(w, lane), bb = load_row<D>(b, lane);
    RowVec<D> o;
#pragma unroll
    for (int i = 0; i < V; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) o.v[i][k] = dv.v[i][k] * rstd * ww.v[i][k] + bb.v[i][k];
    return o;
}

// LayerNorm over rows of width D; seq_t > 0: output row b * (seq_t + pad) + pad + t, rows with 4 t >= lens[b] zeroed
template <int D>
__global__ __launch_bounds__(256) void layernorm_wide_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ b, float* y, int M, float eps, int seq_t,
                                                             int pad, const int* __restrict__ lens) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    size_t orow = row;
    bool zero = false;
    if (seq_t > 0) {
        const int bb = row / seq_t, t = row - bb * seq_t;
        orow = (size_t)bb * (seq_t + pad) + pad + t;
        if (lens && 4 * t >= lens[bb]) zero = true;
    }
    const RowVec<D> o = zero ? zero_row<D>() : layernorm_row<D>(load_row<D>(x + (size_t)row * D, lane), w, b, eps, lane);
    store_row<D>(y + orow * D, lane, o);
}

// CMVN + Conv2d(1 -> C, 3x3, stride 2) + ReLU, channels-last output (conv1_kernel with more channels than threads)
__global__ __launch_bounds__(256) void conv1_wide_kernel(const float* __restrict__ feats, const float* __restrict__ mean,
                                                         const float* __restrict__ istd, const float* __restrict__ w9c,
                                                         const float* __restrict__ bias, float* __restrict__ out, int T, int F,
                                                         int T1, int F1, int C) {
    extern __shared__ float sm[];  // [3][F]
    const int bt = blockIdx.x;
    const int b = bt / T1, t1 = bt % T1;
    for (int i = threadIdx.x; i < 3 * F; i += blockDim.x) {
        const int kh = i / F, f = i % F;
        const float v = feats[((size_t)b * T + 2 * t1 + kh) * F + f];
        sm[i] = (v - mean[f]) * istd[f];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float w[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) w[i] = w9c[i * C + c];
        const float bv = bias[c];
        float* o = out + ((size_t)bt * F1) * C + c;
        for (int f1 = 0; f1 < F1; ++f1) {
            float acc = bv;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) acc = fmaf(w[kh * 3 + kw], sm[kh * F + 2 * f1 + kw], acc);
            o[(size_t)f1 * C] = fmaxf(acc, 0.f);
        }
    }
}

// GLU over the two halves of a pointwise_conv1 output [M, 2 D] (value | gate, bias already added) with the arithmetic of the
// row-block GLU epilogue: out = value * rcp(1 + exp(-gate))
template <int D>
__global__ __launch_bounds__(256) void glu_wide_kernel(const float* __restrict__ in, float* __restrict__ out, long n4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const long row = i / (D / 4);
    const int c4 = (int)(i - row * (D / 4)) * 4;
    const f32x4 a = *reinterpret_cast<const f32x4*>(in + row * 2 * D + c4);
    const f32x4 g = *reinterpret_cast<const f32x4*>(in + row * 2 * D + D + c4);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = a[k] * __builtin_amdgcn_rcpf(1.0f + __expf(-g[k]));
    *reinterpret_cast<f32x4*>(out + row * D + c4) = o;
}

// glu(bias) of pointwise_conv1 [2 d]: the constant history row of the offline causal conv module (glu_const_kernel)
__global__ void glu_const_wide_kernel(const float* __restrict__ bias, float* __restrict__ out, int d) {
    for (int c = threadIdx.x; c < d; c += blockDim.x) out[c] = bias[c] * __builtin_amdgcn_rcpf(1.0f + __expf(-bias[d + c]));
}

// Depthwise Conv1d (KT taps) + LayerNorm(D) + activation ACT (a GemmAct; ACT_SILU: dwconv_ln_silu_kernel).  Input: GLU rows [nseq][in_pad + Tq][D], real rows
// behind in_pad materialised history rows.  Output frame t sums taps j over input frame t + j - pad_l (pad_l = KT - 1: causal,
// (KT - 1) / 2: symmetric).  An input frame in front of the materialised rows reads gconst (the constant glu(bias) history row of
// the offline causal conv) or zero; a frame behind the sequence reads zero.  Workgroup = 16 output frames of one sequence;
// thread = channel (D / 256 of them in turn) for the sliding window, then the tile goes through LDS and each wave normalises rows.
static constexpr int WDW_TT = 16;
template <int D, int KT, int ACT>
__global__ __launch_bounds__(256) void dwconv_ln_silu_wide_kernel(const float* __restrict__ g, const float* __restrict__ wkc,
                                                                  const float* __restrict__ bias, const float* __restrict__ lnw,
                                                                  const float* __restrict__ lnb, float* __restrict__ out, int Tq,
                                                                  int in_pad, int pad_l, float eps,
                                                                  const float* __restrict__ gconst) {
    __shared__ __align__(16) float tile[WDW_TT][D + 4];
    const int tiles = (Tq + WDW_TT - 1) / WDW_TT;
    const int seq = blockIdx.x / tiles;
    const int t0 = (blockIdx.x % tiles) * WDW_TT;
    const int nrows = min(WDW_TT, Tq - t0);
    const float* gseq = g + ((size_t)seq * (in_pad + Tq) + in_pad) * D;      // frame 0 of this sequence
    for (int c = threadIdx.x; c < D; c += 256) {
        float w[KT], win[KT];
#pragma unroll
        for (int j = 0; j < KT; ++j) w[j] = wkc[j * D + c];
        const float bv = bias[c];
        const float gc = gconst ? gconst[c] : 0.f;
        auto frame = [&](int ti) -> float {
            if (ti >= Tq) return 0.f;
            if (ti >= -in_pad) return gseq[(long)ti * D + c];
            return gc;
        };
        win[0] = 0.f;
#pragma unroll
        for (int j = 0; j < KT - 1; ++j) win[j + 1] = frame(t0 + j - pad_l);
        for (int r = 0; r < nrows; ++r) {
#pragma unroll
            for (int j = 0; j < KT - 1; ++j) win[j] = win[j + 1];
            win[KT - 1] = frame(t0 + r + KT - 1 - pad_l);
            float acc = bv;                       // out[t] = b + sum_j w[j] * in[t + j - pad_l]
#pragma unroll
            for (int j = 0; j < KT; ++j) acc = fmaf(w[j], win[j], acc);
            tile[r][c] = acc;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < nrows; r += 4) {
        RowVec<D> o = layernorm_row<D>(load_row<D>(&tile[r][0], lane), lnw, lnb, eps, lane);
#pragma unroll
        for (int i = 0; i < RowVec<D>::V; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) o.v[i][k] = act_f<ACT>(o.v[i][k]);
        store_row<D>(out + ((size_t)seq * Tq + t0 + r) * D, lane, o);
    }
}

// The same for tap counts without an instantiation (dwconv_ln_silu_taps_kernel of elementwise.hip): KMAX = 8 / 16 / 32 registers,
// the tap count K <= KMAX at run time, tap j in slot KMAX - K + j; same steps in the same order as dwconv_ln_silu_wide_kernel<D, K, ACT>.
template <int D, int KMAX, int ACT>
__global__ __launch_bounds__(256) void dwconv_ln_silu_wide_taps_kernel(const float* __restrict__ g, const float* __restrict__ wkc,
                                                                       const float* __restrict__ bias,
                                                                       const float* __restrict__ lnw,
                                                                       const float* __restrict__ lnb, float* __restrict__ out, int K,
                                                                       int Tq, int in_pad, int pad_l, float eps,
                                                                       const float* __restrict__ gconst) {
    __shared__ __align__(16) float tile[WDW_TT][D + 4];
    const int tiles = (Tq + WDW_TT - 1) / WDW_TT;
    const int seq = blockIdx.x / tiles;
    const int t0 = (blockIdx.x % tiles) * WDW_TT;
    const int nrows = min(WDW_TT, Tq - t0);
    const int off = KMAX - K;                                                // slot of tap 0
    const float* gseq = g + ((size_t)seq * (in_pad + Tq) + in_pad) * D;      // frame 0 of this sequence
    for (int c = threadIdx.x; c < D; c += 256) {
        float w[KMAX], win[KMAX];
#pragma unroll
        for (int jj = 0; jj < KMAX; ++jj) w[jj] = jj >= off ? wkc[(jj - off) * D + c] : 0.f;
        const float bv = bias[c];
        const float gc = gconst ? gconst[c] : 0.f;
        auto frame = [&](int ti) -> float {
            if (ti >= Tq) return 0.f;
            if (ti >= -in_pad) return gseq[(long)ti * D + c];
            return gc;
        };
        win[0] = 0.f;
#pragma unroll
        for (int jj = 1; jj < KMAX; ++jj) win[jj] = jj - 1 < off ? 0.f : frame(t0 + jj - 1 - off - pad_l);
        for (int r = 0; r < nrows; ++r) {
#pragma unroll
            for (int jj = 0; jj < KMAX - 1; ++jj) win[jj] = win[jj + 1];
            win[KMAX - 1] = frame(t0 + r + K - 1 - pad_l);
            float acc = bv;                       // out[t] = b + sum_j w[j] * in[t + j - pad_l]
#pragma unroll
            for (int jj = 0; jj < KMAX; ++jj)
                if (jj >= off) acc = fmaf(w[jj], win[jj], acc);
            tile[r][c] = acc;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < nrows; r += 4) {
        RowVec<D> o = layernorm_row<D>(load_row<D>(&tile[r][0], lane), lnw, lnb, eps, lane);
#pragma unroll
        for (int i = 0; i < RowVec<D>::V; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) o.v[i][k] = act_f<ACT>(o.v[i][k]);
        store_row<D>(out + ((size_t)seq * Tq + t0 + r) * D, lane, o);
    }
}

// streaming conv-module front (conv_hist_kernel, LayerNorm variant): lnpad[i][tp] = tp < pad ? cache_rd[i][tp] :
// LayerNorm(x[i][tp - pad]); cache_wr[i][r] = lnpad[i][Tq + r].  One wave per padded row.
template <int D>
__global__ __launch_bounds__(256) void conv_hist_wide_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ b, float* const* __restrict__ cache_rd,
                                                             float* const* __restrict__ cache_wr, float* __restrict__ lnpad, int n,
                                                             int Tq, int pad, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int per = Tq + pad;
    if (row >= n * per) return;
    const int i = row / per, tp = row - i * per;
    const RowVec<D> o = tp < pad ? load_row<D>(cache_rd[i] + (size_t)tp * D, lane)
                                 : layernorm_row<D>(load_row<D>(x + ((size_t)i * Tq + tp - pad) * D, lane), w, b, eps, lane);
    store_row<D>(lnpad + (size_t)row * D, lane, o);
    if (tp >= Tq) store_row<D>(cache_wr[i] + (size_t)(tp - Tq) * D, lane, o);
}

// append the chunk's k | v columns of the fused QKV projection [n * Tq, 3 D] to every stream's cache (rows [k (D) | v (D)], the new
// rows at positions nk - nq .. nk - 1): kv_append_kernel
template <int D>
__global__ __launch_bounds__(D / 2) void kv_append_wide_kernel(const AttSeq* __restrict__ seqs, const float* __restrict__ qkv, int Tq) {
    const int i = blockIdx.y, r = blockIdx.x;
    const AttSeq sq = seqs[i];
    float* dst = const_cast<float*>(sq.k) + (size_t)(sq.nk - sq.nq + r) * 2 * D;
    const float* src = qkv + ((size_t)i * Tq + r) * 3 * D + D;
    reinterpret_cast<f32x4*>(dst)[threadIdx.x] = reinterpret_cast<const f32x4*>(src)[threadIdx.x];
}

// sequence descriptors of the full-context batch: q | k | v interleaved in one [B * Tp, 3 d] buffer (attseq_full_kernel)
__global__ void attseq_full_wide_kernel(AttSeq* seqs, const float* qkv, float* out, const int* __restrict__ lens, int B, int Tp,
                                        int d) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    AttSeq s;
    s.q = qkv + (size_t)b * Tp * 3 * d;
    s.k = s.q + d;
    s.v = s.q + 2 * d;
    s.out = out + (size_t)b * Tp * d;
    s.nq = Tp;
    s.nk = Tp;
    s.klen = lens ? min(Tp, (lens[b] + 3) / 4) : Tp;
    s.pos0 = 0;
    s.q_abs0 = 0;
    s.pad_ = 0;
    seqs[b] = s;
}

}  // namespace

bool wide_supported(int d) { return d == 256 || d == 512; }

bool launch_layernorm_wide(const float* x, const float* w, const float* b, float* y, int M, int d, float eps, int seq_t, int pad,
                           const int* lens, hipStream_t s) {
    if (!wide_supported(d)) return false;
    if (M <= 0) return true;
    const dim3 grid((M + 3) / 4), blk(256);
    if (d == 256) hipLaunchKernelGGL(layernorm_wide_kernel<256>, grid, blk, 0, s, x, w, b, y, M, eps, seq_t, pad, lens);
    else hipLaunchKernelGGL(layernorm_wide_kernel<512>, grid, blk, 0, s, x, w, b, y, M, eps, seq_t, pad, lens);
    return true;
}

void launch_conv1_wide(const float* feats, const float* mean, const float* istd, const float* w9c, const float* bias, float* out,
                       int B, int T, int F, int C, hipStream_t s) {
    const int T1 = (T - 1) / 2, F1 = (F - 1) / 2;
    if (B * T1 <= 0) return;
    hipLaunchKernelGGL(conv1_wide_kernel, dim3(B * T1), dim3(256), 3 * F * sizeof(float), s, feats, mean, istd, w9c, bias, out, T, F,
                       T1, F1, C);
}

bool launch_glu_wide(const float* in, float* out, int M, int d, hipStream_t s) {
    if (!wide_supported(d)) return false;
    if (M <= 0) return true;
    const long n4 = (long)M * (d / 4);
    const dim3 grid((unsigned)((n4 + 255) / 256)), blk(256);
    if (d == 256) hipLaunchKernelGGL(glu_wide_kernel<256>, grid, blk, 0, s, in, out, n4);
    else hipLaunchKernelGGL(glu_wide_kernel<512>, grid, blk, 0, s, in, out, n4);
    return true;
}

void launch_glu_const_wide(const float* bias2d, float* out, int d, hipStream_t s) {
    hipLaunchKernelGGL(glu_const_wide_kernel, dim3(1), dim3(256), 0, s, bias2d, out, d);
}

namespace {
// the tap class of a kernel size: 15 has an instantiation of its own, every other count runs on 8 / 16 / 32 tap registers
template <int D, int ACT>
void launch_dwconv_wide_t(const float* g, const float* wkc, const float* bias, const float* lnw, const float* lnb, float* out, int nseq,
                          int Tq, int ktaps, int in_pad, int pad_l, float eps, const float* gconst, hipStream_t s) {
    const int tiles = (Tq + WDW_TT - 1) / WDW_TT;
    const dim3 grid(nseq * tiles), blk(256);
    if (ktaps == 15)
        hipLaunchKernelGGL((dwconv_ln_silu_wide_kernel<D, 15, ACT>), grid, blk, 0, s, g, wkc, bias, lnw, lnb, out, Tq, in_pad, pad_l, eps,
                           gconst);
    else if (ktaps <= 8)
        hipLaunchKernelGGL((dwconv_ln_silu_wide_taps_kernel<D, 8, ACT>), grid, blk, 0, s, g, wkc, bias, lnw, lnb, out, ktaps, Tq, in_pad,
                           pad_l, eps, gconst);
    else if (ktaps <= 16)
        hipLaunchKernelGGL((dwconv_ln_silu_wide_taps_kernel<D, 16, ACT>), grid, blk, 0, s, g, wkc, bias, lnw, lnb, out, ktaps, Tq, in_pad,
                           pad_l, eps, gconst);
    else
        hipLaunchKernelGGL((dwconv_ln_silu_wide_taps_kernel<D, 32, ACT>), grid, blk, 0, s, g, wkc, bias, lnw, lnb, out, ktaps, Tq, in_pad,
                           pad_l, eps, gconst);
}
template <int D>
bool launch_dwconv_wide_d(int act, const float* g, const float* wkc, const float* bias, const float* lnw, const float* lnb, float* out,
                          int nseq, int Tq, int ktaps, int in_pad, int pad_l, float eps, const float* gconst, hipStream_t s) {
    switch (act) {
#define MASR_WDW_ACT(A) \
    case A: launch_dwconv_wide_t<D, A>(g, wkc, bias, lnw, lnb, out, nseq, Tq, ktaps, in_pad, pad_l, eps, gconst, s); return true;
    MASR_WDW_ACT(ACT_RELU)
    MASR_WDW_ACT(ACT_SILU)
    MASR_WDW_ACT(ACT_GELU)
    MASR_WDW_ACT(ACT_TANH)
    MASR_WDW_ACT(ACT_HARDTANH)
    MASR_WDW_ACT(ACT_SELU)
#undef MASR_WDW_ACT
    default: return false;       // (ACT_NONE is no activation_type: refused like an unknown width)
    }
}
}  // namespace

bool launch_dwconv_ln_silu_wide(const float* g, const float* wkc, const float* bias, const float* lnw, const float* lnb, float* out,
                                int nseq, int Tq, int d, int ktaps, int in_pad, int pad_l, float eps, const float* gconst, int act,
                                hipStream_t s) {
    if (!wide_supported(d) || ktaps < 1 || ktaps > 32 || act < ACT_RELU || act > ACT_SELU) return false;
    if (nseq * Tq <= 0) return true;
    return d == 256 ? launch_dwconv_wide_d<256>(act, g, wkc, bias, lnw, lnb, out, nseq, Tq, ktaps, in_pad, pad_l, eps, gconst, s)
                    : launch_dwconv_wide_d<512>(act, g, wkc, bias, lnw, lnb, out, nseq, Tq, ktaps, in_pad, pad_l, eps, gconst, s);
}

bool launch_conv_hist_wide(const float* x, const float* w, const float* b, float* const* cache_rd, float* const* cache_wr,
                           float* lnpad, int n, int Tq, int pad, int d, float eps, hipStream_t s) {
    if (!wide_supported(d)) return false;
    const int rows = n * (Tq + pad);
    if (rows <= 0) return true;
    const dim3 grid((rows + 3) / 4), blk(256);
    if (d == 256) hipLaunchKernelGGL(conv_hist_wide_kernel<256>, grid, blk, 0, s, x, w, b, cache_rd, cache_wr, lnpad, n, Tq, pad, eps);
    else hipLaunchKernelGGL(conv_hist_wide_kernel<512>, grid, blk, 0, s, x, w, b, cache_rd, cache_wr, lnpad, n, Tq, pad, eps);
    return true;
}

bool launch_kv_append_wide(const AttSeq* seqs, const float* qkv, int n, int Tq, int d, hipStream_t s) {
    if (!wide_supported(d)) return false;
    if (n * Tq <= 0) return true;
    // one thread per float4 of a k | v row (2 d floats): d / 2 threads, the kernel's launch bound
    if (d == 256) hipLaunchKernelGGL(kv_append_wide_kernel<256>, dim3(Tq, n), dim3(128), 0, s, seqs, qkv, Tq);
    else hipLaunchKernelGGL(kv_append_wide_kernel<512>, dim3(Tq, n), dim3(256), 0, s, seqs, qkv, Tq);
    return true;
}

void launch_attseq_full_wide(AttSeq* seqs, const float* qkv, float* out, const int* lens, int B, int Tp, int d, hipStream_t s) {
    hipLaunchKernelGGL(attseq_full_wide_kernel, dim3((B + 63) / 64), dim3(64), 0, s, seqs, qkv, out, lens, B, Tp, d);
}

}  // namespace masr
