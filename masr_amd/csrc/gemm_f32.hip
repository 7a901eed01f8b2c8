// fp32 GEMM on the CDNA4 matrix cores: C[M,N] = epilogue(A[M,K] * W[N,K]^T).
//
// * v_mfma_f32_32x32x2_f32 (exact fp32, == an fmaf chain): the reference computes this path in
//   fp32 (torch Linear / Conv on CPU), north_star asks for 1e-3 fp32 logit parity.
// * 256 threads = 4 wave64 per workgroup, WM x WN wave grid, each wave owns TM x TN tiles of 32x32.
// * K is consumed in BK=32 slabs, register-staged global->LDS with one barrier per slab
//   (double-buffered LDS).  LDS rows are padded to 36 floats so the ds_read_b128 fragment reads
//   (row = lane&31, 16-byte column = lane>>5) are bank-conflict free (row stride 144 B = 9 slots).
// * Fragment trick: MFMA sums over k in any order, so lane half h=(lane>>5) takes the 4 consecutive
//   k values {8g+4h .. 8g+4h+3} of each 8-wide k group with ONE 16-byte LDS read for A and for W.
// * A operand modes: plain row-major, or implicit-GEMM gather for the subsampling convs over channels-last
//   activations (reference conformer/subsampling.py:86-211): 3x3 stride 2 (A_CONV2) or 5x5 stride 3 (A_CONV5, conv2d6),
//   K ordered [32-channel block][kh][kw][channel] so that overlapping window columns are re-read while still cached.
//   A_ROWS: row m is row rows[m] of a row pool (the kept encoder frames of streaming sessions, masr_rescore_rows): the staging is
//   A_PLAIN's, 8 threads x float4 per slab row, only the source pointer differs; the row number is read once per row and thread
//   ahead of the K loop, the address is 64-bit, and a number outside [0, n_rows) stages zeros.  Bit-identical to A_PLAIN on the
//   gathered dense copy: the same tile shape at the same (M, N), so every output element sees the same MFMA chain from zero.
// * Epilogue: bias, ReLU/SiLU, alpha, residual, row masking.  (The K = 256 projections of the layers use
//   rowgemm.hip, the FFN ffn_pc.hip; this kernel serves conv2, the embed projection, the positional-key
//   precompute and the full-probability CTC head; the large offline conv2 runs on conv2_rows_kernel below.)
#include "common.h"

namespace masr {

static constexpr int BK = 32;
static constexpr int LDP = 36;   // padded LDS row (floats)

__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + expf(-x)); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// EPI_SPLITK: blockIdx.y owns a contiguous range of K slabs and stores its raw partial tile to p.C + blockIdx.y*M*ldc
// (p.ksplit slabs per range); splitk_reduce_kernel applies the epilogue.  For M so small that the tile grid cannot fill
// the chip while K is deep (embed projection of a streaming chunk step: M = 256, K = 4864).
// implicit-GEMM window of an A mode: KS x KS taps at stride S (A_CONV2: 3x3 stride 2, A_CONV5: 5x5 stride 3)
__host__ __device__ constexpr int conv_ks(int amode) { return amode == A_CONV5 ? 5 : 3; }
__host__ __device__ constexpr int conv_stride(int amode) { return amode == A_CONV5 ? 3 : 2; }

template <int BM, int BN, int WM, int WN, int AMODE, int EPI>
__global__ __launch_bounds__(64 * WM * WN) void gemm_f32_kernel(GemmArgs p) {
    static_assert(WM * WN == 4 || WM * WN == 8, "4 or 8 waves");
    constexpr int KS = conv_ks(AMODE), S = conv_stride(AMODE);
    constexpr int NT = 64 * WM * WN;
    constexpr int RPP = NT / 8;   // slab rows staged per pass of the workgroup (8 threads x float4 per 32-wide row)
    constexpr int TM = BM / WM / 32;
    constexpr int TN = BN / WN / 32;
    constexpr int AL = BM / RPP;  // float4 loads per thread for the A slab
    constexpr int WL = BN / RPP;
    extern __shared__ __align__(16) float smem[];
    float* As = smem;                       // [2][BM][LDP]
    float* Ws = smem + 2 * BM * LDP;        // [2][BN][LDP]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    // XCD-aware tile order: consecutive block ids land on different XCDs (id % 8); give every XCD a
    // contiguous range of M-tiles so that the W panel and neighbouring A rows stay in that XCD's L2.
    const int nbm = (p.M + BM - 1) / BM;
    const int nbn = (p.N + BN - 1) / BN;
    const int nblk = nbm * nbn;
    int bid = blockIdx.x;
    if (p.skip_rps <= 0) {          // (tiles are skipped by sequence length: contiguous per-XCD ranges would leave the XCDs of the
                                    //  short sequences idle -- plain order then, every XCD sees every sequence)
        const int q = nblk / 8, r = nblk % 8, xcd = bid % 8, idx = bid / 8;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int bm = (bid / nbn) * BM;
    const int bn = (bid % nbn) * BN;
    if (p.skip_rps > 0 && p.lens) {         // a tile of padded frames only (whole workgroup, before any barrier)
        const int span = min(bm + BM, p.M) - 1 - bm;
        const int b0 = bm / p.skip_rps, r0 = bm - b0 * p.skip_rps;
        if (r0 + span < p.skip_rps && 4 * (r0 / p.skip_div) >= p.lens[b0]) return;
    }

    // ---- per-thread global source pointers ------------------------------------------------
    const int lrow = tid >> 3;          // 0..RPP-1
    const int lc4 = (tid & 7) * 4;      // float offset inside the 32-wide slab
    const float* aptr[AL];
    bool aok[AL];
#pragma unroll
    for (int i = 0; i < AL; ++i) {
        const int m = bm + lrow + RPP * i;
        aok[i] = m < p.M;
        const int mm = aok[i] ? m : 0;
        if constexpr (AMODE == A_ROWS) {
            // the row number is fetched once per row and thread, here, ahead of the K loop; a number outside [0, n_rows) (the -1
            // padding of a table) makes a row of zeros and no address
            const int64_t r = p.rows[mm];
            aok[i] = aok[i] && r >= 0 && r < p.n_rows;
            aptr[i] = p.A + (aok[i] ? (size_t)r * (size_t)p.lda : (size_t)0) + lc4;
        } else if (AMODE == A_PLAIN) {
            aptr[i] = p.A + (size_t)mm * p.lda + lc4;
        } else {
            const int f2 = mm % p.F2;
            const int bt = mm / p.F2;
            const int t2 = bt % p.T2;
            const int b = bt / p.T2;
            aptr[i] = p.A + (((size_t)b * p.T1 + S * t2) * p.F1 + S * f2) * p.Cc + lc4;
        }
    }
    const float* wptr[WL];
    bool wok[WL];
#pragma unroll
    for (int i = 0; i < WL; ++i) {
        const int n = bn + lrow + RPP * i;
        wok[i] = n < p.N;
        wptr[i] = p.W + (size_t)(wok[i] ? n : 0) * p.K + lc4;
    }

    f32x4 areg[AL], wreg[WL];
    auto load_slab = [&](int kt) {
        size_t aoff;
        if constexpr (AMODE == A_ROWS) {
            aoff = (size_t)kt * BK;       // (the row is in aptr: only the source pointer differs from A_PLAIN)
        } else if (AMODE == A_PLAIN) {
            aoff = (size_t)kt * BK;
        } else {
            // K is ordered [channel block of 32][kh][kw][32 channels] (weights re-laid out at load): slab kt = window position
            // kt % KS^2 of channel block kt / KS^2
            const int cb = kt / (KS * KS), pos = kt - KS * KS * cb;
            const int kh = pos / KS, kw = pos - KS * kh;
            aoff = ((size_t)kh * p.F1 + kw) * p.Cc + (size_t)cb * BK;
        }
#pragma unroll
        for (int i = 0; i < AL; ++i)
            areg[i] = aok[i] ? *reinterpret_cast<const f32x4*>(aptr[i] + aoff) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < WL; ++i)
            wreg[i] = wok[i] ? *reinterpret_cast<const f32x4*>(wptr[i] + (size_t)kt * BK) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto store_slab = [&](int buf) {
#pragma unroll
        for (int i = 0; i < AL; ++i)
            *reinterpret_cast<f32x4*>(&As[(buf * BM + lrow + RPP * i) * LDP + lc4]) = areg[i];
#pragma unroll
        for (int i = 0; i < WL; ++i)
            *reinterpret_cast<f32x4*>(&Ws[(buf * BN + lrow + RPP * i) * LDP + lc4]) = wreg[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int n = 0; n < TN; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    const int kt_lo = EPI == EPI_SPLITK ? (int)blockIdx.y * p.ksplit : 0;
    const int KT = EPI == EPI_SPLITK ? min(kt_lo + p.ksplit, p.K / BK) : p.K / BK;
    load_slab(kt_lo);
    store_slab(0);
    __syncthreads();

    const int frow = lane & 31;
    const int fcol = (lane >> 5) * 4;
    for (int kt = kt_lo; kt < KT; ++kt) {
        const int buf = (kt - kt_lo) & 1;
        if (kt + 1 < KT) load_slab(kt + 1);
        __builtin_amdgcn_sched_barrier(0);       // the loads stay ahead of this slab's MFMAs (the scheduler would sink them)
        const float* Ab = &As[(buf * BM + wm * (BM / WM) + frow) * LDP + fcol];
        const float* Wb = &Ws[(buf * BN + wn * (BN / WN) + frow) * LDP + fcol];
#pragma unroll
        for (int g = 0; g < BK / 8; ++g) {
            f32x4 af[TM], wf[TN];
#pragma unroll
            for (int m = 0; m < TM; ++m) af[m] = *reinterpret_cast<const f32x4*>(Ab + m * 32 * LDP + g * 8);
#pragma unroll
            for (int n = 0; n < TN; ++n) wf[n] = *reinterpret_cast<const f32x4*>(Wb + n * 32 * LDP + g * 8);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int m = 0; m < TM; ++m)
#pragma unroll
                    for (int n = 0; n < TN; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m][s], wf[n][s], acc[m][n], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < KT) store_slab(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue ---------------------------------------------------------------------------
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
    const int ccol = lane & 31;
    const int rbase = 4 * (lane >> 5);
    if (EPI == EPI_SPLITK) {
        float* cp = p.C + (size_t)blockIdx.y * p.M * p.ldc;
#pragma unroll
        for (int n = 0; n < TN; ++n) {
            const int col = bn + wn * (BN / WN) + n * 32 + ccol;
            if (col >= p.N) continue;
#pragma unroll
            for (int m = 0; m < TM; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = bm + wm * (BM / WM) + m * 32 + (r & 3) + 8 * (r >> 2) + rbase;
                    if (row < p.M) cp[(size_t)row * p.ldc + col] = acc[m][n][r];
                }
        }
    }
    if (EPI == EPI_STD || EPI == EPI_ACT) {   // EPI_ACT: EPI_STD with the activations behind ACT_SILU (instantiations of their own:
                                              // the product launches keep the code they had)
#pragma unroll
        for (int n = 0; n < TN; ++n) {
            const int col = bn + wn * (BN / WN) + n * 32 + ccol;
            if (col >= p.N) continue;
            const float bv = p.bias ? p.bias[col] : 0.f;
#pragma unroll
            for (int m = 0; m < TM; ++m) {
                float res[16];   // residual loads before the stores (R may alias C)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = min(bm + wm * (BM / WM) + m * 32 + (r & 3) + 8 * (r >> 2) + rbase, p.M - 1);
                    res[r] = p.R ? p.R[(size_t)row * p.ldr + col] : 0.f;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = bm + wm * (BM / WM) + m * 32 + (r & 3) + 8 * (r >> 2) + rbase;
                    float v = acc[m][n][r] + (p.bias_after_alpha ? 0.f : bv);
                    if (p.act == ACT_RELU) v = fmaxf(v, 0.f);
                    else if (p.act == ACT_SILU) v = silu_f(v);
                    else if (EPI == EPI_ACT) v = act_f(p.act, v);       // gelu / tanh / hardtanh / selu: act is uniform, a scalar branch
                    if (p.mask_tp > 0) {
                        const int rc = min(row, p.M - 1);
                        const int b = rc / p.mask_tp, t = rc - b * p.mask_tp;
                        if (4 * t >= p.lens[b]) v = 0.f;
                    }
                    v = res[r] + v * p.alpha + (p.bias_after_alpha ? bv : 0.f);
                    if (row < p.M) p.C[(size_t)row * p.ldc + col] = v;
                }
            }
        }
    }
}

// Offline conv2 on full-width row blocks (N = 256): a workgroup owns 64 output rows x all 256 channels, 8 waves, wave w the
// columns 32w .. 32w+31 of all 64 rows (two 32x32 accumulators).  The implicit-GEMM A slab (64 rows x 32 k) is gathered ONCE per
// block into double-buffered LDS (one dwordx4 load + one ds_write_b128 per thread and slab, one barrier per slab) and shared by all
// 8 waves; the 128x128-tile launch staged every A element twice (once per column tile) and every weight element through LDS.  The
// weights come from a packed copy in consumption order (launch_pack_conv2_rows: [wave][kt][g][lane][4]) through raw buffer loads
// straight into MFMA operand registers, a ring of RB_RING fragments (two slabs ahead); each 1 KB fragment feeds 8 MFMAs (4 k steps
// x 2 row tiles).  Per 32 MFMAs and wave: 2 staging + 8 A fragment reads + 4 weight loads (the 128x128 tile: 8 + 12).
// 92 VGPRs and 18 KB of LDS: two workgroups per CU.  (Two slabs per barrier, 36 KB of LDS: 1 412 against 1 375 us; not kept.)
// Bit-identical to gemm_f32_kernel: every output element sees the same MFMA chain (kt -> g -> s, k = 8g + s and 8g + 4 + s in
// MFMA s) from zero, then the same epilogue.
//
// A operand modes (template AM):
// * RB_X1: the implicit-GEMM gather from the conv1 output x1 [B, T1, F1, 256] (written by conv1_kernel, elementwise.hip), or
//   from any channels-last [B, T1, F1, 256] activation: KS x KS window at stride S (template <KS, S>: <3, 2> for conv2 and
//   conv2d8's third conv, <5, 3> for conv2d6's second conv), slab kt = window position kt % KS^2 of channel block kt / KS^2.
// * RB_FUSED (masr_debug_set key 41): conv1 is computed in the gather, and x1 never exists.  At block start the CMVN-normalised
//   7 x 7 feature patch of every row (frames 4 t2 .. 4 t2 + 6, mel bins 4 f2 .. 4 f2 + 6) and the conv1 weights + bias go to LDS
//   (12.25 + 10 KB).  Thread (row lrow, channels 32 cb + lc4 .. + 3) computes slab (cb, kh, kw) as the conv1 output at
//   t1 = 2 t2 + kh, f1 = 2 f2 + kw: bias, then 9 fmaf in conv1_kernel's tap order, then ReLU, so every value is bit-identical to
//   conv1_kernel's.  Its taps are spread over the MFMA groups of the slab before (LDS reads ahead of the group's MFMAs, the fmaf
//   behind them), and one ds_write_b128 replaces the global load.
// * RB_PLAIN: row-major A (lda), K split into gridDim.y ranges of p.ksplit slabs, raw partials stored as EPI_SPLITK
//   (splitk_reduce_kernel applies the epilogue): the offline embed projection (masr_debug_set key 42).
static constexpr int RB_BM = 64;
static constexpr int RB_N = 256;
static constexpr int RB_RING = 8;
static constexpr int RB_PP = 49;     // RB_FUSED: 7 x 7 feature patch per row (odd pitch: the 8 rows of a wave on 8 banks)
enum { RB_X1 = 0, RB_FUSED = 1, RB_PLAIN = 2 };

__device__ __forceinline__ f32x4 rb_bufld(__amdgpu_buffer_rsrc_t rs, unsigned lane16, unsigned frag) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, lane16, frag * 1024u, 0));
}

// RB_FUSED: first conv1 tap of MFMA group g (taps [rb_tap(g), rb_tap(g + 1)) follow group g's MFMAs)
__device__ constexpr int rb_tap(int g) { return g == 0 ? 0 : g == 1 ? 2 : g == 2 ? 4 : g == 3 ? 6 : 9; }

template <int AM, int KS = 3, int S = 2>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void conv2_rows_kernel(GemmArgs p) {
    static_assert(AM != RB_FUSED || (KS == 3 && S == 2), "conv1 in the gather: 3x3 stride 2 only");
    constexpr int XS = AM == RB_FUSED ? 10 * RB_N + RB_BM * RB_PP : 4;      // conv1 weights [9][256] + bias [256], patches [64][49]
    __shared__ __align__(16) float As[2][RB_BM * LDP];
    __shared__ __align__(16) float Xs[XS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbm = (p.M + RB_BM - 1) / RB_BM;
    int bid = blockIdx.x;
    if (p.skip_rps <= 0) {          // XCD-aware block order as in gemm_f32_kernel
        const int q = nbm / 8, r = nbm % 8, xcd = bid % 8, idx = bid / 8;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int bm = bid * RB_BM;
    if (p.skip_rps > 0 && p.lens) {         // a block of padded frames only (whole workgroup, before any barrier)
        const int span = min(bm + RB_BM, p.M) - 1 - bm;
        const int b0 = bm / p.skip_rps, r0 = bm - b0 * p.skip_rps;
        if (r0 + span < p.skip_rps && 4 * (r0 / p.skip_div) >= p.lens[b0]) return;
    }
    const int KT = p.K / BK;
    const int kt_lo = AM == RB_PLAIN ? (int)blockIdx.y * p.ksplit : 0;
    const int kt_hi = AM == RB_PLAIN ? min(kt_lo + p.ksplit, KT) : KT;

    // ---- A gather: thread = (row tid >> 3, 4 k values), one float4 per slab ----------------------------------------------
    const int lrow = tid >> 3, lc4 = (tid & 7) * 4;
    const float* aptr = nullptr;
    const bool aok = bm + lrow < p.M;
    if (AM == RB_X1) {
        const int mm = aok ? bm + lrow : 0;
        const int f2 = mm % p.F2, bt = mm / p.F2, t2 = bt % p.T2, b = bt / p.T2;
        aptr = p.A + (((size_t)b * p.T1 + S * t2) * p.F1 + S * f2) * p.Cc + lc4;
    } else if (AM == RB_PLAIN) {
        aptr = p.A + (size_t)(aok ? bm + lrow : 0) * p.lda + lc4;
    }
    auto load_a = [&](int kt) -> f32x4 {
        size_t aoff;
        if (AM == RB_PLAIN) {
            aoff = (size_t)kt * BK;
        } else {
            const int cb = kt / (KS * KS), pos = kt - KS * KS * cb;       // K order [channel block of 32][kh][kw][32 channels]
            const int kh = pos / KS, kw = pos - KS * kh;
            aoff = ((size_t)kh * p.F1 + kw) * p.Cc + (size_t)cb * BK;
        }
        return aok ? *reinterpret_cast<const f32x4*>(aptr + aoff) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    float* const adst = &As[0][lrow * LDP + lc4];

    // ---- weights: fragment (kt, g) of wave w at ((w * KT + kt) * 4 + g) KB -----------------------------------------------
    const __amdgpu_buffer_rsrc_t wrs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.Wp), 0, RB_N * p.K * (int)sizeof(float), 0x00020000);
    const unsigned lane16 = lane * 16;
    const unsigned wfrag0 = (unsigned)(wave * KT) * 4u;
    auto bld = [&](int kt, int g) -> f32x4 { return rb_bufld(wrs, lane16, wfrag0 + (unsigned)min(kt, KT - 1) * 4u + g); };

    f32x4 pre[RB_RING];
#pragma unroll
    for (int i = 0; i < RB_RING; ++i) pre[i] = bld(kt_lo + (i >> 2), i & 3);
    __builtin_amdgcn_sched_barrier(0);       // (RB_FUSED: issued ahead of the staging loads)

    // ---- RB_FUSED: conv1 weights and the rows' feature patches in LDS ----------------------------------------------------
    // (rows >= M take row M - 1's patch: defined values, never stored)
    const float* const w1s = Xs;                        // [10][256]: taps 0..8, bias
    const float* const xrow = Xs + 10 * RB_N + lrow * RB_PP;
    if (AM == RB_FUSED) {
        for (int i = tid; i < 9 * RB_N; i += 512) Xs[i] = p.c1w[i];
        if (tid < RB_N) Xs[9 * RB_N + tid] = p.c1b[tid];
        // the 8 threads of row lrow stage its patch (one row decomposition per thread)
        const int m = min(bm + lrow, p.M - 1);
        const int f2 = m % p.F2, bt = m / p.F2, t2 = bt % p.T2, b = bt / p.T2;
        const float* src = p.feats + ((size_t)b * p.Tin + 4 * t2) * p.Fin + 4 * f2;
        for (int q = tid & 7; q < RB_PP; q += 8) {
            const int dt = q / 7, df = q - 7 * dt, f = 4 * f2 + df;
            Xs[10 * RB_N + lrow * RB_PP + q] = (src[dt * p.Fin + df] - p.mean[f]) * p.istd[f];
        }
    }
    // conv1 taps [t0, t1) of slab kt into c (tap = 3 kh' + kw': feature (2 kh + kh', 2 kw + kw') of the row's patch); the LDS
    // reads (rd) and the fmaf (fma) are separate so that the reads can be issued ahead of an MFMA group
    auto c1_rd = [&](int kt, int t, f32x4& w, float& x) {
        const int cb = kt / 9, pos = kt - 9 * cb, kh = pos / 3, kw = pos - 3 * kh;
        x = xrow[2 * kh * 7 + 2 * kw + (t / 3) * 7 + t % 3];
        w = *reinterpret_cast<const f32x4*>(w1s + t * RB_N + 32 * cb + lc4);
    };
    auto c1_fma = [&](f32x4& c, const f32x4& w, float x) {
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = fmaf(w[q], x, c[q]);
    };
    auto c1_bias = [&](int kt) -> f32x4 { return *reinterpret_cast<const f32x4*>(w1s + 9 * RB_N + 32 * (kt / 9) + lc4); };
    auto c1_relu = [&](f32x4& c) {
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = fmaxf(c[q], 0.f);
    };

    if (AM == RB_FUSED) {       // slab 0 (the weight ring loads in flight behind the staging)
        __syncthreads();
        f32x4 c = c1_bias(0);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            f32x4 w;
            float x;
            c1_rd(0, t, w, x);
            c1_fma(c, w, x);
        }
        c1_relu(c);
        *reinterpret_cast<f32x4*>(adst) = c;
    }
    f32x16 acc[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

    if (AM != RB_FUSED) *reinterpret_cast<f32x4*>(adst) = load_a(kt_lo);
    __syncthreads();

    const int frow = lane & 31, fcol = (lane >> 5) * 4;
    const float* afrag = &As[0][frow * LDP + fcol];
    for (int kt0 = kt_lo; kt0 < kt_hi; kt0 += 2) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {           // slab kt = kt0 + j lives in LDS buffer j, its fragments in ring slots 4j .. 4j+3
            const int kt = kt0 + j;
            if (j == 1 && kt >= kt_hi) break;
            const bool next = kt + 1 < kt_hi;
            const int ktn = min(kt + 1, kt_hi - 1);     // RB_FUSED: the slab computed behind this one's MFMAs
            f32x4 areg;
            if (AM == RB_FUSED) areg = c1_bias(ktn);
            else if (next) areg = load_a(kt + 1);
            const float* Ab = afrag + j * RB_BM * LDP;
            f32x4 af[2] = {*reinterpret_cast<const f32x4*>(Ab), *reinterpret_cast<const f32x4*>(Ab + 32 * LDP)};
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < BK / 8; ++g) {
                f32x4 an[2];
                if (g + 1 < BK / 8) {
                    an[0] = *reinterpret_cast<const f32x4*>(Ab + (g + 1) * 8);
                    an[1] = *reinterpret_cast<const f32x4*>(Ab + 32 * LDP + (g + 1) * 8);
                }
                constexpr int NTAP = 3;
                f32x4 cw[NTAP];
                float cx[NTAP];
                if (AM == RB_FUSED) {
#pragma unroll
                    for (int t = rb_tap(g); t < rb_tap(g + 1); ++t) c1_rd(ktn, t, cw[t - rb_tap(g)], cx[t - rb_tap(g)]);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int m = 0; m < 2; ++m)
                        acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m][s], pre[4 * j + g][s], acc[m], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                pre[4 * j + g] = bld(kt + 2, g);
                __builtin_amdgcn_sched_barrier(0);
                if (AM == RB_FUSED) {
#pragma unroll
                    for (int t = rb_tap(g); t < rb_tap(g + 1); ++t) c1_fma(areg, cw[t - rb_tap(g)], cx[t - rb_tap(g)]);
                }
                if (g + 1 < BK / 8) {
                    af[0] = an[0];
                    af[1] = an[1];
                }
            }
            if (AM == RB_FUSED) c1_relu(areg);
            if (next) *reinterpret_cast<f32x4*>(adst + (j ^ 1) * RB_BM * LDP) = areg;
            __syncthreads();
        }
    }

    const int ccol = lane & 31;
    const int rbase = 4 * (lane >> 5);
    const int col = wave * 32 + ccol;
    if (AM == RB_PLAIN) {       // ---- raw partial of K range blockIdx.y (gemm_f32_kernel EPI_SPLITK) ----------------------
        float* cp = p.C + (size_t)blockIdx.y * p.M * p.ldc;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = bm + m * 32 + (r & 3) + 8 * (r >> 2) + rbase;
                if (row < p.M) cp[(size_t)row * p.ldc + col] = acc[m][r];
            }
        return;
    }
    // ---- epilogue (gemm_f32_kernel EPI_STD with TM = 2, TN = 1) ---------------------------------------------------------
    const float bv = p.bias ? p.bias[col] : 0.f;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        float res[16];   // residual loads before the stores (R may alias C)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = min(bm + m * 32 + (r & 3) + 8 * (r >> 2) + rbase, p.M - 1);
            res[r] = p.R ? p.R[(size_t)row * p.ldr + col] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = bm + m * 32 + (r & 3) + 8 * (r >> 2) + rbase;
            float v = acc[m][r] + (p.bias_after_alpha ? 0.f : bv);
            if (p.act == ACT_RELU) v = fmaxf(v, 0.f);
            else if (p.act == ACT_SILU) v = silu_f(v);
            if (p.mask_tp > 0) {
                const int rc = min(row, p.M - 1);
                const int b = rc / p.mask_tp, t = rc - b * p.mask_tp;
                if (4 * t >= p.lens[b]) v = 0.f;
            }
            v = res[r] + v * p.alpha + (p.bias_after_alpha ? bv : 0.f);
            if (row < p.M) p.C[(size_t)row * p.ldc + col] = v;
        }
    }
}

// W [256, K] (K order of the implicit GEMM, any window: K = KS^2 * 256 or a plain K) -> conv2_rows_kernel's layout [wave][kt][g][lane][4]:
//   P = W[32 wave + (lane & 31)][32 kt + 8 g + 4 (lane >> 5) + q]
__global__ __launch_bounds__(256) void pack_conv2_rows_kernel(const float* __restrict__ w, float* __restrict__ p, int K) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)RB_N * K) return;
    const int KT = K / BK;
    const int q = (int)(e & 3), lane = (int)((e >> 2) & 63);
    const size_t frag = e >> 8;
    const int g = (int)(frag & 3), kt = (int)((frag >> 2) % KT), wave = (int)((frag >> 2) / KT);
    p[e] = w[(size_t)(32 * wave + (lane & 31)) * K + kt * BK + 8 * g + 4 * (lane >> 5) + q];
}
void launch_pack_conv2_rows(const float* w, float* p, int K, hipStream_t s) {
    const size_t n = (size_t)RB_N * K;
    hipLaunchKernelGGL(pack_conv2_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, p, K);
}

template <int BM, int BN, int WM, int WN, int AMODE, int EPI>
static void launch_t(const GemmArgs& a, hipStream_t s) {
    const int nbm = (a.M + BM - 1) / BM, nbn = (a.N + BN - 1) / BN;
    const size_t lds = (size_t)2 * (BM + BN) * LDP * sizeof(float);
    auto k = gemm_f32_kernel<BM, BN, WM, WN, AMODE, EPI>;
    static LdsAttr attr;
    ensure_dynamic_lds(reinterpret_cast<const void*>(k), lds, attr);
    hipLaunchKernelGGL(k, dim3(nbm * nbn, EPI == EPI_SPLITK ? a.nsplit : 1), dim3(64 * WM * WN), lds, s, a);
}

// out = R + alpha * act(sum_s partial[s] + bias) [+ bias after alpha]; partials added in ascending s (deterministic)
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmArgs p, const float* __restrict__ partial, float* out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)p.M * p.N) return;
    const int row = (int)(i / p.N), col = (int)(i - (size_t)row * p.N);
    float acc = 0.f;
    for (int sp = 0; sp < p.nsplit; ++sp) acc += partial[((size_t)sp * p.M + row) * p.N + col];
    const float bv = p.bias ? p.bias[col] : 0.f;
    float v = acc + (p.bias_after_alpha ? 0.f : bv);
    if (p.act == ACT_RELU) v = fmaxf(v, 0.f);
    else if (p.act == ACT_SILU) v = silu_f(v);
    const float r = p.R ? p.R[(size_t)row * p.ldr + col] : 0.f;
    out[(size_t)row * p.ldc + col] = r + v * p.alpha + (p.bias_after_alpha ? bv : 0.f);
}

// the conv2 tile choice of launch_gemm below (A_CONV2, EPI_STD): few rows -> 64x64, a thin last round -> 64x128, else 128x128
// tiles or, given a.Wp, the row blocks
static int conv2_tiles(const GemmArgs& a) {
    // few output rows (streaming chunk steps): 64x64 tiles so that the grid still covers the chip
    const long t128c = (long)((a.M + 127) / 128) * ((a.N + 127) / 128);
    // mid sizes (the 128-stream chunk step: 608 tiles of 128x128 on 512 resident slots = two rounds, the second at 19 %):
    // 128x64 tiles (four waves, the tile count doubles) when the last round of the 128x128 grid would be under conv2_mid_fill
    // percent full (masr_debug_set key 33; 0 = never)
    const long rounds = (t128c + 511) / 512;
    const int mid_fill = knobs().conv2_mid_fill;
    const bool thin_tail = mid_fill > 0 && t128c >= 200 && t128c <= 1024 &&
                           (t128c - (rounds - 1) * 512) * 100 < (long)mid_fill * 512;
    if (t128c < 200) return 64;
    if (thin_tail) return 128;
    return a.Wp && a.N == RB_N && a.K % BK == 0 ? 0 : 256;
}
bool gemm_conv2_rows(const GemmArgs& a) { return a.M > 0 && conv2_tiles(a) == 0; }

// Tile choice of the row-major EPI_STD launches (A_PLAIN, its EPI_ACT twin and A_ROWS): fill >= 256 CUs.  128x128 when that already
// yields enough workgroups, otherwise 64x128 / 64x64 (N = 256 projections at M = B*T' ~ 8k rows).  -> the tile's BM + BN
static int std_tiles(const GemmArgs& a) {
    const long t128 = (long)((a.M + 127) / 128) * ((a.N + 127) / 128);
    const long t64 = (long)((a.M + 63) / 64) * ((a.N + 127) / 128);
    return t128 >= 384 ? 256 : t64 >= 200 ? 192 : 128;
}

void launch_gemm(const GemmArgs& a, int amode, int epi, hipStream_t s) {
    if (a.M <= 0 || a.N <= 0) return;
    if (a.act > ACT_SILU) {       // gelu / tanh / hardtanh / selu: the plain tiled launch only (wide_ffn, masr_op_gemm)
        if (amode != A_PLAIN || epi != EPI_STD || a.act > ACT_SELU) {
            note_launch_error("launch_gemm: an activation behind silu runs on the plain tiled launch only", hipErrorInvalidValue);
            return;
        }
        const int tiles = std_tiles(a);
        if (tiles == 256) launch_t<128, 128, 2, 2, A_PLAIN, EPI_ACT>(a, s);
        else if (tiles == 192) launch_t<64, 128, 2, 2, A_PLAIN, EPI_ACT>(a, s);
        else launch_t<64, 64, 2, 2, A_PLAIN, EPI_ACT>(a, s);
        return;
    }
    if (amode == A_ROWS) {        // row-table A (GemmArgs::rows): instantiations of their own, A_PLAIN's tile at the same (M, N)
        if (epi != EPI_STD || !a.rows || a.n_rows <= 0 || a.K % BK) {
            note_launch_error("launch_gemm: the row-table A operand takes EPI_STD, a table, n_rows > 0 and K a multiple of 32",
                              hipErrorInvalidValue);
            return;
        }
        const int tiles = std_tiles(a);
        if (tiles == 256) launch_t<128, 128, 2, 2, A_ROWS, EPI_STD>(a, s);
        else if (tiles == 192) launch_t<64, 128, 2, 2, A_ROWS, EPI_STD>(a, s);
        else launch_t<64, 64, 2, 2, A_ROWS, EPI_STD>(a, s);
        return;
    }
    if (amode == A_CONV2 && epi == EPI_SPLITK) {      // caller set a.C = partial buffer, a.nsplit, a.ksplit
        launch_t<64, 64, 2, 2, A_CONV2, EPI_SPLITK>(a, s);
        return;
    }
    if (amode == A_CONV5) {       // conv2d6's 5x5 stride-3 conv: the conv2 launch shapes with the wider window (never conv1 in the gather)
        if (epi == EPI_SPLITK) launch_t<64, 64, 2, 2, A_CONV5, EPI_SPLITK>(a, s);
        else if (conv2_tiles(a) == 64) launch_t<64, 64, 2, 2, A_CONV5, EPI_STD>(a, s);
        else if (conv2_tiles(a) == 128) launch_t<64, 128, 2, 2, A_CONV5, EPI_STD>(a, s);
        else if (conv2_tiles(a) == 0)
            hipLaunchKernelGGL((conv2_rows_kernel<RB_X1, 5, 3>), dim3((unsigned)((a.M + RB_BM - 1) / RB_BM)), dim3(512), 0, s, a);
        else launch_t<128, 128, 2, 4, A_CONV5, EPI_STD>(a, s);
        return;
    }
    if (amode == A_CONV2) {
        const int tiles = conv2_tiles(a);
        if (tiles == 64) launch_t<64, 64, 2, 2, A_CONV2, EPI_STD>(a, s);
        else if (tiles == 128) launch_t<64, 128, 2, 2, A_CONV2, EPI_STD>(a, s);
        // 8 waves (2 x 4 grid, 64 x 32 per wave) on the 128x128 tile: two workgroups per CU = four waves per SIMD cover each
        // other's slab barriers; 1 494 -> 1 457 us at B = 32 x 10 s by HIP events.  (4 x 2 grid: 1 488 us; 16 waves as a 4 x 4 grid: 1 624 us; 128x256 /
        // 256x128 tiles with 8 waves, one workgroup per CU: 1 540 us.)
        // full-width 64-row blocks with packed weights in registers when the caller supplies the packed copy (a.Wp: offline conv2,
        // masr_debug_set key 40), conv1 computed in the gather when it supplies the features (a.feats: masr_debug_set key 41)
        else if (a.Wp && a.N == RB_N && a.K % BK == 0) {
            const dim3 grid((unsigned)((a.M + RB_BM - 1) / RB_BM));
            if (a.feats) hipLaunchKernelGGL(conv2_rows_kernel<RB_FUSED>, grid, dim3(512), 0, s, a);
            else hipLaunchKernelGGL(conv2_rows_kernel<RB_X1>, grid, dim3(512), 0, s, a);
        } else if (knobs().gemm_waves == 8) launch_t<128, 128, 2, 4, A_CONV2, EPI_STD>(a, s);
        else launch_t<128, 128, 2, 2, A_CONV2, EPI_STD>(a, s);
        return;
    }
    if (epi == EPI_SPLITK) {            // caller set a.C = partial buffer, a.nsplit, a.ksplit
        // full-width 64-row blocks with packed weights in registers when the caller supplies the packed copy (a.Wp: the offline
        // embed projection, masr_debug_set key 42)
        if (a.Wp && a.N == RB_N && a.K % BK == 0) {
            hipLaunchKernelGGL(conv2_rows_kernel<RB_PLAIN>, dim3((unsigned)((a.M + RB_BM - 1) / RB_BM), (unsigned)a.nsplit), dim3(512),
                               0, s, a);
            return;
        }
        // many rows (the offline embed projection: 248 tiles of 64x128 = one 4-wave workgroup per CU): the wide tile, so that
        // the split doubles the waves per SIMD instead of the LDS traffic per MFMA
        // (four waves: as a 2 x 4 grid of eight waves, 32 x 32 per wave, this launch is slower -- 183.6 vs 177.4 us in one
        // kernel trace, tools/gemm_waves_trace.py -- the LDS reads per MFMA double)
        if (a.nsplit >= 4 && (long)((a.M + 127) / 128) * ((a.N + 127) / 128) >= 100) launch_t<128, 128, 2, 4, A_PLAIN, EPI_SPLITK>(a, s);
        else if ((long)((a.M + 63) / 64) * ((a.N + 127) / 128) >= 200) launch_t<64, 128, 2, 2, A_PLAIN, EPI_SPLITK>(a, s);
        else launch_t<64, 64, 2, 2, A_PLAIN, EPI_SPLITK>(a, s);
        return;
    }
    const int tiles = std_tiles(a);
    if (tiles == 256) launch_t<128, 128, 2, 2, A_PLAIN, EPI_STD>(a, s);
    else if (tiles == 192) launch_t<64, 128, 2, 2, A_PLAIN, EPI_STD>(a, s);
    else launch_t<64, 64, 2, 2, A_PLAIN, EPI_STD>(a, s);
}

void launch_gemm_splitk(const GemmArgs& a, float* partial, int nsplit, hipStream_t s, int amode) {
    if (a.M <= 0 || a.N <= 0) return;
    GemmArgs b = a;
    const int kts = a.K / BK;
    b.ksplit = (kts + nsplit - 1) / nsplit;
    b.nsplit = (kts + b.ksplit - 1) / b.ksplit;          // every range owns at least one slab
    b.C = partial;
    b.ldc = a.N;
    launch_gemm(b, amode, EPI_SPLITK, s);
    GemmArgs r = a;
    r.nsplit = b.nsplit;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)(((size_t)a.M * a.N + 255) / 256)), dim3(256), 0, s, r, partial, a.C);
}

}  // namespace masr
