// DeepSpeech2 with use_gru: True (reference masr/model_utils/deepspeech2/{encoder.py:21-28, gru.py}): nn.GRU(batch_first,
// 1 layer, uni- or bi-directional) over a packed sequence, PyTorch gate order r, z, n:
//   r = sigma(W_ir x + b_ir + W_hr h + b_hr),  z = sigma(W_iz x + b_iz + W_hz h + b_hz),
//   n = tanh(W_in x + b_in + r * (W_hn h + b_hn)),  h' = (1 - z) n + z h.
// As for the LSTM (lstm.hip), W_ih . x_t of ALL timesteps is one MFMA GEMM (gemm_f32.hip) whose bias is b_ih + [b_hr, b_hz, 0];
// b_hn sits inside the reset-gate product and comes to the step as its own [ndir][H] vector.  One launch per timestep, both
// directions in it (blockIdx.y).  pack_padded_sequence semantics: a sequence advances only while t < len (the reverse
// direction therefore starts at its own last frame), padded outputs are zero.  There is no cell state.
#include "common.h"

namespace masr {

static __device__ __forceinline__ float gsigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// gate epilogue of (sequence b, unit j): dot = W_h{r,z,n} . h_{t-1}
static __device__ __forceinline__ void gru_cell(const float* __restrict__ gx, const float* __restrict__ bhn,
                                                const float* __restrict__ h_prev, float* __restrict__ h_next,
                                                float* __restrict__ out, const int* __restrict__ lens, const float dot[3],
                                                int b, int j, int dir, int B, int T, int t, int ndir, int H) {
    const size_t sidx = ((size_t)dir * B + b) * H + j;
    const bool active = !lens || t < lens[b];
    const float* gr = gx + ((size_t)b * T + t) * (ndir * 3 * H) + (size_t)dir * 3 * H + j;
    const float h_old = h_prev[sidx];
    const float r = gsigm(gr[0] + dot[0]);
    const float z = gsigm(gr[H] + dot[1]);
    const float n = tanhf(gr[2 * H] + r * (dot[2] + bhn[dir * H + j]));
    const float h_new = (1.0f - z) * n + z * h_old;
    float* o = out + ((size_t)b * T + t) * (ndir * H) + dir * H + j;
    h_next[sidx] = active ? h_new : h_old;
    *o = active ? h_new : 0.f;
}

// Wave-per-unit form (B <= 4 and B > 32): a wave owns ONE hidden unit, its 3 gate rows of W_hh stay in registers (48 values
// per lane at rnn_size 1024, 3 H / 64 in general), and walks over the batch; H units / 4 waves = H / 4 workgroups per direction.
// H is instantiated for every multiple of 256 from 256 to 2048, as for the LSTM (lstm.hip).
template <int H>
__global__ __launch_bounds__(256) void gru_step_kernel(const float* __restrict__ gx, const float* __restrict__ whh,
                                                       const float* __restrict__ bhn, const float* __restrict__ h_prev,
                                                       float* __restrict__ h_next, float* __restrict__ out,
                                                       const int* __restrict__ lens, int B, int T, int step, int ndir) {
    constexpr int PL = H / 64;                      // W_hh values per lane and gate
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int dir = blockIdx.y;
    const int j = blockIdx.x * 4 + wave;
    const int t = dir ? T - 1 - step : step;
    float w[3][PL];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const float* wr = whh + ((size_t)dir * 3 * H + (size_t)g * H + j) * H + lane * PL;
#pragma unroll
        for (int k = 0; k < PL; k += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(wr + k);
            w[g][k] = v[0]; w[g][k + 1] = v[1]; w[g][k + 2] = v[2]; w[g][k + 3] = v[3];
        }
    }
    // the three dot products of (unit j, sequence b) end up in lane (b & 63); the epilogue runs once per 64 sequences
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int nb = min(64, B - b0);
        float mine[3] = {0.f, 0.f, 0.f};
        for (int bb = 0; bb < nb; ++bb) {
            const float* hp = h_prev + ((size_t)dir * B + b0 + bb) * H + lane * PL;
            float hv[PL];
#pragma unroll
            for (int k = 0; k < PL; k += 4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(hp + k);
                hv[k] = v[0]; hv[k + 1] = v[1]; hv[k + 2] = v[2]; hv[k + 3] = v[3];
            }
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < PL; ++k) a = fmaf(w[g][k], hv[k], a);
                a = wave_sum_dpp(a);
                if (lane == bb) mine[g] = a;
            }
        }
        if (lane < nb) gru_cell(gx, bhn, h_prev, h_next, out, lens, mine, b0 + lane, j, dir, B, T, t, ndir, H);
    }
}

// Matrix-core form (4 < B <= 32): U hidden units x 3 gates of a workgroup against the h_{t-1} rows of 16 * BT sequences
// (v_mfma_f32_16x16x4_f32: D[16 sequences, 16 columns] += h[16, 4] . W^T[4, 16]).  Column c of the workgroup's 3U columns is
// gate c / U of unit c % U, in NT = ceil(3U / 16) tiles of 16; U = 8 leaves the last 8 columns of the second tile empty (their
// lanes load nothing), U = 16 fills three tiles exactly but gives half as many workgroups, U = 4 is 12 columns of one tile and
// twice as many workgroups.  H / U workgroups per direction.  8 waves split K = H (H / 8 each, in steps of 16: H % 128 == 0),
// partial tiles are summed through LDS, then one thread per (sequence, unit) applies the gates.  Operand fetch as in
// lstm_step_mfma_kernel: 16-byte vectors along k, element i of every lane's vector feeds MFMA i of a group of four.
template <int H, int U, int BT>
__global__ __launch_bounds__(512) void gru_step_mfma_kernel(const float* __restrict__ gx, const float* __restrict__ whh,
                                                            const float* __restrict__ bhn, const float* __restrict__ h_prev,
                                                            float* __restrict__ h_next, float* __restrict__ out,
                                                            const int* __restrict__ lens, int B, int T, int step, int ndir) {
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    constexpr int NT = (3 * U + 15) / 16;
    __shared__ float red[8][BT * NT * 4][64];         // [wave][sequence tile, column tile, acc reg][lane]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int dir = blockIdx.y;
    const int j0 = blockIdx.x * U;
    const int t = dir ? T - 1 - step : step;
    const int col = lane & 15, q = lane >> 4;
    const int k0 = wave * (H / 8);
    f32x4v acc[BT][NT];
#pragma unroll
    for (int bt = 0; bt < BT; ++bt)
#pragma unroll
        for (int p = 0; p < NT; ++p) acc[bt][p] = f32x4v{0.f, 0.f, 0.f, 0.f};
    const float* wrow[NT];
    bool wok[NT];
#pragma unroll
    for (int p = 0; p < NT; ++p) {
        const int c = p * 16 + col, g = c / U;
        wok[p] = g < 3;
        wrow[p] = whh + ((size_t)dir * 3 * H + (size_t)min(g, 2) * H + j0 + c % U) * H + k0 + 4 * q;
    }
    const float* hbase = h_prev + (size_t)dir * B * H + k0 + 4 * q;
#pragma unroll
    for (int kb = 0; kb < H / 8; kb += 16) {
        f32x4 wv[NT], hv[BT];
#pragma unroll
        for (int p = 0; p < NT; ++p)
            wv[p] = wok[p] ? *reinterpret_cast<const f32x4*>(wrow[p] + kb) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int bt = 0; bt < BT; ++bt) {
            const int b = min(bt * 16 + col, B - 1);
            hv[bt] = *reinterpret_cast<const f32x4*>(hbase + (size_t)b * H + kb);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int bt = 0; bt < BT; ++bt)
#pragma unroll
                for (int p = 0; p < NT; ++p)
                    acc[bt][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[bt][i], wv[p][i], acc[bt][p], 0, 0, 0);
    }
#pragma unroll
    for (int bt = 0; bt < BT; ++bt)
#pragma unroll
        for (int p = 0; p < NT; ++p)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][(bt * NT + p) * 4 + r][lane] = acc[bt][p][r];
    __syncthreads();
    // D layout of the 16x16 tile: lane l, register r -> row (sequence) 4 * (l / 16) + r, column l % 16
    for (int e = threadIdx.x; e < BT * 16 * U; e += 512) {       // one thread per (sequence, unit)
        const int b = e / U, u = e % U;
        if (b >= B) continue;
        const int bt = b >> 4, r = b & 3, lq = (b >> 2) & 3;     // b = 16 bt + 4 lq + r
        float dot[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const int c = g * U + u;
            const int l = lq * 16 + (c & 15);
            float a = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) a += red[w][(bt * NT + (c >> 4)) * 4 + r][l];
            dot[g] = a;
        }
        gru_cell(gx, bhn, h_prev, h_next, out, lens, dot, b, j0 + u, dir, B, T, t, ndir, H);
    }
}

// masr_debug_set key 43 (knobs.h rnn_mfma_units): hidden units per workgroup of the matrix-core form; any value but 16 and -8 is 8
static int gru_units() {
    const int u = knobs().rnn_mfma_units;
    return u == 16 || u == -8 ? u : 8;
}

template <int H, int U>
static void launch_gru_mfma(const float* gx, const float* whh, const float* bhn, const float* h_prev, float* h_next, float* out,
                            const int* lens, int B, int T, int step, int ndir, hipStream_t s) {
    const dim3 grid(H / U, ndir), blk(512);
    if (B <= 16)
        hipLaunchKernelGGL((gru_step_mfma_kernel<H, U, 1>), grid, blk, 0, s, gx, whh, bhn, h_prev, h_next, out, lens, B, T, step, ndir);
    else
        hipLaunchKernelGGL((gru_step_mfma_kernel<H, U, 2>), grid, blk, 0, s, gx, whh, bhn, h_prev, h_next, out, lens, B, T, step, ndir);
}

template <int H>
static void launch_gru_step_h(const float* gx, const float* whh, const float* bhn, const float* h_prev, float* h_next, float* out,
                              const int* lens, int B, int T, int step, int ndir, hipStream_t s) {
    if (B > 4 && B <= 32) {           // matrix-core form: U units per workgroup, 16 * BT sequences
        if constexpr (H == 1024) {
            if (gru_units() == 16) return launch_gru_mfma<H, 16>(gx, whh, bhn, h_prev, h_next, out, lens, B, T, step, ndir, s);
        }
        if constexpr (H <= 512) {
            if (gru_units() != -8) return launch_gru_mfma<H, 4>(gx, whh, bhn, h_prev, h_next, out, lens, B, T, step, ndir, s);
        }
        return launch_gru_mfma<H, 8>(gx, whh, bhn, h_prev, h_next, out, lens, B, T, step, ndir, s);
    }
    hipLaunchKernelGGL(gru_step_kernel<H>, dim3(H / 4, ndir), dim3(256), 0, s, gx, whh, bhn, h_prev, h_next, out, lens, B, T,
                       step, ndir);
}

// 0: launched; 1: no step kernel is instantiated for this H (nothing was written)
int launch_gru_step(const float* gx, const float* whh, const float* bhn, const float* h_prev, float* h_next, float* out,
                    const int* lens, int B, int T, int H, int step, int ndir, hipStream_t s) {
    switch (H) {
#define MASR_GRU_H(N) case N: launch_gru_step_h<N>(gx, whh, bhn, h_prev, h_next, out, lens, B, T, step, ndir, s); return 0;
        MASR_GRU_H(256) MASR_GRU_H(512) MASR_GRU_H(768) MASR_GRU_H(1024)
        MASR_GRU_H(1280) MASR_GRU_H(1536) MASR_GRU_H(1792) MASR_GRU_H(2048)
#undef MASR_GRU_H
    }
    return 1;
}

}  // namespace masr
