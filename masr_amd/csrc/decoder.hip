// Attention decoder of the second pass (decoder: attention_rescoring): the row kernels that the tiled GEMM and the LayerNorm row
// kernels do not cover.  Replaces, for the n-best prefixes of the CTC search, TransformerDecoder.forward of both halves of the
// reference's BiTransformerDecoder (masr/model_utils/transformer/decoder.py:188-231, DecoderLayer.forward :321-394) and the
// log_softmax + gather + sum of WeNet's attention_rescoring.
//
// Row space: sequence s = b * N + n (utterance b, hypothesis n) owns the Lp = Lmax + 1 rows s * Lp .. s * Lp + Lp - 1; row p is
// position p of the decoder input [sos, h_0 .. h_{L-1}] (left) or [sos, h_{L-1} .. h_0] (right).  Rows p > L are padding: the embed
// kernel zeroes them, the attention and scoring kernels never read or write them, and since every other launch is row-local (GEMM,
// LayerNorm) nothing a valid row holds depends on them -- nor on N, B or the other hypotheses of the table.
#include "common.h"

namespace masr {
namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// x[row] = emb[token] * sqrt(d) + pe[p]   (nn.Embedding + PositionalEncoding, conformer/embedding.py:52-66)
__global__ __launch_bounds__(64) void dec_embed_kernel(const int* __restrict__ hyp, const int* __restrict__ lens,
                                                       const float* __restrict__ emb, const float* __restrict__ pe,
                                                       float* __restrict__ x, int Lp, int Lmax, int d, int V, int reverse,
                                                       float scale) {
    const int row = blockIdx.x, s = row / Lp, p = row - s * Lp;
    const int L = clampi(lens[s], 0, Lmax);
    float4* xr = reinterpret_cast<float4*>(x + (size_t)row * d);
    if (p > L) {
        for (int c = threadIdx.x; c < d / 4; c += 64) xr[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    int tok = V - 1;                                                      // sos
    if (p > 0) tok = clampi(hyp[(size_t)s * Lmax + (reverse ? L - p : p - 1)], 0, V - 1);
    const float4* er = reinterpret_cast<const float4*>(emb + (size_t)tok * d);
    const float4* pr = reinterpret_cast<const float4*>(pe + (size_t)p * d);
    for (int c = threadIdx.x; c < d / 4; c += 64) {
        const float4 a = er[c], b = pr[c];
        xr[c] = make_float4(a.x * scale + b.x, a.y * scale + b.y, a.z * scale + b.z, a.w * scale + b.w);
    }
}

// Few-query attention, heads of 64: one wave per (query chunk of 64, head, sequence), one query per lane, the keys in sequence
// with a running maximum (every lane reads the same key / value row: the addresses are uniform over the wave).
//   causal = 1: self-attention over the sequence's own rows, key j <= query i   (subsequent_mask & pad mask, decoder.py:215-220)
//   causal = 0: source attention over the encoder frames of utterance s / N, keys j < key_lens[s / N]
struct DecAttArgs {
    const float* q;
    const float* k;
    const float* v;
    float* out;
    const int* hyp_lens;     // [S]
    const int* key_lens;     // [B] (causal = 0)
    int q_stride, kv_stride, out_stride;
    int Lp, Lmax, N, Tp, causal;
    float scale;
};

__global__ __launch_bounds__(64) void dec_attention_kernel(DecAttArgs a) {
    const int s = blockIdx.z, h = blockIdx.y, lane = threadIdx.x;
    const int nq = clampi(a.hyp_lens[s], 0, a.Lmax) + 1;
    const int i0 = blockIdx.x * 64;
    if (i0 >= nq) return;
    const int i = i0 + lane;
    const bool active = i < nq;
    size_t key0;
    int nk;
    if (a.causal) {
        key0 = (size_t)s * a.Lp;
        nk = min(nq, i0 + 64);
    } else {
        const int b = s / a.N;
        key0 = (size_t)b * a.Tp;
        nk = clampi(a.key_lens[b], 0, a.Tp);
    }
    float q[64], o[64];
    const size_t qrow = (size_t)s * a.Lp + (active ? i : i0);
    {
        const float4* qp = reinterpret_cast<const float4*>(a.q + qrow * a.q_stride + h * 64);
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const float4 t = qp[c];
            q[4 * c] = t.x; q[4 * c + 1] = t.y; q[4 * c + 2] = t.z; q[4 * c + 3] = t.w;
        }
#pragma unroll
        for (int c = 0; c < 64; ++c) o[c] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int j = 0; j < nk; ++j) {
        const float4* kp = reinterpret_cast<const float4*>(a.k + (key0 + j) * a.kv_stride + h * 64);
        const float4* vp = reinterpret_cast<const float4*>(a.v + (key0 + j) * a.kv_stride + h * 64);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const float4 t = kp[c];
            dot += q[4 * c] * t.x;
            dot += q[4 * c + 1] * t.y;
            dot += q[4 * c + 2] * t.z;
            dot += q[4 * c + 3] * t.w;
        }
        if (a.causal && j > i) continue;
        const float sc = dot * a.scale;
        const float mn = fmaxf(m, sc);
        const float f = expf(m - mn), pj = expf(sc - mn);
        l = l * f + pj;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const float4 t = vp[c];
            o[4 * c] = o[4 * c] * f + pj * t.x;
            o[4 * c + 1] = o[4 * c + 1] * f + pj * t.y;
            o[4 * c + 2] = o[4 * c + 2] * f + pj * t.z;
            o[4 * c + 3] = o[4 * c + 3] * f + pj * t.w;
        }
        m = mn;
    }
    if (!active) return;
    const float inv = l > 0.f ? 1.0f / l : 0.f;          // no visible key: the reference's masked softmax gives zeros
    float4* op = reinterpret_cast<float4*>(a.out + qrow * a.out_stride + h * 64);
#pragma unroll
    for (int c = 0; c < 16; ++c) op[c] = make_float4(o[4 * c] * inv, o[4 * c + 1] * inv, o[4 * c + 2] * inv, o[4 * c + 3] * inv);
}

__device__ __forceinline__ float wave_max(float v) {
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_add(float v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// rowlp[row] = log_softmax(logits[row])[target of the row]: one wave per valid row, the [rows, V] log-probabilities are never
// written.  Target of position p: the hypothesis' (left) or the reversed hypothesis' (right) token p, eos = V - 1 at p = L.
__global__ __launch_bounds__(64) void dec_row_score_kernel(const float* __restrict__ logits, const int* __restrict__ hyp,
                                                           const int* __restrict__ lens, float* __restrict__ rowlp, int Lp,
                                                           int Lmax, int V, int reverse) {
    const int row = blockIdx.x, s = row / Lp, p = row - s * Lp;
    const int L = clampi(lens[s], 0, Lmax);
    if (p > L) return;
    const int tgt = p < L ? clampi(hyp[(size_t)s * Lmax + (reverse ? L - 1 - p : p)], 0, V - 1) : V - 1;
    const float* x = logits + (size_t)row * V;
    float m = -INFINITY;
    for (int c = threadIdx.x; c < V; c += 64) m = fmaxf(m, x[c]);
    m = wave_max(m);
    float sum = 0.f;
    for (int c = threadIdx.x; c < V; c += 64) sum += expf(x[c] - m);
    sum = wave_add(sum);
    if (threadIdx.x == 0) rowlp[row] = (x[tgt] - m) - logf(sum);
}

// out[s] = sum of rowlp over positions 0 .. L in index order (one thread per sequence: the sum is the same whatever N or B is)
__global__ void dec_sum_kernel(const float* __restrict__ rowlp, const int* __restrict__ lens, float* __restrict__ out, int S,
                               int Lp, int Lmax) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int L = clampi(lens[s], 0, Lmax);
    float acc = 0.f;
    for (int p = 0; p <= L; ++p) acc += rowlp[(size_t)s * Lp + p];
    out[s] = acc;
}

}  // namespace

void launch_dec_embed(const int* hyp, const int* lens, const float* emb, const float* pe, float* x, int S, int Lmax, int d, int V,
                      int reverse, hipStream_t s) {
    if (S <= 0) return;
    const int Lp = Lmax + 1;
    hipLaunchKernelGGL(dec_embed_kernel, dim3((unsigned)(S * Lp)), dim3(64), 0, s, hyp, lens, emb, pe, x, Lp, Lmax, d, V, reverse,
                       sqrtf((float)d));
}

void launch_dec_attention(const float* q, int q_stride, const float* k, const float* v, int kv_stride, float* out, int out_stride,
                          const int* hyp_lens, const int* key_lens, int S, int N, int Lmax, int Tp, int heads, int causal,
                          hipStream_t s) {
    if (S <= 0) return;
    DecAttArgs a{};
    a.q = q; a.k = k; a.v = v; a.out = out; a.hyp_lens = hyp_lens; a.key_lens = key_lens;
    a.q_stride = q_stride; a.kv_stride = kv_stride; a.out_stride = out_stride;
    a.Lp = Lmax + 1; a.Lmax = Lmax; a.N = N; a.Tp = Tp; a.causal = causal;
    a.scale = 0.125f;                                   // 1 / sqrt(64)
    hipLaunchKernelGGL(dec_attention_kernel, dim3((unsigned)((a.Lp + 63) / 64), (unsigned)heads, (unsigned)S), dim3(64), 0, s, a);
}

void launch_dec_scores(const float* logits, const int* hyp, const int* lens, float* rowlp, float* out, int S, int Lmax, int V,
                       int reverse, hipStream_t s) {
    if (S <= 0) return;
    const int Lp = Lmax + 1;
    hipLaunchKernelGGL(dec_row_score_kernel, dim3((unsigned)(S * Lp)), dim3(64), 0, s, logits, hyp, lens, rowlp, Lp, Lmax, V, reverse);
    hipLaunchKernelGGL(dec_sum_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, s, rowlp, lens, out, S, Lp, Lmax);
}

}  // namespace masr
