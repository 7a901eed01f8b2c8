// Autoregressive beam search with the left attention decoder (decoder: attention; masr_attention_decode / masr_op_decoder_step):
// the kernels of ONE decode step that the tiled GEMM and the LayerNorm row kernel do not cover.  Replaces, per step, the reference's
// TransformerDecoder.forward_one_step (masr/model_utils/transformer/decoder.py:233-270) for the live hypotheses, and the top-k /
// mask_finished_* / merge of WeNet's attention decoding mode.
//
// Row space: row s = b * N + n is hypothesis rank n of utterance b.  Step i = 1, 2, ... handles decoder position p = i - 1 (input
// [sos, tokens...]): ONE new row per hypothesis.  Self-attention k | v of earlier positions are never recomputed and never copied
// when the beam is reordered: position j's row of rank r lives in slot (j, r) of the layer's cache [Lrun][S][2 d], and the
// ancestor table anc [S][Lcap] names, per hypothesis and position j < p, the rank whose slot holds ITS position j.  The merge
// kernel rewrites the token and ancestor tables (double-buffered: read `cur`, write `next`) through the parent index.
//
// Every launch here is per row or per utterance, with a fixed order of every sum: a hypothesis' figures do not depend on B, on the
// other utterances or on the padding of the encoder output.
#include "common.h"
#include "step_select.h"

namespace masr {
namespace {

__device__ __forceinline__ float wave_max(float v) {
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_add(float v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// x[s] = emb[last token of s] * sqrt(d) + pe[p]; the last token is sos = V - 1 at p = 0, else tok[s][p - 1]
// (rows of a frozen utterance read whatever the table holds there: the id is clamped, their results are never used)
__global__ __launch_bounds__(64) void step_embed_kernel(const int* __restrict__ tok, const float* __restrict__ emb,
                                                        const float* __restrict__ pe, float* __restrict__ x, int p, int Lcap,
                                                        int d, int V, float scale) {
    const int s = blockIdx.x;
    const int t = p == 0 ? V - 1 : clampi(tok[(size_t)s * Lcap + (p - 1)], 0, V - 1);
    const float4* er = reinterpret_cast<const float4*>(emb + (size_t)t * d);
    const float4* pr = reinterpret_cast<const float4*>(pe + (size_t)p * d);
    float4* xr = reinterpret_cast<float4*>(x + (size_t)s * d);
    for (int c = threadIdx.x; c < d / 4; c += 64) {
        const float4 a = er[c], b = pr[c];
        xr[c] = make_float4(a.x * scale + b.x, a.y * scale + b.y, a.z * scale + b.z, a.w * scale + b.w);
    }
}

// One-query attention, heads of 64: one wave per (hypothesis, head).  Lane l takes keys l, l + 64, ... with a running maximum, then
// the 64 (max, sum, accumulator) partials are merged with the usual rescale.  The split depends on the key count alone.
//   anc != nullptr: self-attention over positions 0 .. p; key j < p is row anc[s][j] of cache slab j, key p the row's own new k | v
//   anc == nullptr: source attention over the key_lens[s / N] encoder frames of utterance s / N (k | v rows [B * Tp])
struct StepAttArgs {
    const float* q;        // [S, q_stride]
    const float* kv;       // self: [Lrun][S][2 d]; source: [B * Tp][2 d]
    float* out;            // [S, d]
    const int* anc;        // [S, Lcap] or nullptr
    const int* key_lens;   // [B] (source)
    int q_stride, d, S, N, Tp, Lcap, p;
    float scale;
};

__global__ __launch_bounds__(64) void step_attention_kernel(StepAttArgs a) {
    const int s = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const int b = s / a.N, n = s - b * a.N;
    const int nk = a.anc ? a.p + 1 : clampi(a.key_lens[b], 0, a.Tp);
    float q[64], o[64];
    {
        const float4* qp = reinterpret_cast<const float4*>(a.q + (size_t)s * a.q_stride + h * 64);
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const float4 t = qp[c];
            q[4 * c] = t.x; q[4 * c + 1] = t.y; q[4 * c + 2] = t.z; q[4 * c + 3] = t.w;
        }
#pragma unroll
        for (int c = 0; c < 64; ++c) o[c] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int j = lane; j < nk; j += 64) {
        size_t row;
        if (a.anc) {
            const int r = j == a.p ? n : clampi(a.anc[(size_t)s * a.Lcap + j], 0, a.N - 1);
            row = (size_t)j * a.S + (size_t)b * a.N + r;
        } else {
            row = (size_t)b * a.Tp + j;
        }
        const float4* kp = reinterpret_cast<const float4*>(a.kv + row * (2 * a.d) + h * 64);
        const float4* vp = reinterpret_cast<const float4*>(a.kv + row * (2 * a.d) + a.d + h * 64);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const float4 t = kp[c];
            dot += q[4 * c] * t.x;
            dot += q[4 * c + 1] * t.y;
            dot += q[4 * c + 2] * t.z;
            dot += q[4 * c + 3] * t.w;
        }
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
    // merge over the lanes: a lane without a key holds m = -inf, l = 0 and contributes nothing
    const float mall = wave_max(m);
    const float f = (m == -INFINITY) ? 0.f : expf(m - mall);
    const float lall = wave_add(l * f);
    const float inv = lall > 0.f ? 1.0f / lall : 0.f;      // no visible key: the reference's masked softmax gives zeros
    float mine = 0.f;
#pragma unroll
    for (int c = 0; c < 64; ++c) {
        const float v = wave_add(o[c] * f);
        if (lane == c) mine = v;
    }
    a.out[(size_t)s * a.d + h * 64 + lane] = mine * inv;
}

// log_softmax of one logits row and its top-n, one workgroup of 256 per row: top_v / top_i [row][n] in the order above; the [S, V]
// log-probabilities are written only when `full` is given.  only_pos != nullptr (the teacher-forced op): a row writes its outputs
// at the step p == only_pos[row] alone.
__global__ __launch_bounds__(256) void step_topn_kernel(const float* __restrict__ logits, int V, int n, float* __restrict__ top_v,
                                                        int* __restrict__ top_i, float* __restrict__ full,
                                                        const int* __restrict__ only_pos, int p) {
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    __shared__ float red_s[4];
    const int row = blockIdx.x;
    if (only_pos && only_pos[row] != p) return;
    const float* x = logits + (size_t)row * V;
    float m = -INFINITY;
    for (int c = threadIdx.x; c < V; c += 256) m = fmaxf(m, x[c]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red_s[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red_s[0], red_s[1]), fmaxf(red_s[2], red_s[3]));
    __syncthreads();
    float sum = 0.f;
    for (int c = threadIdx.x; c < V; c += 256) sum += expf(x[c] - m);
    sum = wave_add(sum);
    if ((threadIdx.x & 63) == 0) red_s[threadIdx.x >> 6] = sum;
    __syncthreads();
    const float lse = logf((red_s[0] + red_s[1]) + (red_s[2] + red_s[3]));
    if (full)
        for (int c = threadIdx.x; c < V; c += 256) full[(size_t)row * V + c] = (x[c] - m) - lse;
    // n rounds: the first entry that comes strictly behind the previous winner
    float pv = 0.f;
    int pi = -1;
    for (int k = 0; k < n; ++k) {
        float bv = 0.f;
        int bi = -1;
        for (int c = threadIdx.x; c < V; c += 256) {
            const float v = (x[c] - m) - lse;
            if (v != v) continue;
            if (pi >= 0 && !before(pv, pi, v, c)) continue;
            if (bi < 0 || before(v, c, bv, bi)) {
                bv = v;
                bi = c;
            }
        }
        block_first(bv, bi, red_v, red_i);
        if (threadIdx.x == 0) {
            top_v[(size_t)row * n + k] = bi >= 0 ? bv : -INFINITY;
            top_i[(size_t)row * n + k] = bi >= 0 ? bi : V - 1;
        }
        if (bi < 0) {            // (a row with fewer than n comparable entries: NaN logits; the rest is -inf | eos)
            pv = -INFINITY;
            pi = V;
        } else {
            pv = bv;
            pi = bi;
        }
    }
}

// Beam merge of step i = p + 1, one workgroup of 256 per utterance: finished rows offer (0, eos), (-inf, eos), ...; the N best of
// the N x N sums score + logp, ties to the smaller flat index parent * N + candidate; scores, tokens and ancestors of the new
// ranks written to the `next` tables through the parent index.  An utterance past its limit copies its rows unchanged.
__global__ __launch_bounds__(256) void step_merge_kernel(StepMerge a) {
    __shared__ float cand[64 * 64];
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    __shared__ int parent[64], newtok[64], nfin;
    const int b = blockIdx.x, N = a.N, eos = a.V - 1, p = a.p;
    const size_t s0 = (size_t)b * N;
    const int lim = step_limit(a.enc_lens[b], a.Tp, a.max_len, a.max_pos, a.Lcap);
    const bool frozen = p + 1 > lim;
    if (threadIdx.x == 0) nfin = 0;
    if (!frozen) {
        for (int c = threadIdx.x; c < N * N; c += 256) {
            const int h = c / N, k = c - h * N;
            const bool fin = p > 0 && a.tok_cur[(s0 + h) * a.Lcap + (p - 1)] == eos;
            const float lp = fin ? (k == 0 ? 0.f : -INFINITY) : a.top_v[(s0 + h) * N + k];
            cand[c] = a.score_cur[s0 + h] + lp;
        }
        __syncthreads();
        float pv = 0.f;
        int pi = -1;
        for (int k = 0; k < N; ++k) {
            float bv = 0.f;
            int bi = -1;
            for (int c = threadIdx.x; c < N * N; c += 256) {
                const float v = cand[c];
                if (v != v) continue;
                if (pi >= 0 && !before(pv, pi, v, c)) continue;
                if (bi < 0 || before(v, c, bv, bi)) {
                    bv = v;
                    bi = c;
                }
            }
            block_first(bv, bi, red_v, red_i);
            if (bi < 0) {            // (NaN scores only: keep the row count with dead entries)
                bv = -INFINITY;
                bi = min(k, N * N - 1);
            }
            if (threadIdx.x == 0) {
                const int h = bi / N;
                const bool fin = p > 0 && a.tok_cur[(s0 + h) * a.Lcap + (p - 1)] == eos;
                const int t = fin ? eos : clampi(a.top_i[(s0 + h) * N + (bi - h * N)], 0, a.V - 1);
                parent[k] = h;
                newtok[k] = t;
                a.score_next[s0 + k] = bv;
                if (t == eos) nfin += 1;
            }
            pv = bv;
            pi = bi;
        }
    } else {
        for (int k = threadIdx.x; k < N; k += 256) {
            parent[k] = k;
            a.score_next[s0 + k] = a.score_cur[s0 + k];
        }
    }
    __syncthreads();
    // columns 0 .. p - 1 through the parent, column p: the new token | the parent's rank (whose slot holds position p)
    for (int c = threadIdx.x; c < N * (p + 1); c += 256) {
        const int k = c / (p + 1), j = c - k * (p + 1);
        const size_t src = (s0 + parent[k]) * a.Lcap + j, dst = (s0 + k) * a.Lcap + j;
        if (j < p) {
            a.tok_next[dst] = a.tok_cur[src];
            a.anc_next[dst] = a.anc_cur[src];
        } else {
            a.tok_next[dst] = frozen ? a.tok_cur[src] : newtok[k];
            a.anc_next[dst] = parent[k];
        }
    }
    if (threadIdx.x == 0 && !a.done[b] && (frozen || p + 1 == lim || nfin == N)) {
        a.done[b] = 1;
        atomicSub(a.active, 1);
    }
}

// scores = [0, -inf, ...] per utterance, done = 0, active = the utterances with at least one step to run
__global__ void step_init_kernel(float* score, int* done, int* active, const int* enc_lens, int B, int N, int Tp, int Lcap, int max_len,
                                 int max_pos) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * N) score[i] = (i % N == 0) ? 0.f : -INFINITY;
    if (i < B) {
        const bool none = step_limit(enc_lens[i], Tp, max_len, max_pos, Lcap) < 1;
        done[i] = none ? 1 : 0;
        if (!none) atomicAdd(active, 1);
    }
}

// The result: tokens after sos of every rank up to and excluding its first eos (eos from there to Lcap), that length, the score.
// `steps` columns were written; an utterance holds min(steps, its limit) of them.
__global__ __launch_bounds__(64) void step_result_kernel(const int* __restrict__ tok, const float* __restrict__ score,
                                                         const int* __restrict__ enc_lens, int* __restrict__ tokens_out,
                                                         int* __restrict__ lens_out, float* __restrict__ scores_out, int N, int Lcap,
                                                         int Tp, int V, int steps, int max_len, int max_pos) {
    const int s = blockIdx.x, b = s / N, eos = V - 1;
    const int have = min(steps, step_limit(enc_lens[b], Tp, max_len, max_pos, Lcap));
    int first = have;
    for (int j = threadIdx.x; j < have; j += 64)
        if (tok[(size_t)s * Lcap + j] == eos) first = min(first, j);
    for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off, 64));
    for (int j = threadIdx.x; j < Lcap; j += 64) tokens_out[(size_t)s * Lcap + j] = j < first ? tok[(size_t)s * Lcap + j] : eos;
    if (threadIdx.x == 0) {
        lens_out[s] = first;
        scores_out[s] = score[s];
    }
}

}  // namespace

void launch_step_embed(const int* tok, const float* emb, const float* pe, float* x, int S, int p, int Lcap, int d, int V,
                       hipStream_t s) {
    hipLaunchKernelGGL(step_embed_kernel, dim3((unsigned)S), dim3(64), 0, s, tok, emb, pe, x, p, Lcap, d, V, sqrtf((float)d));
}

void launch_step_attention(const float* q, int q_stride, const float* kv, float* out, const int* anc, const int* key_lens, int S,
                           int N, int Tp, int Lcap, int p, int d, int heads, hipStream_t s) {
    StepAttArgs a{};
    a.q = q; a.kv = kv; a.out = out; a.anc = anc; a.key_lens = key_lens;
    a.q_stride = q_stride; a.d = d; a.S = S; a.N = N; a.Tp = Tp; a.Lcap = Lcap; a.p = p;
    a.scale = 0.125f;                                   // 1 / sqrt(64)
    hipLaunchKernelGGL(step_attention_kernel, dim3((unsigned)S, (unsigned)heads), dim3(64), 0, s, a);
}

void launch_step_topn(const float* logits, int S, int V, int n, float* top_v, int* top_i, float* full, const int* only_pos, int p,
                      hipStream_t s) {
    hipLaunchKernelGGL(step_topn_kernel, dim3((unsigned)S), dim3(256), 0, s, logits, V, n, top_v, top_i, full, only_pos, p);
}

void launch_step_merge(const StepMerge& m, int B, hipStream_t s) {
    hipLaunchKernelGGL(step_merge_kernel, dim3((unsigned)B), dim3(256), 0, s, m);
}

void launch_step_init(float* score, int* done, int* active, const int* enc_lens, int B, int N, int Tp, int Lcap, int max_len,
                      int max_pos, hipStream_t s) {
    (void)hipMemsetAsync(active, 0, sizeof(int), s);
    hipLaunchKernelGGL(step_init_kernel, dim3((unsigned)((B * N + 255) / 256)), dim3(256), 0, s, score, done, active, enc_lens, B, N,
                       Tp, Lcap, max_len, max_pos);
}

void launch_step_result(const int* tok, const float* score, const int* enc_lens, int* tokens_out, int* lens_out, float* scores_out,
                        int S, int N, int Lcap, int Tp, int V, int steps, int max_len, int max_pos, hipStream_t s) {
    hipLaunchKernelGGL(step_result_kernel, dim3((unsigned)S), dim3(64), 0, s, tok, score, enc_lens, tokens_out, lens_out, scores_out,
                       N, Lcap, Tp, V, steps, max_len, max_pos);
}

}  // namespace masr
