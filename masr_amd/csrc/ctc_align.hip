// CTC forced alignment (masr_ctc_align): the Viterbi path of a hypothesis through the CTC trellis of its own utterance, and from it
// the first / last frame and the peak log-probability of every token.  The definition is the textbook one: extended label sequence
// blank, y1, blank, ..., yL, blank (S = 2 L + 1 states); a state is reached by staying, from s - 1, or -- an odd state whose label
// differs from the previous token's -- from s - 2; the path starts in state 0 or 1 and ends in state S - 1 or S - 2.
//
// Arithmetic (the contract the bit-exact tests pin; tests/ctc_align_ref.py restates it in numpy):
//   * log domain, float32 adds and compares only; MASR_ALIGN_NEG stands for "unreachable" (no infinities);
//   * the predecessor is taken in the order stay, s - 1, s - 2, a later one only if STRICTLY greater;
//   * at the end state S - 1 wins a tie against S - 2;
//   * peak = max over the token's frames of its log-probability (order-free).
//
// Mapping: one workgroup of 256 threads per utterance, states across the threads (a loop when S > 256), frames in sequence with one
// barrier each.  The two trellis rows, the hypothesis and the L + 1 log-probabilities a frame needs live in LDS; the gather of frame
// t + 1 is issued under the row update of frame t (double-buffered), so a frame reads L + 1 values of its V-wide row and nothing else.
// The predecessor choice (0 / 1 / 2) goes to the lane's workspace, one byte per state and frame; one thread walks it backwards into
// the start / end tables (LDS), then the tokens' peaks are taken in parallel, one thread per token over its own frames.
//
// Where frame t of utterance b lies is the one thing the two entry points differ in, and the kernel takes it as a template argument:
// DenseFrames -- row t of the utterance's own [T', V] block (masr_ctc_align); RowFrames -- row frame_row[b, t] of a shared
// [n_rows, V] matrix (masr_ctc_align_rows: the posterior history of a streaming session, whose rows are neither contiguous nor
// increasing).  The row number of a frame is one uniform load for the workgroup, fetched TWO frames ahead of its use: the gather of
// frame t + 1 finds its row pointer in a register, so the table adds nothing to the serial chain of the frame loop.  Row numbers
// are validated once, in front of the trellis (a number outside [0, n_rows) is status 2 and nothing of that utterance is read);
// every address from a row number is 64-bit.
#include <hip/hip_runtime.h>

#include <cstring>

#include "engine_state.h"

namespace masr {

constexpr int ALIGN_THREADS = 256;
constexpr int ALIGN_LMAX = MASR_ALIGN_MAX_TOKENS;       // LDS rows: S <= 2 * ALIGN_LMAX + 1
constexpr int ALIGN_SMAX = 2 * ALIGN_LMAX + 1;

template <int IS_LOG>
__device__ __forceinline__ float align_logp(float v) {
    if (IS_LOG) return v;
    return v > 0.f ? logf(v) : MASR_ALIGN_NEG;          // (a NaN probability is "not > 0" as well)
}

// frame t of utterance b -> its V-wide row
struct DenseFrames {
    const float* post;      // [B, T', V]
    int Tp, V;
    __device__ __forceinline__ void bind(int b) { post += (size_t)b * Tp * V; }
    __device__ __forceinline__ bool valid(int, int, int) const { return true; }
    __device__ __forceinline__ const float* frame(int t) const { return post + (size_t)t * V; }
};
struct RowFrames {
    const float* rows;              // [n_rows, V]
    const long long* frame_row;     // [B, Tmax]
    long long n_rows;
    int Tp, V;
    __device__ __forceinline__ void bind(int b) { frame_row += (size_t)b * Tp; }
    // every row number of the T valid frames inside [0, n_rows)?  (each thread its share; the caller ORs the answers)
    __device__ __forceinline__ bool valid(int T, int tid, int nthreads) const {
        bool ok = true;
        for (int t = tid; t < T; t += nthreads) {
            const long long r = frame_row[t];
            ok = ok && r >= 0 && r < n_rows;
        }
        return ok;
    }
    __device__ __forceinline__ const float* frame(int t) const { return rows + (size_t)frame_row[t] * (size_t)V; }
};

template <int IS_LOG, class Frames>
__global__ __launch_bounds__(ALIGN_THREADS) void ctc_align_kernel(Frames fr,
                                                                  const int* __restrict__ n_frames, const int* __restrict__ tokens,
                                                                  const int* __restrict__ n_tokens, int Lmax, unsigned char* __restrict__ bp,
                                                                  int* __restrict__ start, int* __restrict__ end, float* __restrict__ peak,
                                                                  float* __restrict__ score, int* __restrict__ status) {
    __shared__ float row[2][ALIGN_SMAX];
    __shared__ float em[2][ALIGN_LMAX + 1];       // em[.][0] = blank, em[.][j] = token j - 1
    __shared__ int tok[ALIGN_LMAX];
    __shared__ int s_start[ALIGN_LMAX], s_end[ALIGN_LMAX];
    __shared__ int s_flag[2];                     // [0] a token id outside [1, V); [1] adjacent equal tokens
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = n_frames[b], L = n_tokens[b];
    int* o_start = start + (size_t)b * Lmax;
    int* o_end = end + (size_t)b * Lmax;
    float* o_peak = peak + (size_t)b * Lmax;
    for (int j = tid; j < Lmax; j += ALIGN_THREADS) {
        o_start[j] = -1;
        o_end[j] = -1;
        o_peak[j] = 0.f;
    }
    if (tid == 0) {
        s_flag[0] = 0;
        s_flag[1] = 0;
    }
    const int Tp = fr.Tp, V = fr.V;
    const bool lens_ok = T >= 0 && T <= Tp && L >= 0 && L <= Lmax;      // (uniform over the workgroup)
    if (!lens_ok) {
        if (tid == 0) {
            score[b] = 0.f;
            status[b] = 2;
        }
        return;
    }
    __syncthreads();
    fr.bind(b);
    if (!fr.valid(T, tid, ALIGN_THREADS)) atomicOr(&s_flag[0], 1);     // (a row number out of range: nothing of it is read)
    for (int j = tid; j < L; j += ALIGN_THREADS) {
        const int id = tokens[(size_t)b * Lmax + j];
        tok[j] = id;
        if (id <= 0 || id >= V) atomicOr(&s_flag[0], 1);
    }
    __syncthreads();
    int rep = 0;
    for (int j = tid + 1; j < L; j += ALIGN_THREADS) rep += tok[j] == tok[j - 1];
    if (rep) atomicAdd(&s_flag[1], rep);
    __syncthreads();
    if (s_flag[0] || T < L + s_flag[1]) {
        if (tid == 0) {
            score[b] = 0.f;
            status[b] = s_flag[0] ? 2 : 1;
        }
        return;
    }
    if (T == 0) {                                  // (L == 0 as well: the empty path of the empty hypothesis)
        if (tid == 0) {
            score[b] = 0.f;
            status[b] = 0;
        }
        return;
    }
    const int S = 2 * L + 1, Sb = 2 * Lmax + 1;
    const float* pb = fr.frame(0);
    unsigned char* bpb = bp + (size_t)b * Tp * Sb;
    // frame 0: its L + 1 values, then the first row
    for (int j = tid; j <= L; j += ALIGN_THREADS) em[0][j] = align_logp<IS_LOG>(pb[j ? tok[j - 1] : 0]);
    __syncthreads();
    for (int s = tid; s < S; s += ALIGN_THREADS) {
        row[0][s] = s == 0 ? em[0][0] : s == 1 ? em[0][1] : MASR_ALIGN_NEG;
        bpb[s] = 0;
    }
    if (T > 1) {
        const float* p1 = fr.frame(1);
        for (int j = tid; j <= L; j += ALIGN_THREADS) em[1][j] = align_logp<IS_LOG>(p1[j ? tok[j - 1] : 0]);
    }
    const float* pnext = T > 2 ? fr.frame(2) : nullptr;      // the row of frame t + 1, found one frame before its gather
    __syncthreads();
    for (int t = 1; t < T; ++t) {
        const float* pr = pnext;
        if (t + 2 < T) pnext = fr.frame(t + 2);
        const float* prev = row[(t - 1) & 1];
        float* cur = row[t & 1];
        const float* e = em[t & 1];
        unsigned char* bpt = bpb + (size_t)t * Sb;
        for (int s = tid; s < S; s += ALIGN_THREADS) {
            float best = prev[s];
            int k = 0;
            if (s >= 1) {
                const float a = prev[s - 1];
                if (a > best) {
                    best = a;
                    k = 1;
                }
            }
            if ((s & 1) && s >= 3 && tok[s >> 1] != tok[(s >> 1) - 1]) {
                const float a = prev[s - 2];
                if (a > best) {
                    best = a;
                    k = 2;
                }
            }
            cur[s] = best + e[(s & 1) ? (s + 1) >> 1 : 0];
            bpt[s] = (unsigned char)k;
        }
        if (t + 1 < T) {
            float* en = em[(t + 1) & 1];
            for (int j = tid; j <= L; j += ALIGN_THREADS) en[j] = align_logp<IS_LOG>(pr[j ? tok[j - 1] : 0]);
        }
        __syncthreads();
    }
    // the predecessor bytes of this workgroup are read back by thread 0: make them visible to it
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        const float* last = row[(T - 1) & 1];
        int s = S - 1;
        float sc = last[S - 1];
        if (S >= 2 && last[S - 2] > sc) {
            sc = last[S - 2];
            s = S - 2;
        }
        score[b] = sc;
        status[b] = 0;
        for (int j = 0; j < L; ++j) s_end[j] = -1;
        for (int t = T - 1; t >= 0; --t) {
            if (s & 1) {
                const int j = s >> 1;
                if (s_end[j] < 0) s_end[j] = t;
                s_start[j] = t;
            }
            const int k = bpb[(size_t)t * Sb + s];
            s = s - k < 0 ? 0 : s - k;
        }
    }
    __syncthreads();
    for (int j = tid; j < L; j += ALIGN_THREADS) {
        const int t0 = s_start[j], t1 = s_end[j];
        if (t1 < 0) continue;                      // (cannot happen on a path the trellis allows)
        const int id = tok[j];
        float m = align_logp<IS_LOG>(fr.frame(t0)[id]);
        for (int t = t0 + 1; t <= t1; ++t) {
            const float v = align_logp<IS_LOG>(fr.frame(t)[id]);
            if (v > m) m = v;
        }
        o_start[j] = t0;
        o_end[j] = t1;
        o_peak[j] = m;
    }
}

}  // namespace masr

using namespace masr;

// what the two entry points refuse alike, then the one launch of either: ``fr`` says where the frames lie
template <class Frames>
static int align_launch(masr_engine* e, const std::string& name, Frames fr, int32_t input_is_log, int32_t B, const int32_t* n_frames_dev,
                        const int32_t* tokens_dev, const int32_t* n_tokens_dev, int32_t Lmax, int32_t* start_dev, int32_t* end_dev,
                        float* peak_dev, float* score_dev, int32_t* status_dev, bool frames_null, void* stream) {
    const int32_t Tp = fr.Tp, V = fr.V;
    if (B <= 0 || Tp <= 0 || V < 2 || Lmax < 0) return fail(name + ": B > 0, T' > 0, V >= 2 and Lmax >= 0 expected");
    if (V > 16384) return fail(name + ": V > 16384 is not supported (the CTC head's own limit)");
    if (Lmax > ALIGN_LMAX)
        return fail(name + ": Lmax " + std::to_string(Lmax) + " gives S = 2 Lmax + 1 = " + std::to_string(2 * Lmax + 1) +
                    " states, more than the " + std::to_string(ALIGN_SMAX) + " the trellis rows in LDS hold (MASR_ALIGN_MAX_TOKENS)");
    if (Lmax > Tp) return fail(name + ": Lmax " + std::to_string(Lmax) + " > T' " + std::to_string(Tp) + ": a hypothesis cannot hold more tokens than its utterance has frames");
    if (frames_null || !n_frames_dev || !n_tokens_dev || !score_dev || !status_dev || (Lmax > 0 && (!tokens_dev || !start_dev || !end_dev || !peak_dev)))
        return fail(name + ": null argument");
    hipStream_t s = (hipStream_t)stream;
    // predecessor choices [B][T'][2 Lmax + 1], one byte each: a workspace of the CURRENT lane, like every other per-pass workspace
    CHK(e->align_bp.ensure((size_t)B * Tp * (2 * (size_t)Lmax + 1)));
    unsigned char* bp = e->align_bp.as<unsigned char>();
    if (input_is_log)
        hipLaunchKernelGGL((ctc_align_kernel<1, Frames>), dim3(B), dim3(ALIGN_THREADS), 0, s, fr, n_frames_dev, tokens_dev, n_tokens_dev,
                           Lmax, bp, start_dev, end_dev, peak_dev, score_dev, status_dev);
    else
        hipLaunchKernelGGL((ctc_align_kernel<0, Frames>), dim3(B), dim3(ALIGN_THREADS), 0, s, fr, n_frames_dev, tokens_dev, n_tokens_dev,
                           Lmax, bp, start_dev, end_dev, peak_dev, score_dev, status_dev);
    LAUNCHCHK();
    return 0;
}

extern "C" int masr_ctc_align(masr_engine* e, const float* post_dev, int32_t input_is_log, int32_t B, int32_t Tp, int32_t V,
                              const int32_t* n_frames_dev, const int32_t* tokens_dev, const int32_t* n_tokens_dev, int32_t Lmax,
                              int32_t* start_dev, int32_t* end_dev, float* peak_dev, float* score_dev, int32_t* status_dev,
                              void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    return align_launch(e, "masr_ctc_align", DenseFrames{post_dev, Tp, V}, input_is_log, B, n_frames_dev, tokens_dev, n_tokens_dev, Lmax,
                        start_dev, end_dev, peak_dev, score_dev, status_dev, !post_dev, stream);
}

extern "C" int masr_ctc_align_rows(masr_engine* e, const float* rows_dev, int64_t n_rows, int32_t V, int32_t input_is_log,
                                   const int64_t* frame_row_dev, int32_t B, int32_t Tmax, const int32_t* n_frames_dev,
                                   const int32_t* tokens_dev, const int32_t* n_tokens_dev, int32_t Lmax, int32_t* start_dev,
                                   int32_t* end_dev, float* peak_dev, float* score_dev, int32_t* status_dev, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    if (n_rows <= 0) return fail("masr_ctc_align_rows: n_rows > 0 expected");
    return align_launch(e, "masr_ctc_align_rows", RowFrames{rows_dev, (const long long*)frame_row_dev, (long long)n_rows, Tmax, V},
                        input_is_log, B, n_frames_dev, tokens_dev, n_tokens_dev, Lmax, start_dev, end_dev, peak_dev, score_dev, status_dev,
                        !rows_dev || !frame_row_dev, stream);
}
