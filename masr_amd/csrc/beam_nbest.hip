// The N best prefixes of a CTC prefix beam search that has finished (beam_gpu.hip): a second, small kernel over what the search
// left in HBM.  beam_search_kernel ends by persisting its whole live set (state_i: n_live, node[], ch[]; state_f: score[]) for
// offline calls and streams alike, and the survivors' trie is the utterance's node pool (pool_parent, pool_ch) -- nothing of the
// search changes, so every result it gives stays bit-identical.
//
// One workgroup (512 threads >= beam) per utterance:
//   rank     the order is the search's own best pick (tail of beam_search_kernel): higher score first; of bit-equal scores the
//            smaller last character; of equal (score, character) the smaller live index.  The keys of the live prefixes go to LDS
//            as order-preserving integers (-inf and equal bits compare as integers, never as floats) and every thread COUNTS the
//            prefixes that precede its own: a total order, so the ranks are a permutation and order[rank] = i has no conflicts.
//            One difference from the search's float comparison: it takes +0.0 and -0.0 for equal, the integer keys put -0.0
//            below +0.0.  A search score is a sum of logarithms of probabilities, where log(1) = +0.0: it is never -0.0.
//   extract  thread r < min(nbest, n_live) walks the parent chain of order[r] as the search does for its one result: length
//            first, then the tokens root to leaf; the walk stops at x <= 0 || x >= pool_cap.  With a scorer bound the reported
//            score is the decoder's approx_ctc, computed by the same lm_* calls in the same order as the search's own.
#include <math.h>

#include "common.h"

namespace masr {

static constexpr int NB_THREADS = 512;

__device__ __forceinline__ unsigned nb_okey(float f) {      // larger float -> larger unsigned (okey of beam_gpu.hip)
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(NB_THREADS) void beam_nbest_kernel(BeamNbestArgs a) {
    __shared__ unsigned k_sc[NB_THREADS];
    __shared__ int k_ch[NB_THREADS];
    __shared__ int order[NB_THREADS];
    const int u = blockIdx.x, tid = threadIdx.x, beam = a.beam;
    const int* st_i = a.state_i + (size_t)u * (2 + 3 * beam);
    const float* st_f = a.state_f + (size_t)u * (7 * beam);
    const int* pool_parent = a.pool_parent + (size_t)u * a.pool_cap;
    const int* pool_ch = a.pool_ch + (size_t)u * a.pool_cap;
    const int n = min(max(st_i[0], 0), beam);
    if (tid < n) {
        k_sc[tid] = nb_okey(st_f[2 * beam + tid]);
        k_ch[tid] = st_i[2 + beam + tid];
    }
    __syncthreads();
    if (tid < n) {
        const unsigned ms = k_sc[tid];
        const int mc = k_ch[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const unsigned s = k_sc[j];
            const int c = k_ch[j];
            rank += (s > ms || (s == ms && (c < mc || (c == mc && j < tid)))) ? 1 : 0;
        }
        order[rank] = tid;
    }
    __syncthreads();
    const int cnt = min(a.nbest, n);
    if (tid == 0) a.count[u] = cnt;
    if (tid >= a.nbest) return;
    const size_t row = (size_t)u * a.nbest + tid;
    if (tid >= cnt) {                        // rows past count: empty, their tokens untouched
        a.len[row] = 0;
        a.score[row] = -INFINITY;
        return;
    }
    const int i = order[tid];
    const int node = st_i[2 + i];
    float bs = st_f[2 * beam + i];
    int* tokens = a.tokens + row * a.max_len;
    int L = 0;
    // (a node's parent was allocated before it, so a chain of the search is shorter than the pool: the bound on L only ends the
    // walk over a pool that is not one)
    for (int x = node; x > 0 && x < a.pool_cap && L < a.pool_cap; x = pool_parent[x]) ++L;
    a.len[row] = L;
    int pos = L - 1;
    for (int x = node; x > 0 && x < a.pool_cap && pos >= 0; x = pool_parent[x], --pos)
        if (pos < a.max_len) tokens[pos] = pool_ch[x];
    if (a.use_lm && L <= a.max_len) {
        // approx_ctc of the reference decoder, as at the tail of beam_search_kernel: score - |prefix| * beta - alpha * ln
        // P_LM(sentence), the sentence probability counting </s>
        unsigned long long ctx = lm_root_ctx(a.lm);
        float sent = L == 0 ? lm_cond(a.lm, lm_state_of(a.lm, ctx), a.lm.bos) : 0.f;
        for (int k = 0; k <= L; ++k) {
            const int w = k < L ? tokens[k] : a.lm.eos;
            sent += lm_cond(a.lm, lm_state_of(a.lm, ctx), w);
            ctx = lm_push(ctx, w);
        }
        bs = bs - (float)L * a.beta - a.alpha * sent;
    }
    a.score[row] = bs;
}

int launch_beam_nbest(const BeamNbestArgs& a, int B, hipStream_t s) {
    if (B <= 0) return 0;
    if (a.beam < 1 || a.beam > NB_THREADS || a.nbest < 1 || a.nbest > a.beam || a.max_len < 1 || a.pool_cap < 1 ||
        a.pool_cap > (1 << 30))
        return 1;
    if (a.use_lm && (a.lm.max_order < 1 || a.lm.max_order > 5)) return 1;
    hipLaunchKernelGGL(beam_nbest_kernel, dim3(B), dim3(NB_THREADS), 0, s, a);
    return 0;
}

}  // namespace masr
