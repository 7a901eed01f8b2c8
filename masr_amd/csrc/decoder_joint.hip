// Joint CTC / attention beam search (decoder: joint; masr_joint_decode / masr_op_ctc_prefix_scores): the kernels that come on top
// of the step launches of decoder_step.hip.  Every hypothesis of the attention search carries the log CTC prefix probability psi
// of its tokens over the utterance's valid frames (Watanabe et al., the prefix scorer of joint CTC / attention decoding), and the
// beam is ranked by J = ((1 - ctc_weight) A + ctc_weight psi) + length_bonus n.
//
// Prefix state of hypothesis g: r_n(g)[t] / r_b(g)[t], the log-probabilities of the alignments of g over frames 0 .. t that end in
// a non-blank / in a blank (blank = id 0, eos = V - 1, lp = ln of the posterior).  Extension of g by c (neither blank nor eos),
// phi[t] = r_b(g)[t] when c == last(g), else lse2(r_n(g)[t], r_b(g)[t]):
//     r_n'[0] = lp[0][c] for the empty g, else -inf;  r_b'[0] = -inf;  psi' = r_n'[0]
//     r_n'[t] = lse2(r_n'[t - 1], phi[t - 1]) + lp[t][c]
//     r_b'[t] = lse2(r_n'[t - 1], r_b'[t - 1]) + lp[t][blank]
//     psi'    = lse2(psi', phi[t - 1] + lp[t][c])
// eos: psi' = lse2(r_n(g)[T - 1], r_b(g)[T - 1]); blank: -inf.  All of it float32 in exactly this order, with logf / expf (the
// lse2 of beam_gpu.hip): tests/ctc_prefix_ref.py restates it in numpy.
//
// Mapping: the score kernel runs one wave per hypothesis with lane m = candidate m: r_n(g)[t], r_b(g)[t] are one address for the
// wave, the gathered lp[t][c_m] one per lane, and neither depends on the recurrence, so a batch of frames is loaded in front of
// the chain that consumes it.  The advance kernel runs one wave per winner: the lanes fetch 64 frames at a time (the next 64 while
// the chain of the current ones runs), lane 0 runs the chain out of LDS, the lanes store the 64 results.  The merge kernel is the
// merge of decoder_step.hip over N x M keys.
//
// Shallow fusion with the n-gram language model (masr_joint_decode_lm / masr_op_lm_scores): every hypothesis also carries Lm, the
// float32 running sum of lm(g, c) = ln P(c | the last max_order - 1 tokens of g, <s>-padded) -- masr_lm_cond_log_prob's value bit
// for bit (lm_scorer.h) -- and the key becomes J = (((1 - ctc_weight) A + ctc_weight psi) + lm_weight Lm) + length_bonus n.  The LM
// score kernel has the mapping of the prefix score kernel: one wave per hypothesis, lane m = candidate m.  The scorer state of the
// row (its packed context, matched suffix length and backoffs) is the same for every lane -- the lanes read the same table slots,
// one transaction per probe -- and the candidates' own n-grams are one divergent 16-byte probe per lane and order, longest n-gram
// first (lm_cond_desc: the kernel is bound by the number of such probes, so no more are issued than the recursion needs).
#include "common.h"
#include "step_select.h"

namespace masr {
namespace {

constexpr int BLANK = 0;
constexpr int SCORE_AHEAD = 8;        // frames whose loads are issued in front of their use

__device__ __forceinline__ float lse2(float x, float y) {
    if (x == -INFINITY) return y;
    if (y == -INFINITY) return x;
    const float m = fmaxf(x, y);
    return m + logf(expf(x - m) + expf(y - m));
}

template <int IS_LOG>
__device__ __forceinline__ float logp_of(float v) {
    if (IS_LOG) return v;
    return v > 0.f ? logf(v) : -INFINITY;           // (a NaN probability is "not > 0" as well)
}

__device__ __forceinline__ int utt_of(const PrefixRows& a, int s) { return a.row_utt ? a.row_utt[s] : s / a.N; }

// one wave per row: r_n = -inf, r_b = the running sum of lp[t][blank]; frames behind T are never read and left alone
template <int IS_LOG>
__global__ __launch_bounds__(64) void ctc_prefix_init_kernel(PrefixRows a, float* __restrict__ r) {
    __shared__ float lpb[64];
    const int s = blockIdx.x, lane = threadIdx.x, b = utt_of(a, s);
    const int T = clampi(a.enc_lens[b], 0, a.Tp);
    const float* blank = a.post + (size_t)b * a.Tp * a.V + BLANK;
    float* rn = r + (size_t)s * 2 * a.Tp;
    float* rb = rn + a.Tp;
    float sum = 0.f;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        lpb[lane] = t < T ? logp_of<IS_LOG>(blank[(size_t)t * a.V]) : 0.f;
        __syncthreads();
        float mine = 0.f;
        const int cnt = min(64, T - t0);
        for (int j = 0; j < cnt; ++j) {          // (every lane runs the same sum and keeps the value of its own frame)
            sum += lpb[j];
            if (j == lane) mine = sum;
        }
        if (t < T) {
            rn[t] = -INFINITY;
            rb[t] = mine;
        }
        __syncthreads();
    }
}

struct ScoreArgs {
    PrefixRows pr;
    const int* cand;         // [S, M]
    const int* tok;          // [S, Lcap]
    const int* only_pos;     // [S] or nullptr
    const float* r_cur;      // [S][2][Tp]
    float* psi_out;          // [S, M]
    int M, Lcap, p;
};

template <int IS_LOG>
__global__ __launch_bounds__(64) void ctc_prefix_score_kernel(ScoreArgs a) {
    const PrefixRows& pr = a.pr;
    const int s = blockIdx.x, lane = threadIdx.x, eos = pr.V - 1;
    if (a.only_pos && a.only_pos[s] != a.p) return;
    const int b = utt_of(pr, s);
    if (pr.done && pr.done[b]) return;
    const int last = a.p > 0 ? a.tok[(size_t)s * a.Lcap + (a.p - 1)] : -1;
    if (last == eos) return;                       // a finished hypothesis offers itself: nothing to score
    if (lane >= a.M) return;
    const int T = clampi(pr.enc_lens[b], 0, pr.Tp);
    const int c = clampi(a.cand[(size_t)s * a.M + lane], 0, pr.V - 1);
    const float* __restrict__ rn = a.r_cur + (size_t)s * 2 * pr.Tp;
    const float* __restrict__ rb = rn + pr.Tp;
    float psi;
    if (T < 1 || c == BLANK) {
        psi = -INFINITY;
    } else if (c == eos) {
        psi = lse2(rn[T - 1], rb[T - 1]);
    } else {
        const float* __restrict__ col = pr.post + (size_t)b * pr.Tp * pr.V + c;
        const bool rep = c == last;
        psi = a.p == 0 ? logp_of<IS_LOG>(col[0]) : -INFINITY;
        int t = 1;
        for (; t + SCORE_AHEAD <= T; t += SCORE_AHEAD) {
            float v[SCORE_AHEAD], gn[SCORE_AHEAD], gb[SCORE_AHEAD];
#pragma unroll
            for (int j = 0; j < SCORE_AHEAD; ++j) {
                v[j] = col[(size_t)(t + j) * pr.V];
                gn[j] = rn[t + j - 1];
                gb[j] = rb[t + j - 1];
            }
#pragma unroll
            for (int j = 0; j < SCORE_AHEAD; ++j) {
                const float phi = rep ? gb[j] : lse2(gn[j], gb[j]);
                psi = lse2(psi, __fadd_rn(phi, logp_of<IS_LOG>(v[j])));
            }
        }
        for (; t < T; ++t) {
            const float phi = rep ? rb[t - 1] : lse2(rn[t - 1], rb[t - 1]);
            psi = lse2(psi, __fadd_rn(phi, logp_of<IS_LOG>(col[(size_t)t * pr.V])));
        }
    }
    a.psi_out[(size_t)s * a.M + lane] = psi;
}

struct AdvanceArgs {
    PrefixRows pr;
    const int* tok_next;     // [S, Lcap]
    const int* anc_next;     // [S, Lcap]
    const int* row_len;      // [S] or nullptr
    const float* r_cur;
    float* r_next;
    int Lcap, p;
};

template <int IS_LOG>
__global__ __launch_bounds__(64) void ctc_prefix_advance_kernel(AdvanceArgs a) {
    __shared__ float in[4][64];          // lp[t][c] | lp[t][blank] | r_n(g)[t - 1] | r_b(g)[t - 1] of the chunk's frames
    __shared__ float out[2][64];
    const PrefixRows& pr = a.pr;
    const int s = blockIdx.x, lane = threadIdx.x, eos = pr.V - 1, Tp = pr.Tp;
    const int b = utt_of(pr, s);
    if (pr.done && pr.done[b]) return;
    const int T = clampi(pr.enc_lens[b], 0, Tp);
    float* __restrict__ rn_o = a.r_next + (size_t)s * 2 * Tp;
    float* __restrict__ rb_o = rn_o + Tp;
    if (a.row_len && a.p >= a.row_len[s]) {        // (the scorer op: a prefix that has no token at p keeps its state)
        const float* own = a.r_cur + (size_t)s * 2 * Tp;
        for (int t = lane; t < T; t += 64) {
            rn_o[t] = own[t];
            rb_o[t] = own[Tp + t];
        }
        return;
    }
    const int c = a.tok_next[(size_t)s * a.Lcap + a.p];
    if (c == eos) return;                          // finished: its state is never read again
    const int s0 = (s / pr.N) * pr.N;
    const int parent = s0 + clampi(a.anc_next[(size_t)s * a.Lcap + a.p], 0, pr.N - 1);
    const float* __restrict__ rn_g = a.r_cur + (size_t)parent * 2 * Tp;
    const float* __restrict__ rb_g = rn_g + Tp;
    if (c <= BLANK || c > eos) {                   // blank (or no token id at all): no alignment ends in it
        for (int t = lane; t < T; t += 64) {
            rn_o[t] = -INFINITY;
            rb_o[t] = -INFINITY;
        }
        return;
    }
    const int last = a.p > 0 ? a.tok_next[(size_t)s * a.Lcap + (a.p - 1)] : -1;
    const bool rep = c == last;
    const float* __restrict__ frame = pr.post + (size_t)b * Tp * pr.V;
    float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f;           // the chunk fetched ahead
    auto fetch = [&](int t0) {
        const int t = t0 + lane;
        if (t < T) {
            n0 = frame[(size_t)t * pr.V + c];
            n1 = frame[(size_t)t * pr.V + BLANK];
            n2 = t > 0 ? rn_g[t - 1] : -INFINITY;
            n3 = t > 0 ? rb_g[t - 1] : -INFINITY;
        }
    };
    fetch(0);
    float cn = -INFINITY, cb = -INFINITY;          // r_n'[t - 1], r_b'[t - 1] (lane 0)
    for (int t0 = 0; t0 < T; t0 += 64) {
        in[0][lane] = logp_of<IS_LOG>(n0);
        in[1][lane] = logp_of<IS_LOG>(n1);
        in[2][lane] = n2;
        in[3][lane] = n3;
        __syncthreads();
        if (t0 + 64 < T) fetch(t0 + 64);
        if (lane == 0) {
            const int cnt = min(64, T - t0);
            for (int j = 0; j < cnt; ++j) {
                float vn, vb;
                if (t0 + j == 0) {
                    vn = a.p == 0 ? in[0][0] : -INFINITY;
                    vb = -INFINITY;
                } else {
                    const float phi = rep ? in[3][j] : lse2(in[2][j], in[3][j]);
                    vn = __fadd_rn(lse2(cn, phi), in[0][j]);
                    vb = __fadd_rn(lse2(cn, cb), in[1][j]);
                }
                out[0][j] = vn;
                out[1][j] = vb;
                cn = vn;
                cb = vb;
            }
        }
        __syncthreads();
        if (t0 + lane < T) {
            rn_o[t0 + lane] = out[0][lane];
            rb_o[t0 + lane] = out[1][lane];
        }
    }
}

// lm_out [S, M] = lm(row s, candidate m): the row's scorer state from the last max_order - 1 of its tokens (tok [S, Lcap]; row_len
// [S] given: the op's prefix lengths, else every row holds p tokens), the candidate scored behind it.  eos = V - 1 is read as the
// model's </s>, every other id is its own LM word; an unknown candidate or context word gives LM_OOV_SCORE.  Rows of a finished
// utterance and (in the search) rows whose last token is eos are skipped.
struct LmScoreArgs {
    LmView lm;
    const int* cand;         // [S, M]
    const int* tok;          // [S, Lcap]
    const int* row_len;      // [S] or nullptr
    const int* done;         // [B] or nullptr
    float* lm_out;           // [S, M]
    int N, M, Lcap, p, V;
};

template <int ORD>
__global__ __launch_bounds__(64) void joint_lm_score_kernel(LmScoreArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x, eos = a.V - 1;
    if (a.done && a.done[s / a.N]) return;
    const int* __restrict__ row = a.tok + (size_t)s * a.Lcap;
    const int len = a.row_len ? clampi(a.row_len[s], 0, a.Lcap) : a.p;
    if (!a.row_len && len > 0 && row[len - 1] == eos) return;        // a finished hypothesis offers itself: nothing to score
    // the <s>-padded window of masr_lm_cond_log_prob; one address per token for the whole wave
    unsigned long long ctx = lm_root_ctx(a.lm);
    for (int j = len - min(len, a.lm.max_order - 1); j < len; ++j) ctx = lm_push(ctx, __builtin_amdgcn_readfirstlane(row[j]));
    const LmState st = lm_state_of(a.lm, ctx);
    if (lane >= a.M) return;
    const int c = clampi(a.cand[(size_t)s * a.M + lane], 0, a.V - 1);
    const int w = c == eos ? a.lm.eos : c;
    float v = LM_OOV_SCORE;
    if (!st.oov && w < a.lm.n_words && a.lm.known[w]) {
        float uni = LM_OOV_SCORE, ubo = 0.f;
        lm_find(a.lm, lm_key(0ull, 0, w), &uni, &ubo);       // (a known word has its unigram)
        v = lm_cond_desc<ORD>(a.lm, st, w, uni);
    }
    a.lm_out[(size_t)s * a.M + lane] = v;
}

// Beam merge of step i = p + 1 by the joint key, one workgroup of 256 per utterance (step_merge_kernel over N x M candidates): a
// finished row offers itself once with its own J, A, psi, Lm, n and -inf otherwise; the N best keys, ties to the smaller flat index
// parent * M + candidate; everything a hypothesis carries written to the `next` tables through the parent index.
__global__ __launch_bounds__(256) void joint_merge_kernel(JointMerge a) {
    __shared__ float cand[64 * 64];
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    __shared__ int parent[64], newtok[64], nfin;
    const int b = blockIdx.x, N = a.N, M = a.M, eos = a.V - 1, p = a.p;
    const size_t s0 = (size_t)b * N;
    const int lim = step_limit(a.enc_lens[b], a.Tp, a.max_len, a.max_pos, a.Lcap);
    const bool frozen = p + 1 > lim;
    const float wa = __fsub_rn(1.0f, a.ctc_weight);
    if (threadIdx.x == 0) nfin = 0;
    if (!frozen) {
        for (int c = threadIdx.x; c < N * M; c += 256) {
            const int h = c / M, k = c - h * M;
            const bool fin = p > 0 && a.tok_cur[(s0 + h) * a.Lcap + (p - 1)] == eos;
            float key;
            if (fin) {
                key = k == 0 ? a.key_cur[s0 + h] : -INFINITY;
            } else {
                const int t = clampi(a.top_i[(s0 + h) * M + k], 0, a.V - 1);
                const float att = __fadd_rn(a.att_cur[s0 + h], a.top_v[(s0 + h) * M + k]);
                const float n = (float)(a.n_cur[s0 + h] + (t != eos ? 1 : 0));
                float mix = __fmul_rn(wa, att);
                if (a.psi_cand) mix = __fadd_rn(mix, __fmul_rn(a.ctc_weight, a.psi_cand[(s0 + h) * M + k]));
                if (a.lm_cand)
                    mix = __fadd_rn(mix, __fmul_rn(a.lm_weight, __fadd_rn(a.lm_cur[s0 + h], a.lm_cand[(s0 + h) * M + k])));
                key = __fadd_rn(mix, __fmul_rn(a.length_bonus, n));
            }
            cand[c] = key;
        }
        __syncthreads();
        float pv = 0.f;
        int pi = -1;
        for (int k = 0; k < N; ++k) {
            float bv = 0.f;
            int bi = -1;
            for (int c = threadIdx.x; c < N * M; c += 256) {
                const float v = cand[c];
                if (v != v) continue;
                if (pi >= 0 && !before(pv, pi, v, c)) continue;
                if (bi < 0 || before(v, c, bv, bi)) {
                    bv = v;
                    bi = c;
                }
            }
            block_first(bv, bi, red_v, red_i);
            if (bi < 0) {            // (NaN keys only: keep the row count with dead entries)
                bv = -INFINITY;
                bi = min(k, N * M - 1);
            }
            if (threadIdx.x == 0) {
                const int h = bi / M, kk = bi - h * M;
                const bool fin = p > 0 && a.tok_cur[(s0 + h) * a.Lcap + (p - 1)] == eos;
                const int t = fin ? eos : clampi(a.top_i[(s0 + h) * M + kk], 0, a.V - 1);
                parent[k] = h;
                newtok[k] = t;
                a.key_next[s0 + k] = bv;
                a.att_next[s0 + k] = fin ? a.att_cur[s0 + h] : __fadd_rn(a.att_cur[s0 + h], a.top_v[(s0 + h) * M + kk]);
                a.psi_next[s0 + k] = fin ? a.psi_cur[s0 + h] : (a.psi_cand ? a.psi_cand[(s0 + h) * M + kk] : 0.f);
                a.lm_next[s0 + k] = (fin || !a.lm_cand) ? a.lm_cur[s0 + h] : __fadd_rn(a.lm_cur[s0 + h], a.lm_cand[(s0 + h) * M + kk]);
                a.n_next[s0 + k] = a.n_cur[s0 + h] + ((!fin && t != eos) ? 1 : 0);
                if (t == eos) nfin += 1;
            }
            pv = bv;
            pi = bi;
        }
    } else {
        for (int k = threadIdx.x; k < N; k += 256) {
            parent[k] = k;
            a.key_next[s0 + k] = a.key_cur[s0 + k];
            a.att_next[s0 + k] = a.att_cur[s0 + k];
            a.psi_next[s0 + k] = a.psi_cur[s0 + k];
            a.lm_next[s0 + k] = a.lm_cur[s0 + k];
            a.n_next[s0 + k] = a.n_cur[s0 + k];
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

__global__ void joint_init_kernel(float* att, float* psi, float* lm, int* n, int S, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    att[i] = (i % N == 0) ? 0.f : -INFINITY;
    psi[i] = 0.f;
    lm[i] = 0.f;
    n[i] = 0;
}

}  // namespace

void launch_prefix_init(const PrefixRows& pr, float* r, hipStream_t s) {
    if (pr.input_is_log) hipLaunchKernelGGL(ctc_prefix_init_kernel<1>, dim3((unsigned)pr.S), dim3(64), 0, s, pr, r);
    else hipLaunchKernelGGL(ctc_prefix_init_kernel<0>, dim3((unsigned)pr.S), dim3(64), 0, s, pr, r);
}

void launch_prefix_score(const PrefixRows& pr, const int* cand, int M, const int* tok, int Lcap, int p, const int* only_pos,
                         const float* r_cur, float* psi_out, hipStream_t s) {
    ScoreArgs a{};
    a.pr = pr; a.cand = cand; a.tok = tok; a.only_pos = only_pos; a.r_cur = r_cur; a.psi_out = psi_out;
    a.M = M; a.Lcap = Lcap; a.p = p;
    if (pr.input_is_log) hipLaunchKernelGGL(ctc_prefix_score_kernel<1>, dim3((unsigned)pr.S), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(ctc_prefix_score_kernel<0>, dim3((unsigned)pr.S), dim3(64), 0, s, a);
}

void launch_prefix_advance(const PrefixRows& pr, const int* tok_next, const int* anc_next, int Lcap, int p, const int* row_len,
                           const float* r_cur, float* r_next, hipStream_t s) {
    AdvanceArgs a{};
    a.pr = pr; a.tok_next = tok_next; a.anc_next = anc_next; a.row_len = row_len; a.r_cur = r_cur; a.r_next = r_next;
    a.Lcap = Lcap; a.p = p;
    if (pr.input_is_log) hipLaunchKernelGGL(ctc_prefix_advance_kernel<1>, dim3((unsigned)pr.S), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(ctc_prefix_advance_kernel<0>, dim3((unsigned)pr.S), dim3(64), 0, s, a);
}

void launch_joint_merge(const JointMerge& m, int B, hipStream_t s) {
    hipLaunchKernelGGL(joint_merge_kernel, dim3((unsigned)B), dim3(256), 0, s, m);
}

void launch_joint_init(float* att, float* psi, float* lm, int* n, int S, int N, hipStream_t s) {
    hipLaunchKernelGGL(joint_init_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, att, psi, lm, n, S, N);
}

int launch_joint_lm_score(const LmView& lm, const int* cand, int M, const int* tok, int Lcap, int p, const int* row_len,
                          const int* done, int S, int N, int V, float* lm_out, hipStream_t s) {
    if (lm.max_order < 1 || lm.max_order > 5) return 1;
    LmScoreArgs a{};
    a.lm = lm; a.cand = cand; a.tok = tok; a.row_len = row_len; a.done = done; a.lm_out = lm_out;
    a.N = N; a.M = M; a.Lcap = Lcap; a.p = p; a.V = V;
    // (the order bounds the keys a lane holds in registers: two instantiations, as the CTC search has them)
    if (lm.max_order <= 3) hipLaunchKernelGGL(joint_lm_score_kernel<3>, dim3((unsigned)S), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(joint_lm_score_kernel<5>, dim3((unsigned)S), dim3(64), 0, s, a);
    return 0;
}

}  // namespace masr
