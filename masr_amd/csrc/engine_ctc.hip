// libmasr_hip.so -- engine, CTC: the head, greedy collapse, top-k pruning and the prefix beam search on the device.  Host code only (file map: engine_state.h).
#include "engine_encoder.h"

using namespace masr;

// the one refusal of a vocabulary the softmax / pruning kernels cannot hold (masr_ctc_probs and the chunk steps)
static const char kVocabRefusal[] = "vocab_size > 16384 is not supported by the softmax / pruning kernels (one 256-thread workgroup holds a row in registers)";

extern "C" {

static int ctc_head(masr_engine* e, const float* enc_dev, int M, float* probs_dev, int write_probs, int32_t* argmax_dev,
                    float* maxprob_dev, hipStream_t s) {
    const int d = enc_dim(e), V = e->cfg.vocab_size;
    float* logits = probs_dev;
    if (!logits) {
        CHK(e->logits.ensure((size_t)M * V * sizeof(float)));
        logits = e->logits.as<float>();
    }
    gemm(e, s, enc_dev, d, e->ctc_w, e->ctc_b, logits, V, M, V, d, ACT_NONE, 1.f, nullptr, 0);
    launch_softmax_argmax(logits, M, V, V, write_probs, argmax_dev, maxprob_dev, s);
    LAUNCHCHK();
    return 0;
}

int masr_ctc_probs(masr_engine* e, const float* enc_dev, int32_t M, float* probs_dev, int32_t* argmax_dev,
                   float* maxprob_dev, void* stream) {
    if (!e || !e->finalized) return fail("engine not finalized");
    ENTER(e);
    CallGuard call_guard(e, (hipStream_t)stream);
    if (!probs_dev) return fail("probs_dev is null");
    if (e->cfg.vocab_size > 16384) return fail(kVocabRefusal);
    return ctc_head(e, enc_dev, M, probs_dev, 1, argmax_dev, maxprob_dev, (hipStream_t)stream);
}

int masr_ctc_greedy_frames(masr_engine* e, const float* enc_dev, int32_t M, int32_t* argmax_dev, float* maxprob_dev,
                           void* stream) {
    if (!e || !e->finalized) return fail("engine not finalized");
    ENTER(e);
    CallGuard call_guard(e, (hipStream_t)stream);
    if (e->cfg.model_kind == 3 || is_wide(e))      // K = 512 / 1024 / 2048 rows, or the width-generic path at 256 (no packed copies): generic GEMM + softmax statistics (logits stay in a workspace)
        return ctc_head(e, enc_dev, M, nullptr, 0, argmax_dev, maxprob_dev, (hipStream_t)stream);
    // few row blocks (one utterance: 7; the Efficient Conformer's half-rate output at 32 x 10 s: 124): the fused head gives a
    // workgroup 32 rows x the WHOLE vocabulary (165 us whether 7 or 248 row blocks run); below knobs().ctc_fused_blocks the logits go
    // through the tiled GEMM (vocabulary spread over the CUs) into a workspace and the softmax statistics are a second launch
    if ((M + 31) / 32 < knobs().ctc_fused_blocks) return ctc_head(e, enc_dev, M, nullptr, 0, argmax_dev, maxprob_dev, (hipStream_t)stream);
    // fused: logits GEMM + online softmax statistics + argmax, nothing but (idx, prob) leaves the chip
    {
        RowGemmArgs g = rg_args(enc_dev, e->cfg.d_model, e->ctc_w, e->ctc_b, nullptr, 0, M, e->cfg.vocab_size);
        g.out_idx = argmax_dev; g.out_maxp = maxprob_dev;
        rowgemm(e, (hipStream_t)stream, RG_PRO_PLAIN, RG_EPI_CTC, g);
    }
    LAUNCHCHK();
    return 0;
}

int masr_ctc_collapse(masr_engine* e, const int32_t* argmax_dev, const float* maxprob_dev, const int32_t* n_frames_dev,
                      int32_t B, int32_t Tp, int32_t blank, int32_t* tokens_dev, int32_t* n_tokens_dev,
                      float* score_dev, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    if (Tp > CTC_COLLAPSE_MAX_FRAMES) return fail(std::string("masr_ctc_collapse: ") + ctc_collapse_refusal);
    launch_ctc_collapse(argmax_dev, maxprob_dev, n_frames_dev, B, Tp, blank, tokens_dev, n_tokens_dev, score_dev,
                        (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

int masr_op_ctc_collapse_rows(masr_engine* e, const int32_t* argmax_dev, const float* maxprob_dev, const int32_t* n_frames_dev,
                              const int32_t* in_rows_dev_or_null, int32_t ld_in, int32_t B, int32_t Tp, int32_t blank,
                              int32_t* rows_dev, void* stream) {
    if (!e) return fail("null engine");
    if (!argmax_dev || !maxprob_dev || !n_frames_dev || !rows_dev) return fail("masr_op_ctc_collapse_rows: null argument");
    if (B < 0 || Tp < 0) return fail("masr_op_ctc_collapse_rows: B and Tp must not be negative");
    if (in_rows_dev_or_null && ld_in < Tp) return fail("masr_op_ctc_collapse_rows: ld_in must be at least Tp");
    if (Tp > CTC_COLLAPSE_MAX_FRAMES) return fail(std::string("masr_op_ctc_collapse_rows: ") + ctc_collapse_refusal);
    ENTER(e);
    if (in_rows_dev_or_null)
        launch_ctc_collapse_hist(argmax_dev, maxprob_dev, n_frames_dev, in_rows_dev_or_null, ld_in, B, Tp, blank, rows_dev,
                                 (hipStream_t)stream);
    else
        launch_ctc_collapse_rows(argmax_dev, maxprob_dev, n_frames_dev, B, Tp, blank, rows_dev, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

int masr_argmax_rows(masr_engine* e, const float* probs_dev, int32_t M, int32_t V, int32_t* argmax_dev,
                     float* maxprob_dev, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    if (V > 16384) return fail("V > 16384 not supported (one 256-thread workgroup holds a row in registers)");
    launch_argmax_rows(probs_dev, M, V, argmax_dev, maxprob_dev, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

int masr_ctc_topk(masr_engine* e, const float* probs_dev, int32_t M, int32_t V, int32_t top_n, float cutoff_prob,
                  int32_t* idx_dev, float* logp_dev, int32_t* count_dev, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    if (V > 16384) return fail("V > 16384 not supported (one 256-thread workgroup holds a row in registers)");
    if (top_n <= 0) return fail("top_n must be positive");
    launch_topk_prune(probs_dev, M, V, top_n, cutoff_prob, idx_dev, logp_dev, count_dev, -1, nullptr, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

int masr_ctc_topk_blank(masr_engine* e, const float* probs_dev, int32_t M, int32_t V, int32_t top_n, float cutoff_prob,
                        int32_t blank, int32_t* idx_dev, float* logp_dev, int32_t* count_dev, float* blank_logp_dev,
                        void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    if (V > 16384) return fail("V > 16384 not supported (one 256-thread workgroup holds a row in registers)");
    if (top_n <= 0) return fail("top_n must be positive");
    if (blank < 0 || blank >= V || !blank_logp_dev) return fail("masr_ctc_topk_blank: blank id out of range or null output");
    launch_topk_prune(probs_dev, M, V, top_n, cutoff_prob, idx_dev, logp_dev, count_dev, blank, blank_logp_dev,
                      (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

static int bind_lm(BeamGpuArgs& a, masr_lm* lm, float alpha, float beta) {
    a.use_lm = 0;
    a.lm_cache = knobs().beam_lm_cache;
    a.narrow = knobs().beam_narrow;
    a.alpha = alpha;
    a.beta = beta;
    if (!lm) return 0;
    if (lm_device_view(lm, &a.lm)) return fail(masr_lm_last_error());
    a.use_lm = 1;
    return 0;
}

int masr_beam_search_gpu(masr_engine* e, const int32_t* idx_dev, const float* logp_dev, const int32_t* count_dev,
                         const int32_t* frames_dev, int32_t B, int32_t T_stride, int32_t K, int32_t beam_size, int32_t blank,
                         int32_t* tokens_dev, int32_t max_len, int32_t* len_dev, float* score_dev, void* stream) {
    return masr_beam_search_gpu_lm(e, idx_dev, logp_dev, count_dev, frames_dev, B, T_stride, K, beam_size, blank, nullptr, 0.f,
                                   0.f, nullptr, tokens_dev, max_len, len_dev, score_dev, stream);
}

int masr_beam_search_gpu_lm(masr_engine* e, const int32_t* idx_dev, const float* logp_dev, const int32_t* count_dev,
                            const int32_t* frames_dev, int32_t B, int32_t T_stride, int32_t K, int32_t beam_size, int32_t blank,
                            masr_lm* lm, float alpha, float beta, const float* blank_logp_dev, int32_t* tokens_dev,
                            int32_t max_len, int32_t* len_dev, float* score_dev, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    if (B <= 0 || T_stride <= 0) return fail("empty batch");
    if (e->cfg.vocab_size > 16384 && e->finalized) return fail("vocab_size > 16384 not supported");
    BeamGpuArgs a{};
    a.cidx = idx_dev; a.clp = logp_dev; a.ccount = count_dev; a.frames = frames_dev;
    a.blank_lp = lm ? blank_logp_dev : nullptr;
    a.T_stride = T_stride; a.K = K; a.beam = beam_size; a.blank = blank; a.max_len = max_len;
    a.pool_cap = T_stride * beam_size + 1;
    if (lm && lm_word_based(lm))
        return fail("word-based language models are searched on host threads (masr_beam_search_batch_lm): the spelling "
                    "dictionary is not in the GPU kernel");
    if (K > 64 || beam_size > 512 || beam_size < 1 || beam_gpu_lds_bytes(beam_size, K, lm != nullptr) > 160 * 1024)
        return fail("beam search on the GPU needs cutoff_top_n <= 64, beam_size <= 512 and beam_size*cutoff_top_n*4 B + tables "
                    "within 160 KB of LDS; use masr_beam_search_batch (host threads) beyond that");
    DevBuf *pool = &e->beam_pool, *state = &e->beam_state;
    if (!e->beam_first_set) {
        e->beam_first_set = true;
        e->beam_first_stream = stream;
    } else if (stream != e->beam_first_stream) {
        auto& ws = e->beam_ws[stream];
        pool = &ws.first;
        state = &ws.second;
    }
    BeamLast& last = e->beam_last[stream];      // (masr_beam_nbest_gpu: nothing to read until this search is launched)
    last.valid = false;
    CHK(pool->ensure((size_t)B * a.pool_cap * 2 * sizeof(int)));
    CHK(state->ensure((size_t)B * beam_state_bytes(beam_size)));
    a.pool_parent = pool->as<int>();
    a.pool_ch = a.pool_parent + (size_t)B * a.pool_cap;
    beam_state_carve(state->p, B, beam_size, &a.state_h, &a.state_i, &a.state_f);
    CHK(bind_lm(a, lm, alpha, beta));
    a.init = 1;
    a.prof = e->beam_prof;
    a.tokens = tokens_dev; a.len = len_dev; a.score = score_dev;
    if (launch_beam_search(a, B, (hipStream_t)stream)) return fail("beam search launch rejected the sizes");
    LAUNCHCHK();
    last.valid = true;
    last.lm = lm;
    last.alpha = lm ? alpha : 0.f;
    last.beta = lm ? beta : 0.f;
    last.B = B;
    last.beam = beam_size;
    last.pool_cap = a.pool_cap;
    return 0;
}

// ---- the N best prefixes of the search that ran last (beam_nbest.hip) ----------------------------------------------------------
static int nbest_sizes(const char* who, int beam, int nbest, int max_len, const void* tokens, const void* len, const void* score,
                       const void* count) {
    if (!tokens || !len || !score || !count) return fail(std::string(who) + ": null output");
    if (nbest < 1 || nbest > beam)
        return fail(std::string(who) + ": nbest = " + std::to_string(nbest) + " is outside 1 .. beam_size = " + std::to_string(beam));
    if (max_len < 1) return fail(std::string(who) + ": max_len must be at least 1");
    return 0;
}

int masr_beam_nbest_gpu(masr_engine* e, int32_t B, int32_t beam_size, int32_t nbest, masr_lm* lm, float alpha, float beta,
                        int32_t* tokens_dev, int32_t max_len, int32_t* len_dev, float* score_dev, int32_t* count_dev, void* stream) {
    if (!e) return fail("null engine");
    const auto it = e->beam_last.find(stream);
    if (it == e->beam_last.end() || !it->second.valid)
        return fail("masr_beam_nbest_gpu: no masr_beam_search_gpu has run on this stream of the engine: there is no live set to read");
    const BeamLast& last = it->second;
    if (B != last.B || beam_size != last.beam)
        return fail("masr_beam_nbest_gpu: B = " + std::to_string(B) + ", beam_size = " + std::to_string(beam_size) +
                    " are not the last search's on this stream (B = " + std::to_string(last.B) + ", beam_size = " +
                    std::to_string(last.beam) + ")");
    if ((const void*)lm != last.lm)
        return fail(!lm ? "masr_beam_nbest_gpu: the last search on this stream had a language model bound and this call has none"
                        : last.lm ? "masr_beam_nbest_gpu: the language model is not the one the last search on this stream had bound"
                                  : "masr_beam_nbest_gpu: the last search on this stream had no language model bound and this call has one");
    if (lm && (alpha != last.alpha || beta != last.beta))
        return fail("masr_beam_nbest_gpu: alpha = " + std::to_string(alpha) + ", beta = " + std::to_string(beta) +
                    " are not the weights of the last search on this stream (alpha = " + std::to_string(last.alpha) + ", beta = " +
                    std::to_string(last.beta) + "): entry 0 would not be that search's score");
    CHK(nbest_sizes("masr_beam_nbest_gpu", beam_size, nbest, max_len, tokens_dev, len_dev, score_dev, count_dev));
    ENTER(e);
    const bool first = e->beam_first_set && stream == e->beam_first_stream;
    DevBuf& pool = first ? e->beam_pool : e->beam_ws[stream].first;
    DevBuf& state = first ? e->beam_state : e->beam_ws[stream].second;
    BeamGpuArgs g{};
    g.pool_cap = last.pool_cap;
    g.pool_parent = pool.as<int>();
    g.pool_ch = g.pool_parent + (size_t)B * g.pool_cap;
    beam_state_carve(state.p, B, beam_size, &g.state_h, &g.state_i, &g.state_f);
    CHK(bind_lm(g, lm, alpha, beta));
    BeamNbestArgs a{};
    a.state_i = g.state_i; a.state_f = g.state_f; a.pool_parent = g.pool_parent; a.pool_ch = g.pool_ch;
    a.pool_cap = g.pool_cap; a.beam = beam_size; a.nbest = nbest; a.max_len = max_len;
    a.tokens = tokens_dev; a.len = len_dev; a.score = score_dev; a.count = count_dev;
    a.use_lm = g.use_lm; a.lm = g.lm; a.alpha = alpha; a.beta = beta;
    if (launch_beam_nbest(a, B, (hipStream_t)stream)) return fail("masr_beam_nbest_gpu: launch rejected the sizes");
    LAUNCHCHK();
    return 0;
}

int masr_op_beam_nbest(masr_engine* e, const int32_t* n_live_host, const int32_t* node_host, const int32_t* ch_host,
                       const float* score_host, const int32_t* pool_parent_host, const int32_t* pool_ch_host, int32_t B,
                       int32_t beam_size, int32_t pool_cap, int32_t nbest, int32_t* tokens_host, int32_t max_len, int32_t* len_host,
                       float* score_host_out, int32_t* count_host) {
    // every refusal comes before the engine is touched: none of them needs a device
    static const char who[] = "masr_op_beam_nbest";
    if (!n_live_host || !node_host || !ch_host || !score_host || !pool_parent_host || !pool_ch_host)
        return fail(std::string(who) + ": null input");
    if (B < 1) return fail(std::string(who) + ": B must be at least 1");
    if (beam_size < 1 || beam_size > 512) return fail(std::string(who) + ": beam_size must be in 1 .. 512");
    if (pool_cap < 1 || pool_cap > (1 << 24)) return fail(std::string(who) + ": pool_cap must be in 1 .. 2^24");
    CHK(nbest_sizes(who, beam_size, nbest, max_len, tokens_host, len_host, score_host_out, count_host));
    for (int b = 0; b < B; ++b) {
        if (n_live_host[b] < 0 || n_live_host[b] > beam_size)
            return fail(std::string(who) + ": n_live of utterance " + std::to_string(b) + " is outside 0 .. beam_size");
        for (int i = 0; i < n_live_host[b]; ++i)
            if (node_host[(size_t)b * beam_size + i] < 0 || node_host[(size_t)b * beam_size + i] >= pool_cap)
                return fail(std::string(who) + ": node " + std::to_string(i) + " of utterance " + std::to_string(b) +
                            " is outside the pool");
        for (int x = 1; x < pool_cap; ++x)
            if (pool_parent_host[(size_t)b * pool_cap + x] >= x)
                return fail(std::string(who) + ": the parent of pool node " + std::to_string(x) + " of utterance " + std::to_string(b) +
                            " is not below it");
    }
    if (!e) return fail("null engine");
    ENTER(e);
    // the search's own layouts: state_i [B][2 + 3 * beam], state_f [B][7 * beam], pool parent | ch [B][pool_cap] each
    const size_t ni = (size_t)B * (2 + 3 * beam_size), nf = (size_t)B * 7 * beam_size, np = (size_t)B * pool_cap;
    const size_t rows = (size_t)B * nbest;
    std::vector<int32_t> hi(ni, 0);
    std::vector<float> hf(nf, 0.f);
    for (int b = 0; b < B; ++b) {
        int32_t* si = hi.data() + (size_t)b * (2 + 3 * beam_size);
        float* sf = hf.data() + (size_t)b * 7 * beam_size;
        si[0] = n_live_host[b];
        for (int i = 0; i < n_live_host[b]; ++i) {
            si[2 + i] = node_host[(size_t)b * beam_size + i];
            si[2 + beam_size + i] = ch_host[(size_t)b * beam_size + i];
            sf[2 * beam_size + i] = score_host[(size_t)b * beam_size + i];
        }
    }
    struct Scratch {
        void* p = nullptr;
        ~Scratch() { if (p) (void)hipFree(p); }
    } dev;
    const size_t words = ni + nf + 2 * np + rows * max_len + 2 * rows + B;
    HIPCHK(hipMalloc(&dev.p, words * 4));
    int32_t* d_i = (int32_t*)dev.p;
    float* d_f = (float*)(d_i + ni);
    int32_t* d_pp = (int32_t*)(d_f + nf);
    int32_t* d_pc = d_pp + np;
    int32_t* d_tok = d_pc + np;
    int32_t* d_len = d_tok + rows * max_len;
    float* d_sc = (float*)(d_len + rows);
    int32_t* d_cnt = (int32_t*)(d_sc + rows);
    HIPCHK(hipMemcpy(d_i, hi.data(), ni * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_f, hf.data(), nf * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_pp, pool_parent_host, np * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_pc, pool_ch_host, np * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_tok, tokens_host, rows * max_len * 4, hipMemcpyHostToDevice));     // (tokens a row does not write stay as given)
    BeamNbestArgs a{};
    a.state_i = d_i; a.state_f = d_f; a.pool_parent = d_pp; a.pool_ch = d_pc;
    a.pool_cap = pool_cap; a.beam = beam_size; a.nbest = nbest; a.max_len = max_len;
    a.tokens = d_tok; a.len = d_len; a.score = d_sc; a.count = d_cnt;
    if (launch_beam_nbest(a, B, nullptr)) return fail(std::string(who) + ": launch rejected the sizes");
    LAUNCHCHK();
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(tokens_host, d_tok, rows * max_len * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(len_host, d_len, rows * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(score_host_out, d_sc, rows * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(count_host, d_cnt, B * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---- streaming beam search on the device (BeamSearchDecoder.decode_chunk / reset_decoder) -----------------------------
static void gbeam_args(GBeam& g, BeamGpuArgs& a) {
    a.pool_cap = g.cap;
    a.pool_parent = g.pool.as<int>();
    a.pool_ch = a.pool_parent + g.cap;
    beam_state_carve(g.state.p, 1, g.beam, &a.state_h, &a.state_i, &a.state_f);
}

int masr_gbeam_open(masr_engine* e, int32_t beam_size, int32_t blank, int32_t max_frames, int32_t* handle) {
    if (!e || !handle) return fail("null argument");
    ENTER(e);
    if (beam_size < 1 || beam_size > 512) return fail("beam_size must be in [1, 512]");
    if (max_frames <= 0) max_frames = 5000;
    int id = -1;
    for (size_t i = 0; i < e->gbeams.size(); ++i)
        if (!e->gbeams[i].open) { id = (int)i; break; }
    if (id < 0) {
        e->gbeams.emplace_back();
        id = (int)e->gbeams.size() - 1;
    }
    GBeam& g = e->gbeams[id];
    g.beam = beam_size;
    g.blank = blank;
    g.cap = max_frames * beam_size + 1;
    CHK(g.pool.ensure((size_t)g.cap * 2 * sizeof(int)));
    CHK(g.state.ensure(beam_state_bytes(beam_size)));
    g.lm = nullptr;
    g.alpha = g.beta = 0.f;
    g.open = true;
    g.started = false;
    *handle = id;
    return 0;
}

static int gbeam_of(masr_engine* e, int id, GBeam** out) {
    if (!e) return fail("null engine");
    if (id < 0 || id >= (int)e->gbeams.size() || !e->gbeams[id].open) return fail("bad beam handle");
    *out = &e->gbeams[id];
    return 0;
}

int masr_gbeam_set_lm(masr_engine* e, int32_t handle, masr_lm* lm, float alpha, float beta) {
    GBeam* g;
    CHK(gbeam_of(e, handle, &g));
    if (g->started) return fail("the language model of a stream can only change between utterances (after masr_gbeam_reset)");
    if (lm && lm_word_based(lm)) return fail("word-based language models are searched on host threads (masr_beam_*)");
    g->lm = lm;
    g->alpha = alpha;
    g->beta = beta;
    return 0;
}

int masr_gbeam_reset(masr_engine* e, int32_t handle) {
    GBeam* g;
    CHK(gbeam_of(e, handle, &g));
    g->started = false;
    return 0;
}

int masr_gbeam_close(masr_engine* e, int32_t handle) {
    GBeam* g;
    CHK(gbeam_of(e, handle, &g));
    ENTER(e);
    HIPCHK(hipDeviceSynchronize());
    g->pool.release();
    g->state.release();
    g->open = false;
    return 0;
}

int masr_gbeam_advance(masr_engine* e, int32_t handle, const int32_t* idx_dev, const float* logp_dev,
                       const int32_t* count_dev, int32_t T, int32_t K, int32_t* tokens_dev, int32_t max_len,
                       int32_t* len_dev, float* score_dev, void* stream) {
    return masr_gbeam_advance_lm(e, handle, idx_dev, logp_dev, count_dev, nullptr, T, K, tokens_dev, max_len, len_dev, score_dev,
                                 stream);
}

int masr_gbeam_advance_lm(masr_engine* e, int32_t handle, const int32_t* idx_dev, const float* logp_dev,
                          const int32_t* count_dev, const float* blank_logp_dev, int32_t T, int32_t K, int32_t* tokens_dev,
                          int32_t max_len, int32_t* len_dev, float* score_dev, void* stream) {
    GBeam* g;
    CHK(gbeam_of(e, handle, &g));
    ENTER(e);
    if (T < 0 || K > 64 || beam_gpu_lds_bytes(g->beam, K, g->lm != nullptr) > 160 * 1024)
        return fail("unsupported chunk / cutoff_top_n");
    BeamGpuArgs a{};
    a.cidx = idx_dev; a.clp = logp_dev; a.ccount = count_dev; a.frames = nullptr;
    a.blank_lp = g->lm ? blank_logp_dev : nullptr;
    a.T_stride = T; a.K = K; a.beam = g->beam; a.blank = g->blank; a.max_len = max_len;
    gbeam_args(*g, a);
    CHK(bind_lm(a, g->lm, g->alpha, g->beta));
    a.init = g->started ? 0 : 1;
    a.prof = nullptr;
    a.tokens = tokens_dev; a.len = len_dev; a.score = score_dev;
    // (the kernel stops allocating trie nodes at the pool capacity; max_frames bounds the utterance length)
    if (launch_beam_search(a, 1, (hipStream_t)stream)) return fail("beam search launch rejected the sizes");
    LAUNCHCHK();
    g->started = true;
    return 0;
}

int masr_gbeam_nbest(masr_engine* e, int32_t handle, int32_t nbest, int32_t* tokens_dev, int32_t max_len, int32_t* len_dev,
                     float* score_dev, int32_t* count_dev, void* stream) {
    GBeam* g;
    CHK(gbeam_of(e, handle, &g));
    if (!g->started)
        return fail("masr_gbeam_nbest: no masr_gbeam_advance since the stream was opened or reset: there is no live set to read");
    CHK(nbest_sizes("masr_gbeam_nbest", g->beam, nbest, max_len, tokens_dev, len_dev, score_dev, count_dev));
    ENTER(e);
    BeamGpuArgs s{};
    gbeam_args(*g, s);
    CHK(bind_lm(s, g->lm, g->alpha, g->beta));
    BeamNbestArgs a{};
    a.state_i = s.state_i; a.state_f = s.state_f; a.pool_parent = s.pool_parent; a.pool_ch = s.pool_ch;
    a.pool_cap = s.pool_cap; a.beam = g->beam; a.nbest = nbest; a.max_len = max_len;
    a.tokens = tokens_dev; a.len = len_dev; a.score = score_dev; a.count = count_dev;
    a.use_lm = s.use_lm; a.lm = s.lm; a.alpha = g->alpha; a.beta = g->beta;
    if (launch_beam_nbest(a, 1, (hipStream_t)stream)) return fail("masr_gbeam_nbest: launch rejected the sizes");
    LAUNCHCHK();
    return 0;
}

}  // extern "C"

namespace masr {
// the CTC head on the step's encoder rows: probabilities where the caller asks for them, argmax and its probability always.
// enc_out (masr_encode_chunk_enc): the rows the head read, copied out behind it (one device-to-device copy of rows x width floats)
int chunk_ctc(masr_engine* e, hipStream_t s, const float* enc, int rows, float* probs, int32_t* argmax, float* maxprob,
              float* enc_out) {
    if (e->cfg.vocab_size > 16384) return fail(kVocabRefusal);
    CHK(ctc_head(e, enc, rows, probs, probs ? 1 : 0, argmax, maxprob, s));
    if (enc_out) HIPCHK(hipMemcpyAsync(enc_out, enc, (size_t)rows * enc_dim(e) * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}
}  // namespace masr
