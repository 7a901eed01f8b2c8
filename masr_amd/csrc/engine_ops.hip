// libmasr_hip.so -- engine, single ops for the tests, the debug switches and the profile calls.  Host code only (file map: engine_state.h).
#include "engine_encoder.h"

using namespace masr;

extern "C" {

int masr_op_layernorm(masr_engine* e, const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev,
                      int32_t M, float eps, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    launch_layernorm(x_dev, w_dev, b_dev, y_dev, M, eps, 0, 0, nullptr, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

int masr_op_gemm(masr_engine* e, const float* a_dev, const float* w_dev, const float* bias_dev, const float* res_dev,
                 float* c_dev, int32_t M, int32_t N, int32_t K, int32_t act, float alpha, void* stream) {
    // (refused before the engine is touched: an unknown value used to run as "none")
    if (!gemm_act_valid(act))
        return fail("masr_op_gemm: act = " + std::to_string(act) + " is not an activation: 0 = none, 1 = relu, 2 = silu, 3 = gelu, "
                    "4 = tanh, 5 = hardtanh, 6 = selu");
    if (!e) return fail("null engine");
    ENTER(e);
    CallGuard call_guard(e, (hipStream_t)stream);
    if (K % 32) return fail("K must be a multiple of 32");
    gemm(e, (hipStream_t)stream, a_dev, K, w_dev, bias_dev, c_dev, N, M, N, K, act, alpha, res_dev, N);
    LAUNCHCHK();
    return 0;
}

}  // extern "C"

// masr_op_attention (pos_mode ATT_REL_POS) and masr_op_attention_plain (ATT_NO_POS: no table, no biases, group 1)
static int op_attention(masr_engine* e, int pos_mode, const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev,
                      const float* ptab_dev, int32_t n_pos, const float* bias_u_dev, const float* bias_v_dev, int32_t nseq,
                      const int64_t* q_off, const int64_t* k_off, const int64_t* v_off, const int64_t* out_off, const int32_t* nq,
                      const int32_t* nk, const int32_t* klen, const int32_t* pos0, const int32_t* q_abs0, int32_t heads,
                      int32_t q_stride, int32_t kv_stride, int32_t chunk_size, int32_t pos_stride, int32_t group, int32_t t_true,
                      void* stream) {
    // every refusal comes before the engine is touched: none of them needs a device
    const bool pos = pos_mode == ATT_REL_POS;
    if (!q_dev || !k_dev || !v_dev || !out_dev || (pos && (!ptab_dev || !bias_u_dev || !bias_v_dev)) || !q_off || !k_off || !v_off ||
        !out_off || !nq || !nk || !klen || !pos0 || !q_abs0)
        return fail("masr_op_attention: null argument");
    if (nseq <= 0) return fail("masr_op_attention: nseq must be positive");
    if (heads != 4 && heads != 8) return fail("masr_op_attention: heads must be 4 or 8");
    if (group != 1 && group != 3) return fail("masr_op_attention: group must be 1 or 3");
    const int w = heads * 64;
    if (q_stride < w || kv_stride < w) return fail("masr_op_attention: q_stride and kv_stride must be at least heads * 64");
    if (group == 3 && (heads != 4 || q_stride != 3 * w || kv_stride != 3 * w))
        return fail("masr_op_attention: the grouped kernels take 4 heads and planar rows of heads * 192 floats");
    if (chunk_size < 0 || pos_stride < 1 || n_pos < 0 || t_true < 0)
        return fail("masr_op_attention: chunk_size, n_pos and t_true must not be negative, pos_stride at least 1");
    if ((q_stride | kv_stride) & 3) return fail("masr_op_attention: strides must be multiples of 4 floats");
    for (const void* p : {(const void*)q_dev, (const void*)k_dev, (const void*)v_dev, (const void*)out_dev, (const void*)ptab_dev,
                          (const void*)bias_u_dev, (const void*)bias_v_dev})
        if ((uintptr_t)p & 15) return fail("masr_op_attention: device buffers must be 16-byte aligned");
    int max_nq = 0;
    std::vector<AttSeq> hs((size_t)nseq);
    for (int b = 0; b < nseq; ++b) {
        if (nq[b] < 0 || nk[b] < 0 || klen[b] < 0 || pos0[b] < 0 || q_abs0[b] < 0 || q_off[b] < 0 || k_off[b] < 0 || v_off[b] < 0 ||
            out_off[b] < 0)
            return fail("masr_op_attention: negative count or offset in sequence " + std::to_string(b));
        if (klen[b] > nk[b]) return fail("masr_op_attention: klen > nk in sequence " + std::to_string(b));
        if ((q_off[b] | k_off[b] | v_off[b] | out_off[b]) & 3)
            return fail("masr_op_attention: offsets must be multiples of 4 floats");
        if ((int64_t)nk[b] * kv_stride >= ((int64_t)1 << 30))
            return fail("masr_op_attention: the key rows of one sequence must span less than 4 GiB");
        // the last positional row a kernel may read: row pos0 + pos_stride * (nk - 1); grouped: frame pos0 + min(t_true, 3 nk) - 1
        const int64_t last = group == 3 ? (int64_t)pos0[b] + std::min<int64_t>(t_true, 3 * (int64_t)nk[b]) - 1
                                        : (int64_t)pos0[b] + (int64_t)pos_stride * (nk[b] - 1);
        if (pos && nk[b] > 0 && last >= n_pos) return fail("masr_op_attention: the positional table is too short for sequence " + std::to_string(b));
        AttSeq& a = hs[(size_t)b];
        a.q = q_dev + q_off[b];
        a.k = k_dev + k_off[b];
        a.v = v_dev + v_off[b];
        a.out = out_dev + out_off[b];
        a.nq = nq[b];
        a.nk = nk[b];
        a.klen = klen[b];
        a.pos0 = pos0[b];
        a.q_abs0 = q_abs0[b];
        a.pad_ = 0;
        max_nq = std::max(max_nq, nq[b]);
    }
    if (!e) return fail("null engine");
    ENTER(e);
    hipStream_t s = (hipStream_t)stream;
    struct Table {
        AttSeq* p = nullptr;
        ~Table() { if (p) (void)hipFree(p); }
    } tab;
    HIPCHK(hipMalloc((void**)&tab.p, hs.size() * sizeof(AttSeq)));
    HIPCHK(hipMemcpyAsync(tab.p, hs.data(), hs.size() * sizeof(AttSeq), hipMemcpyHostToDevice, s));
    {
        ProfScope ps(e, s, PROF_ATT, 6.0 * w * (double)max_nq * max_nq * nseq);
        if (group > 1) launch_attention_grouped(tab.p, nseq, max_nq, heads, group, ptab_dev, t_true, bias_u_dev, bias_v_dev, s, chunk_size);
        else launch_attention(tab.p, nseq, max_nq, heads, q_stride, kv_stride, ptab_dev, bias_u_dev, bias_v_dev, chunk_size, pos_stride, s, w, pos_mode);
    }
    LAUNCHCHK();
    HIPCHK(hipStreamSynchronize(s));       // the table is freed, and the host copy leaves scope, behind the kernel
    return 0;
}

extern "C" {

int masr_op_attention(masr_engine* e, const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev,
                      const float* ptab_dev, int32_t n_pos, const float* bias_u_dev, const float* bias_v_dev, int32_t nseq,
                      const int64_t* q_off, const int64_t* k_off, const int64_t* v_off, const int64_t* out_off, const int32_t* nq,
                      const int32_t* nk, const int32_t* klen, const int32_t* pos0, const int32_t* q_abs0, int32_t heads,
                      int32_t q_stride, int32_t kv_stride, int32_t chunk_size, int32_t pos_stride, int32_t group, int32_t t_true,
                      void* stream) {
    return op_attention(e, ATT_REL_POS, q_dev, k_dev, v_dev, out_dev, ptab_dev, n_pos, bias_u_dev, bias_v_dev, nseq, q_off, k_off, v_off,
                        out_off, nq, nk, klen, pos0, q_abs0, heads, q_stride, kv_stride, chunk_size, pos_stride, group, t_true, stream);
}

int masr_op_attention_plain(masr_engine* e, const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, int32_t nseq,
                            const int64_t* q_off, const int64_t* k_off, const int64_t* v_off, const int64_t* out_off,
                            const int32_t* nq, const int32_t* nk, const int32_t* klen, const int32_t* q_abs0, int32_t heads,
                            int32_t q_stride, int32_t kv_stride, int32_t chunk_size, int32_t pos_stride, void* stream) {
    if (nseq <= 0) return fail("masr_op_attention: nseq must be positive");
    const std::vector<int32_t> pos0((size_t)nseq, 0);         // (no positional rows: nothing is read at them)
    return op_attention(e, ATT_NO_POS, q_dev, k_dev, v_dev, out_dev, nullptr, 0, nullptr, nullptr, nseq, q_off, k_off, v_off, out_off, nq,
                        nk, klen, pos0.data(), q_abs0, heads, q_stride, kv_stride, chunk_size, pos_stride, 1, 0, stream);
}

int masr_debug_set(masr_engine* e, int32_t key, int32_t value) {
    if (!e) return fail("null engine");
    const KnobInfo* k = knob_find(key);
    if (k) {
        if (!MASR_EXPERIMENTS && k->experimental && value != 0)
            return fail("masr_debug_set: this key selects an experimental kernel that is not in this build (MASR_BUILD_EXPERIMENTS=1)");
        knob_set(key, value);
    } else if (key == 38) e->skip_padding = value;
    else if (key == 16) { e->prof_stride = value > 1 ? value : 1; e->prof_seen = 0; }
    else if (key == 2) {            // beam search phase profile of workgroup 0: value 1 = on, 0 = print + off
        if (value) {
            if (!e->beam_prof) {
                void* p = nullptr;
                HIPCHK(hipMalloc(&p, 16 * sizeof(long long)));
                e->owned.push_back(p);
                e->beam_prof = (long long*)p;
            }
        } else if (e->beam_prof) {
            long long h[16];
            HIPCHK(hipMemcpy(h, e->beam_prof, sizeof(h), hipMemcpyDeviceToHost));
            fprintf(stderr, "beam phases (cycles, last workgroup): setup+hash %lld  extensions %lld  prefixes+count %lld  select %lld  compact %lld\n",
                    h[0], h[1], h[2], h[3], h[4]);
            fprintf(stderr, "  narrow step (%lld frames): tables+candidates %lld  hash+contexts %lld  children+scorer table %lld  extensions %lld  "
                    "prefixes+select %lld  scan %lld  survivors %lld  new prefixes %lld\n", h[5], h[6], h[7], h[8], h[9], h[10], h[11], h[12], h[13]);
            if (h[15] > 0) fprintf(stderr, "  wide step (%lld frames): %.1f distinct scorer contexts per frame\n", h[15], (double)h[14] / (double)h[15]);
            e->beam_prof = nullptr;
        }
    }
    else return fail("unknown debug key");
    return 0;
}

int masr_debug_reset(masr_engine* e) {
    if (!e) return fail("null engine");
    knobs_reset();
    e->skip_padding = 7;
    e->prof_stride = 1;
    e->prof_seen = 0;
    return 0;
}

int masr_debug_key_info(int32_t index, int32_t* key, int32_t* default_value, int32_t* experimental, const char** name) {
    const KnobInfo* k = knob_info(index);
    if (!k) return 1;
    if (key) *key = k->key;
    if (default_value) *default_value = knob_default(*k);
    if (experimental) *experimental = k->experimental;
    if (name) *name = k->name;
    return 0;
}

int masr_ffn_plan(int32_t d_model, int32_t d_ff, int32_t m, const int32_t* ask, const int32_t* overrides, int32_t n_overrides,
                  int32_t* plan) {
    if (!ask || !plan || n_overrides < 0 || (n_overrides && !overrides)) return fail("masr_ffn_plan: null argument");
    if (d_ff <= 0 || d_ff % 128 || m <= 0) return fail("masr_ffn_plan: d_ff must be a positive multiple of 128 and m positive");
    Knobs k;                       // the defaults; the process's switches are neither read nor written
    for (int i = 0; i < n_overrides; ++i)
        if (!knob_set(overrides[2 * i], overrides[2 * i + 1], k))
            return fail("masr_ffn_plan: no process-wide switch has key " + std::to_string(overrides[2 * i]));
    const FfnPlan p = ffn_plan(k, d_model, d_ff, m, {ask[0], ask[1], ask[2], ask[3], ask[4]});
    const int32_t out[9] = {p.kernel, p.nsplit, p.cpb, p.ny, p.packed, p.tail_in_kernel, p.head_in_kernel, p.split_head, p.prof};
    std::copy(out, out + 9, plan);
    return 0;
}

int masr_profile_select(masr_engine* e, int32_t kind) {
    if (!e) return fail("null engine");
    e->prof_kind = kind;
    return 0;
}

int masr_profile_read(masr_engine* e, double* total_ms, int64_t* launches, double* flops, int32_t reset) {
    if (!e) return fail("null engine");
    ENTER(e);
    double tot = 0.0;
    for (size_t i = 0; i < e->prof_used; ++i) {
        HIPCHK(hipEventSynchronize(e->prof_events[i].second));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e->prof_events[i].first, e->prof_events[i].second));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = (int64_t)e->prof_used;
    if (flops) *flops = e->prof_flops;
    if (reset) {
        e->prof_used = 0;
        e->prof_flops = 0.0;
    }
    return 0;
}

}  // extern "C"
