// libmasr_hip.so -- engine: the attention decoder of the second pass, host side (kernels: decoder.hip, decoder_step.hip,
// decoder_joint.hip).
#include <math.h>
#include <cmath>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "engine_state.h"

using namespace masr;

// ------------------------------------------------------------------------------------------------
// Attention decoder of the second pass (decoder: attention_rescoring): weights + masr_rescore
// reference: masr/model_utils/transformer/decoder.py (BiTransformerDecoder, TransformerDecoder, DecoderLayer)
// ------------------------------------------------------------------------------------------------
static int finalize_decoder_side(masr_engine* e, const std::string& pre, const char* conf_key, int nl, DecoderW& w) {
    const int d = e->cfg.d_model, V = e->cfg.vocab_size, dff = e->dec.dff;
    auto upn = [&](const std::string& name, std::vector<int64_t> shape, float** out) -> int {
        const HostTensor* t;
        CHK(get(e, name, shape, &t));
        e->dec.weight_bytes += t->v.size() * sizeof(float);
        return upload(e, t->v, out);
    };
    // rows of several [rows, cols] tensors one under the other (fused projections)
    auto cat = [&](std::vector<std::string> names, int rows, int cols, float** out) -> int {
        std::vector<float> v;
        for (const std::string& n : names) {
            const HostTensor* t;
            CHK(get(e, n, cols ? std::vector<int64_t>{rows, cols} : std::vector<int64_t>{rows}, &t));
            v.insert(v.end(), t->v.begin(), t->v.end());
        }
        e->dec.weight_bytes += v.size() * sizeof(float);
        return upload(e, v, out);
    };
    const std::string beyond = pre + "decoders." + std::to_string(nl) + ".norm1.weight";
    if (e->host.count(beyond))
        return fail(std::string("decoder_conf.") + conf_key + "=" + std::to_string(nl) + " but the checkpoint holds " + beyond +
                    " (it was trained with more blocks)");
    w.layers.assign(nl, DecLayerW{});
    if (nl == 0) return 0;
    CHK(upn(pre + "embed.0.weight", {V, d}, &w.emb));
    for (int i = 0; i < nl; ++i) {
        const std::string p = pre + "decoders." + std::to_string(i) + ".";
        if (!e->host.count(p + "norm1.weight"))
            return fail(std::string("decoder_conf.") + conf_key + "=" + std::to_string(nl) + " but the checkpoint has no " + p +
                        "norm1.weight (it was trained with fewer blocks)");
        DecLayerW& l = w.layers[i];
        CHK(upn(p + "norm1.weight", {d}, &l.n1w));
        CHK(upn(p + "norm1.bias", {d}, &l.n1b));
        CHK(cat({p + "self_attn.linear_q.weight", p + "self_attn.linear_k.weight", p + "self_attn.linear_v.weight"}, d, d, &l.wqkv));
        CHK(cat({p + "self_attn.linear_q.bias", p + "self_attn.linear_k.bias", p + "self_attn.linear_v.bias"}, d, 0, &l.bqkv));
        CHK(upn(p + "self_attn.linear_out.weight", {d, d}, &l.wo));
        CHK(upn(p + "self_attn.linear_out.bias", {d}, &l.bo));
        CHK(upn(p + "norm2.weight", {d}, &l.n2w));
        CHK(upn(p + "norm2.bias", {d}, &l.n2b));
        CHK(upn(p + "src_attn.linear_q.weight", {d, d}, &l.wq2));
        CHK(upn(p + "src_attn.linear_q.bias", {d}, &l.bq2));
        CHK(cat({p + "src_attn.linear_k.weight", p + "src_attn.linear_v.weight"}, d, d, &l.wkv2));
        CHK(cat({p + "src_attn.linear_k.bias", p + "src_attn.linear_v.bias"}, d, 0, &l.bkv2));
        CHK(upn(p + "src_attn.linear_out.weight", {d, d}, &l.wo2));
        CHK(upn(p + "src_attn.linear_out.bias", {d}, &l.bo2));
        CHK(upn(p + "norm3.weight", {d}, &l.n3w));
        CHK(upn(p + "norm3.bias", {d}, &l.n3b));
        auto b1 = e->host.find(p + "feed_forward.w_1.bias");
        if (b1 != e->host.end() && (int64_t)b1->second.v.size() != dff)
            return fail("decoder_conf.linear_units=" + std::to_string(dff) + " but the checkpoint was trained with linear_units=" +
                        std::to_string(b1->second.v.size()) + " (" + p + "feed_forward.w_1.bias)");
        CHK(upn(p + "feed_forward.w_1.weight", {dff, d}, &l.w1));
        CHK(upn(p + "feed_forward.w_1.bias", {dff}, &l.b1));
        CHK(upn(p + "feed_forward.w_2.weight", {d, dff}, &l.w2));
        CHK(upn(p + "feed_forward.w_2.bias", {d}, &l.b2));
    }
    CHK(upn(pre + "after_norm.weight", {d}, &w.after_w));
    CHK(upn(pre + "after_norm.bias", {d}, &w.after_b));
    CHK(upn(pre + "output_layer.weight", {V, d}, &w.out_w));
    CHK(upn(pre + "output_layer.bias", {V}, &w.out_b));
    return 0;
}

namespace masr {
int finalize_decoder(masr_engine* e) {
    HIPCHK(hipSetDevice(e->cfg.device_id));
    bool any = false;
    for (const auto& kv : e->host) any = any || kv.first.rfind("decoder.left_decoder.", 0) == 0;
    if (!any) {
        if (e->dec.ready) return 0;        // a reload of encoder tensors only: the decoder weights stay as they are
        return fail("attention_rescoring: the checkpoint holds no decoder.left_decoder.* tensors (it has no attention decoder)");
    }
    // a reload replaces the whole set: the previous weights are freed once the device has drained (launches in flight may
    // still read them), and a finalize that fails midway leaves no half-filled decoder behind
    auto drop = [&]() {
        for (void* p : e->dec.owned) (void)hipFree(p);
        e->dec.owned.clear();
        e->dec.left = DecoderW{};
        e->dec.right = DecoderW{};
        e->dec.weight_bytes = 0;
        e->dec.ready = false;
    };
    if (!e->dec.owned.empty()) (void)hipDeviceSynchronize();
    drop();
    const size_t n0 = e->owned.size();
    int rc = finalize_decoder_side(e, "decoder.left_decoder.", "num_blocks", e->dec.nl, e->dec.left);
    if (!rc) rc = finalize_decoder_side(e, "decoder.right_decoder.", "r_num_blocks", e->dec.nr, e->dec.right);
    e->dec.owned.assign(e->owned.begin() + n0, e->owned.end());       // (upload() files every allocation under e->owned)
    e->owned.resize(n0);
    if (rc) {
        drop();
        return rc;
    }
    e->dec.ready = true;
    return 0;
}
}  // namespace masr

namespace {

// where the source k | v projection finds the encoder frames: frame t of utterance b is row b * Tp + t of the dense block enc, or
// (table given: masr_rescore_rows) row table[b * Tp + t] of the row pool enc [n_rows, d]
struct EncSource {
    const float* enc;
    const int64_t* table = nullptr;
    int64_t n_rows = 0;
};

// one TransformerDecoder over the hypothesis table -> out [B * N] (reverse: the right-to-left decoder's view of the table)
int decoder_forward(masr_engine* e, hipStream_t s, const DecoderW& w, int reverse, const EncSource& src, const int* enc_lens, int B,
                    int Tp, const int* hyp, const int* hyp_lens, int N, int Lmax, float* out) {
    const int d = e->cfg.d_model, V = e->cfg.vocab_size, dff = e->dec.dff, H = e->dec.heads;
    const int S = B * N, Lp = Lmax + 1, M = S * Lp, Mk = B * Tp;
    float *x = e->dec_x.as<float>(), *ln = e->dec_ln.as<float>(), *qkv = e->dec_qkv.as<float>(), *att = e->dec_att.as<float>(),
          *kv = e->dec_kv.as<float>(), *hid = e->dec_hid.as<float>(), *logits = e->dec_logits.as<float>();
    const float eps = 1e-12f;          // nn.LayerNorm(size, eps=1e-12) throughout the decoder (decoder.py:173, 308-310)
    launch_dec_embed(hyp, hyp_lens, w.emb, e->pe, x, S, Lmax, d, V, reverse, s);
    for (const DecLayerW& l : w.layers) {
        // x <- x + Wo . self_attn(norm1(x)), causal over the hypothesis' own rows
        WIDECHK(PROF_WIDE_LN, launch_layernorm_wide(x, l.n1w, l.n1b, ln, M, d, eps, 0, 0, nullptr, s));
        gemm(e, s, ln, d, l.wqkv, l.bqkv, qkv, 3 * d, M, 3 * d, d, ACT_NONE, 1.f, nullptr, 0);
        launch_dec_attention(qkv, 3 * d, qkv + d, qkv + 2 * d, 3 * d, att, d, hyp_lens, nullptr, S, N, Lmax, Tp, H, 1, s);
        gemm(e, s, att, d, l.wo, l.bo, x, d, M, d, d, ACT_NONE, 1.f, x, d);
        // x <- x + Wo . src_attn(norm2(x), memory): k | v of the utterance's encoder frames projected ONCE for its N hypotheses
        WIDECHK(PROF_WIDE_LN, launch_layernorm_wide(x, l.n2w, l.n2b, ln, M, d, eps, 0, 0, nullptr, s));
        gemm(e, s, ln, d, l.wq2, l.bq2, qkv, d, M, d, d, ACT_NONE, 1.f, nullptr, 0);
        if (src.table) gemm_rows(e, s, src.enc, d, src.table, src.n_rows, l.wkv2, l.bkv2, kv, 2 * d, Mk, 2 * d, d);
        else gemm(e, s, src.enc, d, l.wkv2, l.bkv2, kv, 2 * d, Mk, 2 * d, d, ACT_NONE, 1.f, nullptr, 0);
        launch_dec_attention(qkv, d, kv, kv + d, 2 * d, att, d, hyp_lens, enc_lens, S, N, Lmax, Tp, H, 0, s);
        gemm(e, s, att, d, l.wo2, l.bo2, x, d, M, d, d, ACT_NONE, 1.f, x, d);
        // x <- x + W2 . relu(W1 . norm3(x))
        WIDECHK(PROF_WIDE_LN, launch_layernorm_wide(x, l.n3w, l.n3b, ln, M, d, eps, 0, 0, nullptr, s));
        gemm(e, s, ln, d, l.w1, l.b1, hid, dff, M, dff, d, ACT_RELU, 1.f, nullptr, 0);
        gemm(e, s, hid, dff, l.w2, l.b2, x, d, M, d, dff, ACT_NONE, 1.f, x, d);
    }
    WIDECHK(PROF_WIDE_LN, launch_layernorm_wide(x, w.after_w, w.after_b, ln, M, d, eps, 0, 0, nullptr, s));
    gemm(e, s, ln, d, w.out_w, w.out_b, logits, V, M, V, d, ACT_NONE, 1.f, nullptr, 0);
    launch_dec_scores(logits, hyp, hyp_lens, e->dec_rowlp.as<float>(), out, S, Lmax, V, reverse, s);
    return 0;
}

// what needs no device: refused before the engine is touched
int rescore_shape_check(const char* who, const void* enc, const void* enc_lens, int B, int Tp, const void* hyp, const void* hyp_lens,
                        int N, int Lmax, const void* att, const void* r_att) {
    const std::string w(who);
    if (!enc || !enc_lens || !hyp || !hyp_lens || !att || !r_att) return fail(w + ": null argument");
    if (B <= 0 || Tp <= 0) return fail(w + ": B and Tp must be positive");
    if (N < 1 || N > 64) return fail(w + ": N = " + std::to_string(N) + " hypotheses per utterance is outside 1 .. 64 (beam_size)");
    if (Lmax < 1) return fail(w + ": Lmax must be at least 1");
    if ((int64_t)B * N > 65535) return fail(w + ": B * N must not exceed 65535 sequences per call");
    return 0;
}

int rescore_impl(masr_engine* e, const char* who, const EncSource& src, const int* enc_lens, int B, int Tp, const int* hyp,
                 const int* hyp_lens, int N, int Lmax, int with_right, float* att, float* r_att, hipStream_t s) {
    const std::string w(who);
    if (!e->dec.enabled || !e->dec.ready)
        return fail(w + ": this engine holds no attention decoder (masr_decoder_enable before masr_finalize)");
    if (Lmax > e->cfg.max_pos - 1)
        return fail(w + ": hypotheses longer than max_pos - 1 = " + std::to_string(e->cfg.max_pos - 1) +
                    " tokens have no positional rows (Lmax = " + std::to_string(Lmax) + ")");
    if (with_right && e->dec.nr == 0)
        return fail(w + ": reverse_weight > 0 needs the right-to-left decoder, and this checkpoint has none (r_num_blocks: 0)");
    const int d = e->cfg.d_model, V = e->cfg.vocab_size;
    const size_t M = (size_t)B * N * (Lmax + 1), f = sizeof(float);
    CHK(e->dec_x.ensure(M * d * f));
    CHK(e->dec_ln.ensure(M * d * f));
    CHK(e->dec_qkv.ensure(M * 3 * d * f));
    CHK(e->dec_att.ensure(M * d * f));
    CHK(e->dec_kv.ensure((size_t)B * Tp * 2 * d * f));
    CHK(e->dec_hid.ensure(M * e->dec.dff * f));
    CHK(e->dec_logits.ensure(M * V * f));
    CHK(e->dec_rowlp.ensure(M * f));
    CHK(decoder_forward(e, s, e->dec.left, 0, src, enc_lens, B, Tp, hyp, hyp_lens, N, Lmax, att));
    if (with_right) CHK(decoder_forward(e, s, e->dec.right, 1, src, enc_lens, B, Tp, hyp, hyp_lens, N, Lmax, r_att));
    else HIPCHK(hipMemsetAsync(r_att, 0, (size_t)B * N * f, s));
    LAUNCHCHK();
    return 0;
}

}  // namespace

extern "C" {

int masr_decoder_enable(masr_engine* e, int32_t attention_heads, int32_t linear_units, int32_t num_blocks, int32_t r_num_blocks) {
    if (attention_heads != 4 && attention_heads != 8)
        return fail("decoder_conf.attention_heads=" + std::to_string(attention_heads) + " is not supported: output_size / 64 (4 at "
                    "256, 8 at 512; the decoder's attention kernel runs heads of 64)");
    if (linear_units <= 0 || linear_units % 32)
        return fail("decoder_conf.linear_units=" + std::to_string(linear_units) + " is not supported: a positive multiple of 32");
    if (num_blocks < 1) return fail("decoder_conf.num_blocks=" + std::to_string(num_blocks) + " is not supported: at least 1");
    if (r_num_blocks < 0) return fail("decoder_conf.r_num_blocks=" + std::to_string(r_num_blocks) + " is not supported: 0 or more");
    if (!e) return fail("null engine");
    if (e->cfg.model_kind == 3)
        return fail("attention_rescoring: use_model deepspeech2 has no attention decoder (its decoder.* tensors are the CTC head)");
    if (!wide_supported(e->cfg.d_model) || e->cfg.d_model != attention_heads * 64)
        return fail("decoder_conf.attention_heads=" + std::to_string(attention_heads) + " is not supported at output_size " +
                    std::to_string(e->cfg.d_model) + ": output_size / 64 heads, output_size 256 or 512");
    if (e->finalized) return fail("masr_decoder_enable: call it before masr_load_tensor / masr_finalize");
    e->dec.enabled = true;
    e->dec.heads = attention_heads;
    e->dec.dff = linear_units;
    e->dec.nl = num_blocks;
    e->dec.nr = r_num_blocks;
    return 0;
}

int masr_rescore(masr_engine* e, const float* enc_dev, const int32_t* enc_lens_dev, int32_t B, int32_t Tp, const int32_t* hyp_dev,
                 const int32_t* hyp_lens_dev, int32_t N, int32_t Lmax, int32_t with_right, float* att_dev, float* r_att_dev,
                 void* stream) {
    CHK(rescore_shape_check("masr_rescore", enc_dev, enc_lens_dev, B, Tp, hyp_dev, hyp_lens_dev, N, Lmax, att_dev, r_att_dev));
    if (!e || !e->finalized) return fail("engine not finalized");
    ENTER(e);
    CallGuard call_guard(e, (hipStream_t)stream);
    return rescore_impl(e, "masr_rescore", EncSource{enc_dev}, enc_lens_dev, B, Tp, hyp_dev, hyp_lens_dev, N, Lmax, with_right, att_dev,
                        r_att_dev, (hipStream_t)stream);
}

int masr_rescore_rows(masr_engine* e, const float* rows_dev, int64_t n_rows, const int64_t* frame_row_dev, const int32_t* n_frames_dev,
                      int32_t B, int32_t Tmax, const int32_t* hyp_dev, const int32_t* hyp_lens_dev, int32_t N, int32_t Lmax,
                      int32_t with_right, float* att_dev, float* r_att_dev, void* stream) {
    // (the sizes first: an empty pool or table has no address to give)
    if (n_rows <= 0) return fail("masr_rescore_rows: n_rows = " + std::to_string(n_rows) + " must be positive");
    if (Tmax < 1) return fail("masr_rescore_rows: Tmax = " + std::to_string(Tmax) + " must be at least 1");
    if (!frame_row_dev) return fail("masr_rescore_rows: null argument");
    CHK(rescore_shape_check("masr_rescore_rows", rows_dev, n_frames_dev, B, Tmax, hyp_dev, hyp_lens_dev, N, Lmax, att_dev, r_att_dev));
    if ((int64_t)B * Tmax > INT32_MAX) return fail("masr_rescore_rows: B * Tmax must not exceed 2^31 - 1 table entries");
    if (!e || !e->finalized) return fail("engine not finalized");
    ENTER(e);
    CallGuard call_guard(e, (hipStream_t)stream);
    EncSource src{rows_dev};
    src.table = frame_row_dev;
    src.n_rows = n_rows;
    return rescore_impl(e, "masr_rescore_rows", src, n_frames_dev, B, Tmax, hyp_dev, hyp_lens_dev, N, Lmax, with_right, att_dev, r_att_dev,
                        (hipStream_t)stream);
}

int masr_op_decoder_scores(masr_engine* e, const float* enc_dev, const int32_t* enc_lens_host, int32_t B, int32_t Tp,
                           const int32_t* hyp_host, const int32_t* hyp_lens_host, int32_t N, int32_t Lmax, int32_t with_right,
                           float* att_host, float* r_att_host, void* stream) {
    CHK(rescore_shape_check("masr_op_decoder_scores", enc_dev, enc_lens_host, B, Tp, hyp_host, hyp_lens_host, N, Lmax, att_host,
                            r_att_host));
    for (int b = 0; b < B; ++b)
        if (enc_lens_host[b] < 1 || enc_lens_host[b] > Tp)
            return fail("masr_op_decoder_scores: utterance " + std::to_string(b) + " has " + std::to_string(enc_lens_host[b]) +
                        " encoder frames, outside 1 .. Tp");
    for (int s = 0; s < B * N; ++s)
        if (hyp_lens_host[s] < 0 || hyp_lens_host[s] > Lmax)
            return fail("masr_op_decoder_scores: hypothesis " + std::to_string(s) + " has length " + std::to_string(hyp_lens_host[s]) +
                        ", outside 0 .. Lmax");
    if (!e || !e->finalized) return fail("engine not finalized");
    const int V = e->cfg.vocab_size;
    for (int s = 0; s < B * N; ++s)
        for (int i = 0; i < hyp_lens_host[s]; ++i) {
            const int t = hyp_host[(size_t)s * Lmax + i];
            if (t < 0 || t >= V)
                return fail("masr_op_decoder_scores: token id " + std::to_string(t) + " of hypothesis " + std::to_string(s) +
                            " is outside the vocabulary");
        }
    ENTER(e);
    hipStream_t st = (hipStream_t)stream;
    CallGuard call_guard(e, st);
    const size_t S = (size_t)B * N;
    struct Table {
        int* p = nullptr;
        ~Table() { if (p) (void)hipFree(p); }
    } tab;
    // hyp [S, Lmax] | hyp_lens [S] | enc_lens [B] | att [S] | r_att [S] (the last two as float)
    const size_t n_int = S * Lmax + S + B, n_all = n_int + 2 * S;
    HIPCHK(hipMalloc((void**)&tab.p, n_all * sizeof(int)));
    int *hyp_d = tab.p, *len_d = hyp_d + S * Lmax, *enc_d = len_d + S;
    float *att_d = reinterpret_cast<float*>(enc_d + B), *ratt_d = att_d + S;
    HIPCHK(hipMemcpyAsync(hyp_d, hyp_host, S * Lmax * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(len_d, hyp_lens_host, S * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(enc_d, enc_lens_host, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
    CHK(rescore_impl(e, "masr_rescore", EncSource{enc_dev}, enc_d, B, Tp, hyp_d, len_d, N, Lmax, with_right, att_d, ratt_d, st));
    HIPCHK(hipMemcpyAsync(att_host, att_d, S * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(r_att_host, ratt_d, S * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// decoder: attention -- left-to-right beam search with the LEFT decoder alone, one new row per hypothesis and step
// (forward_one_step, transformer/decoder.py:233-270; the kernels and the cache layout: decoder_step.hip)
// ------------------------------------------------------------------------------------------------
namespace {

struct StepPlan {
    int B, N, S, Tp, Lcap, Lrun, max_len;
    int *tok[2], *anc[2], *done, *active;
    float* score[2];
};

// steps the host may have to launch: no utterance runs longer (enc_lens <= Tp)
int step_run_bound(const masr_engine* e, int Tp, int Lcap, int max_len) {
    int r = std::min(std::min(Tp, Lcap), e->cfg.max_pos - 1);
    if (max_len > 0) r = std::min(r, max_len);
    return std::max(r, 1);
}

int step_workspaces(masr_engine* e, StepPlan& pl, int topn) {
    const int d = e->cfg.d_model, V = e->cfg.vocab_size, nl = e->dec.nl;
    const size_t S = (size_t)pl.S, f = sizeof(float);
    CHK(e->st_x.ensure(S * d * f));
    CHK(e->st_ln.ensure(S * d * f));
    CHK(e->st_q.ensure(S * d * f));
    CHK(e->st_att.ensure(S * d * f));
    CHK(e->st_hid.ensure(S * e->dec.dff * f));
    CHK(e->st_logits.ensure(S * V * f));
    CHK(e->st_cache.ensure((size_t)nl * pl.Lrun * S * 2 * d * f));
    CHK(e->st_src.ensure((size_t)nl * pl.B * pl.Tp * 2 * d * f));
    CHK(e->st_top.ensure(S * topn * (f + sizeof(int))));
    // tok[2] | anc[2] [S, Lcap], score[2] [S], done [B], active [1]
    const size_t tab = S * pl.Lcap;
    CHK(e->st_tab.ensure((4 * tab + 2 * S + pl.B + 1) * sizeof(int)));
    int* t = e->st_tab.as<int>();
    pl.tok[0] = t;
    pl.tok[1] = t + tab;
    pl.anc[0] = t + 2 * tab;
    pl.anc[1] = t + 3 * tab;
    pl.score[0] = reinterpret_cast<float*>(t + 4 * tab);
    pl.score[1] = pl.score[0] + S;
    pl.done = t + 4 * tab + 2 * S;
    pl.active = pl.done + pl.B;
    return 0;
}

// source k | v of every block: ONE GEMM per utterance batch and layer, before the loop
void step_source_kv(masr_engine* e, hipStream_t s, const float* enc, const StepPlan& pl) {
    const int d = e->cfg.d_model, Mk = pl.B * pl.Tp;
    float* src = e->st_src.as<float>();
    for (size_t i = 0; i < e->dec.left.layers.size(); ++i) {
        const DecLayerW& l = e->dec.left.layers[i];
        gemm(e, s, enc, d, l.wkv2, l.bkv2, src + i * (size_t)Mk * 2 * d, 2 * d, Mk, 2 * d, d, ACT_NONE, 1.f, nullptr, 0);
    }
}

// position p of every row: embedding, the blocks (the new k | v written straight into cache slab p), after_norm, output layer,
// log_softmax + top n.  full / only_pos: the teacher-forced op's outputs (launch_step_topn)
int step_forward(masr_engine* e, hipStream_t s, const StepPlan& pl, int p, const int* tok, const int* anc, const int* enc_lens,
                 int topn, float* full, const int* only_pos) {
    const DecoderW& w = e->dec.left;
    const int d = e->cfg.d_model, V = e->cfg.vocab_size, dff = e->dec.dff, H = e->dec.heads, S = pl.S;
    float *x = e->st_x.as<float>(), *ln = e->st_ln.as<float>(), *q = e->st_q.as<float>(), *att = e->st_att.as<float>(),
          *hid = e->st_hid.as<float>(), *logits = e->st_logits.as<float>();
    const float eps = 1e-12f;
    launch_step_embed(tok, w.emb, e->pe, x, S, p, pl.Lcap, d, V, s);
    for (size_t i = 0; i < w.layers.size(); ++i) {
        const DecLayerW& l = w.layers[i];
        float* cache = e->st_cache.as<float>() + i * (size_t)pl.Lrun * S * 2 * d;
        const float* src = e->st_src.as<float>() + i * (size_t)pl.B * pl.Tp * 2 * d;
        // x <- x + Wo . self_attn(norm1(x)): q of the new row; its k | v (rows d .. 3 d of the fused projection) appended as slab p
        WIDECHK(PROF_WIDE_LN, launch_layernorm_wide(x, l.n1w, l.n1b, ln, S, d, eps, 0, 0, nullptr, s));
        gemm(e, s, ln, d, l.wqkv, l.bqkv, q, d, S, d, d, ACT_NONE, 1.f, nullptr, 0);
        gemm(e, s, ln, d, l.wqkv + (size_t)d * d, l.bqkv + d, cache + (size_t)p * S * 2 * d, 2 * d, S, 2 * d, d, ACT_NONE, 1.f, nullptr, 0);
        launch_step_attention(q, d, cache, att, anc, nullptr, S, pl.N, pl.Tp, pl.Lcap, p, d, H, s);
        gemm(e, s, att, d, l.wo, l.bo, x, d, S, d, d, ACT_NONE, 1.f, x, d);
        // x <- x + Wo . src_attn(norm2(x), memory)
        WIDECHK(PROF_WIDE_LN, launch_layernorm_wide(x, l.n2w, l.n2b, ln, S, d, eps, 0, 0, nullptr, s));
        gemm(e, s, ln, d, l.wq2, l.bq2, q, d, S, d, d, ACT_NONE, 1.f, nullptr, 0);
        launch_step_attention(q, d, src, att, nullptr, enc_lens, S, pl.N, pl.Tp, pl.Lcap, p, d, H, s);
        gemm(e, s, att, d, l.wo2, l.bo2, x, d, S, d, d, ACT_NONE, 1.f, x, d);
        // x <- x + W2 . relu(W1 . norm3(x))
        WIDECHK(PROF_WIDE_LN, launch_layernorm_wide(x, l.n3w, l.n3b, ln, S, d, eps, 0, 0, nullptr, s));
        gemm(e, s, ln, d, l.w1, l.b1, hid, dff, S, dff, d, ACT_RELU, 1.f, nullptr, 0);
        gemm(e, s, hid, dff, l.w2, l.b2, x, d, S, d, dff, ACT_NONE, 1.f, x, d);
    }
    WIDECHK(PROF_WIDE_LN, launch_layernorm_wide(x, w.after_w, w.after_b, ln, S, d, eps, 0, 0, nullptr, s));
    gemm(e, s, ln, d, w.out_w, w.out_b, logits, V, S, V, d, ACT_NONE, 1.f, nullptr, 0);
    float* top_v = e->st_top.as<float>();
    int* top_i = reinterpret_cast<int*>(top_v + (size_t)S * topn);
    launch_step_topn(logits, S, V, topn, top_v, top_i, full, only_pos, p, s);
    return 0;
}

int step_shape_check(const masr_engine* e, const char* who, int B, int Tp, int N, int Lcap) {
    const std::string w(who);
    if (B <= 0 || Tp <= 0) return fail(w + ": B and Tp must be positive");
    if (N < 1 || N > 64) return fail(w + ": beam_size = " + std::to_string(N) + " is outside 1 .. 64");
    if (Lcap < 1) return fail(w + ": Lcap must be at least 1");
    if ((int64_t)B * N > 65535) return fail(w + ": B * beam_size must not exceed 65535 hypotheses per call");
    if (!e || !e->finalized) return fail("engine not finalized");
    if (!e->dec.enabled || !e->dec.ready)
        return fail(w + ": this engine holds no attention decoder (masr_decoder_enable before masr_finalize)");
    if (N > e->cfg.vocab_size)
        return fail(w + ": beam_size = " + std::to_string(N) + " exceeds the vocabulary of " + std::to_string(e->cfg.vocab_size));
    return 0;
}

// end poll of masr_attention_decode: every MASR_ATTENTION_POLL steps (default 8; 0 = never) the host reads the count of
// utterances still running and stops launching at 0.  The results do not depend on it.
int step_poll_every() {
    const char* v = getenv("MASR_ATTENTION_POLL");
    if (!v || !*v) return 8;
    const int n = atoi(v);
    return n < 0 ? 0 : n;
}

}  // namespace

extern "C" {

int masr_attention_decode(masr_engine* e, const float* enc_dev, const int32_t* enc_lens_dev, int32_t B, int32_t Tp, int32_t beam_size,
                          int32_t max_len, int32_t* tokens_dev, int32_t Lcap, int32_t* lens_dev, float* scores_dev,
                          int32_t* steps_host_or_null, void* stream) {
    if (!enc_dev || !enc_lens_dev || !tokens_dev || !lens_dev || !scores_dev) return fail("masr_attention_decode: null argument");
    if (max_len < 0) return fail("masr_attention_decode: max_len must be 0 (no limit of its own) or positive");
    CHK(step_shape_check(e, "masr_attention_decode", B, Tp, beam_size, Lcap));
    ENTER(e);
    hipStream_t st = (hipStream_t)stream;
    CallGuard call_guard(e, st);
    StepPlan pl{};
    pl.B = B; pl.N = beam_size; pl.S = B * beam_size; pl.Tp = Tp; pl.Lcap = Lcap; pl.max_len = max_len;
    pl.Lrun = step_run_bound(e, Tp, Lcap, max_len);
    CHK(step_workspaces(e, pl, pl.N));
    const int V = e->cfg.vocab_size, poll = step_poll_every();
    launch_step_init(pl.score[0], pl.done, pl.active, enc_lens_dev, B, pl.N, Tp, Lcap, max_len, e->cfg.max_pos, st);
    step_source_kv(e, st, enc_dev, pl);
    float* top_v = e->st_top.as<float>();
    int cur = 0, steps = 0;
    for (int p = 0; p < pl.Lrun; ++p) {
        CHK(step_forward(e, st, pl, p, pl.tok[cur], pl.anc[cur], enc_lens_dev, pl.N, nullptr, nullptr));
        StepMerge m{};
        m.top_v = top_v; m.top_i = reinterpret_cast<const int*>(top_v + (size_t)pl.S * pl.N);
        m.score_cur = pl.score[cur]; m.score_next = pl.score[cur ^ 1];
        m.tok_cur = pl.tok[cur]; m.tok_next = pl.tok[cur ^ 1]; m.anc_cur = pl.anc[cur]; m.anc_next = pl.anc[cur ^ 1];
        m.enc_lens = enc_lens_dev; m.done = pl.done; m.active = pl.active;
        m.N = pl.N; m.Lcap = Lcap; m.Tp = Tp; m.V = V; m.p = p; m.max_len = max_len; m.max_pos = e->cfg.max_pos;
        launch_step_merge(m, B, st);
        cur ^= 1;
        steps = p + 1;
        if (poll > 0 && steps % poll == 0 && steps < pl.Lrun) {
            int active = 1;
            HIPCHK(hipMemcpyAsync(&active, pl.active, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (active <= 0) break;
        }
    }
    launch_step_result(pl.tok[cur], pl.score[cur], enc_lens_dev, tokens_dev, lens_dev, scores_dev, pl.S, pl.N, Lcap, Tp, V, steps,
                       max_len, e->cfg.max_pos, st);
    LAUNCHCHK();
    if (steps_host_or_null) *steps_host_or_null = steps;
    return 0;
}

int masr_op_decoder_step(masr_engine* e, const float* enc_dev, const int32_t* enc_lens_host, int32_t B, int32_t Tp,
                         const int32_t* prefix_host, const int32_t* prefix_lens_host, int32_t N, int32_t L, int32_t top_n,
                         int32_t* top_ids_host, float* top_logp_host, float* logp_host_or_null, void* stream) {
    if (!enc_dev || !enc_lens_host || !prefix_host || !prefix_lens_host || !top_ids_host || !top_logp_host)
        return fail("masr_op_decoder_step: null argument");
    CHK(step_shape_check(e, "masr_op_decoder_step", B, Tp, N, L));
    const int V = e->cfg.vocab_size, S = B * N;
    if (top_n < 1 || top_n > 64 || top_n > V)
        return fail("masr_op_decoder_step: top_n = " + std::to_string(top_n) + " is outside 1 .. min(64, vocabulary)");
    if (L + 1 > e->cfg.max_pos - 1)
        return fail("masr_op_decoder_step: prefixes of L = " + std::to_string(L) + " tokens behind sos exceed max_pos - 1 = " +
                    std::to_string(e->cfg.max_pos - 1) + " positions");
    for (int b = 0; b < B; ++b)
        if (enc_lens_host[b] < 1 || enc_lens_host[b] > Tp)
            return fail("masr_op_decoder_step: utterance " + std::to_string(b) + " has " + std::to_string(enc_lens_host[b]) +
                        " encoder frames, outside 1 .. Tp");
    int maxlen = 0;
    for (int s = 0; s < S; ++s) {
        if (prefix_lens_host[s] < 0 || prefix_lens_host[s] > L)
            return fail("masr_op_decoder_step: prefix " + std::to_string(s) + " has length " + std::to_string(prefix_lens_host[s]) +
                        ", outside 0 .. L");
        maxlen = std::max(maxlen, prefix_lens_host[s]);
        for (int i = 0; i < prefix_lens_host[s]; ++i) {
            const int t = prefix_host[(size_t)s * L + i];
            if (t < 0 || t >= V)
                return fail("masr_op_decoder_step: token id " + std::to_string(t) + " of prefix " + std::to_string(s) +
                            " is outside the vocabulary");
        }
    }
    ENTER(e);
    hipStream_t st = (hipStream_t)stream;
    CallGuard call_guard(e, st);
    StepPlan pl{};
    pl.B = B; pl.N = N; pl.S = S; pl.Tp = Tp; pl.Lcap = L; pl.max_len = 0;
    pl.Lrun = maxlen + 1;                      // positions 0 .. maxlen: [sos, tokens...]
    CHK(step_workspaces(e, pl, top_n));
    if (logp_host_or_null) CHK(e->st_full.ensure((size_t)S * V * sizeof(float)));
    // every row is its own ancestor at every position; it writes its outputs at its last position, p = its length
    std::vector<int> anc((size_t)S * L), pos(S), tok((size_t)S * L, 0);
    for (int s = 0; s < S; ++s) {
        pos[s] = prefix_lens_host[s];
        for (int j = 0; j < L; ++j) anc[(size_t)s * L + j] = s % N;
        for (int j = 0; j < prefix_lens_host[s]; ++j) tok[(size_t)s * L + j] = prefix_host[(size_t)s * L + j];
    }
    struct Table {
        int* p = nullptr;
        ~Table() { if (p) (void)hipFree(p); }
    } tab;
    HIPCHK(hipMalloc((void**)&tab.p, (size_t)(S + B) * sizeof(int)));
    int *pos_d = tab.p, *enc_d = pos_d + S;
    HIPCHK(hipMemcpyAsync(pl.tok[0], tok.data(), tok.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pl.anc[0], anc.data(), anc.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pos_d, pos.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(enc_d, enc_lens_host, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
    step_source_kv(e, st, enc_dev, pl);
    float* full = logp_host_or_null ? e->st_full.as<float>() : nullptr;
    for (int p = 0; p < pl.Lrun; ++p) CHK(step_forward(e, st, pl, p, pl.tok[0], pl.anc[0], enc_d, top_n, full, pos_d));
    LAUNCHCHK();
    float* top_v = e->st_top.as<float>();
    HIPCHK(hipMemcpyAsync(top_logp_host, top_v, (size_t)S * top_n * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(top_ids_host, top_v + (size_t)S * top_n, (size_t)S * top_n * sizeof(int), hipMemcpyDeviceToHost, st));
    if (full) HIPCHK(hipMemcpyAsync(logp_host_or_null, full, (size_t)S * V * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// decoder: joint -- the search above ranked by the joint key: the step launches with the top M of every row, the CTC prefix
// scorer over the M candidates, the joint merge, the prefix states of the N winners (kernels: decoder_joint.hip); with a language
// model (masr_joint_decode_lm) the n-gram score of the same M candidates between the step and the merge
// ------------------------------------------------------------------------------------------------
// (lm_weight 0: no model is looked at and nothing of the LM is launched -- masr_joint_decode's launches and bits)
static int joint_decode_impl(const char* who, masr_engine* e, const float* enc_dev, const int32_t* enc_lens_dev, int32_t B, int32_t Tp,
                             const float* post_dev, int32_t input_is_log, int32_t beam_size, int32_t ctc_candidates, float ctc_weight,
                             float length_bonus, masr_lm* lm_model, float lm_weight, int32_t max_len, int32_t* tokens_dev, int32_t Lcap,
                             int32_t* lens_dev, float* scores_dev, float* att_or_null, float* ctc_or_null, float* lm_or_null,
                             int32_t* steps_host_or_null, void* stream) {
    const std::string w(who);
    if (!enc_dev || !enc_lens_dev || !tokens_dev || !lens_dev || !scores_dev) return fail(w + ": null argument");
    if (max_len < 0) return fail(w + ": max_len must be 0 (no limit of its own) or positive");
    if (!(ctc_weight >= 0.f && ctc_weight < 1.f)) return fail(w + ": ctc_weight = " + std::to_string(ctc_weight) + " is outside [0, 1)");
    if (!std::isfinite(length_bonus)) return fail(w + ": length_bonus must be finite");
    if (!(std::isfinite(lm_weight) && lm_weight >= 0.f))
        return fail(w + ": lm_weight = " + std::to_string(lm_weight) + " is not a finite number >= 0");
    if (lm_weight > 0.f && !lm_model) return fail(w + ": lm_weight > 0 needs a language model (lm_or_null is null)");
    if (lm_model && lm_word_based(lm_model))
        return fail(w + ": word-based language models are searched on host threads (masr_beam_search_batch_lm): the joint search "
                    "scores vocabulary tokens");
    if (ctc_weight > 0.f && !post_dev) return fail(w + ": ctc_weight > 0 needs the CTC posteriors (post_dev is null)");
    if (beam_size >= 1 && beam_size <= 64 && (ctc_candidates < beam_size || ctc_candidates > 64))
        return fail(w + ": ctc_candidates = " + std::to_string(ctc_candidates) + " is outside beam_size .. 64");
    CHK(step_shape_check(e, who, B, Tp, beam_size, Lcap));
    const int V = e->cfg.vocab_size, M = ctc_candidates;
    if (M > V) return fail(w + ": ctc_candidates = " + std::to_string(M) + " exceeds the vocabulary of " + std::to_string(V));
    if (lm_model && lm_vocab_size(lm_model) != V)
        return fail(w + ": the language model was loaded for a vocabulary of " + std::to_string(lm_vocab_size(lm_model)) +
                    " tokens, the engine has " + std::to_string(V));
    ENTER(e);
    hipStream_t st = (hipStream_t)stream;
    CallGuard call_guard(e, st);
    // the table of the model on this device, before the first launch of the call (a first use uploads it and waits for that)
    const bool fuse = lm_weight > 0.f;
    LmView lmv{};
    if (fuse && lm_device_view(lm_model, &lmv)) return fail(w + ": " + masr_lm_last_error());
    StepPlan pl{};
    pl.B = B; pl.N = beam_size; pl.S = B * beam_size; pl.Tp = Tp; pl.Lcap = Lcap; pl.max_len = max_len;
    pl.Lrun = step_run_bound(e, Tp, Lcap, max_len);
    CHK(step_workspaces(e, pl, M));
    const bool ctc = ctc_weight > 0.f;
    const size_t S = (size_t)pl.S, rows = S * 2 * Tp;
    // att[2] | psi[2] [S], n[2] [S], Lm[2] [S], the candidates' psi [S, M] and (with a model) their lm [S, M]
    CHK(e->jt_tab.ensure((8 * S + (fuse ? 2 : 1) * S * M) * sizeof(float)));
    float* jt = e->jt_tab.as<float>();
    float *att[2] = {jt, jt + S}, *psi[2] = {jt + 2 * S, jt + 3 * S}, *lms[2] = {jt + 6 * S, jt + 7 * S}, *psi_cand = jt + 8 * S,
          *lm_cand = psi_cand + S * M;
    int* cnt[2] = {reinterpret_cast<int*>(jt + 4 * S), reinterpret_cast<int*>(jt + 5 * S)};
    float* r[2] = {nullptr, nullptr};
    PrefixRows pr{};
    pr.post = post_dev; pr.enc_lens = enc_lens_dev; pr.row_utt = nullptr; pr.done = pl.done;
    pr.S = pl.S; pr.N = pl.N; pr.V = V; pr.Tp = Tp; pr.input_is_log = input_is_log ? 1 : 0;
    if (ctc) {
        CHK(e->jt_r.ensure(2 * rows * sizeof(float)));
        r[0] = e->jt_r.as<float>();
        r[1] = r[0] + rows;
    }
    const int poll = step_poll_every();
    launch_step_init(pl.score[0], pl.done, pl.active, enc_lens_dev, B, pl.N, Tp, Lcap, max_len, e->cfg.max_pos, st);
    launch_joint_init(att[0], psi[0], lms[0], cnt[0], pl.S, pl.N, st);
    if (ctc) launch_prefix_init(pr, r[0], st);
    step_source_kv(e, st, enc_dev, pl);
    float* top_v = e->st_top.as<float>();
    const int* top_i = reinterpret_cast<const int*>(top_v + S * M);
    int cur = 0, steps = 0;
    for (int p = 0; p < pl.Lrun; ++p) {
        CHK(step_forward(e, st, pl, p, pl.tok[cur], pl.anc[cur], enc_lens_dev, M, nullptr, nullptr));
        if (ctc) launch_prefix_score(pr, top_i, M, pl.tok[cur], Lcap, p, nullptr, r[cur], psi_cand, st);
        if (fuse && launch_joint_lm_score(lmv, top_i, M, pl.tok[cur], Lcap, p, nullptr, pl.done, pl.S, pl.N, V, lm_cand, st))
            return fail(w + ": language model order " + std::to_string(lmv.max_order) + " is outside 1 .. 5");
        JointMerge m{};
        m.top_v = top_v; m.top_i = top_i; m.psi_cand = ctc ? psi_cand : nullptr; m.lm_cand = fuse ? lm_cand : nullptr;
        m.lm_cur = lms[cur]; m.lm_next = lms[cur ^ 1]; m.lm_weight = lm_weight;
        m.key_cur = pl.score[cur]; m.key_next = pl.score[cur ^ 1];
        m.att_cur = att[cur]; m.att_next = att[cur ^ 1]; m.psi_cur = psi[cur]; m.psi_next = psi[cur ^ 1];
        m.n_cur = cnt[cur]; m.n_next = cnt[cur ^ 1];
        m.tok_cur = pl.tok[cur]; m.tok_next = pl.tok[cur ^ 1]; m.anc_cur = pl.anc[cur]; m.anc_next = pl.anc[cur ^ 1];
        m.enc_lens = enc_lens_dev; m.done = pl.done; m.active = pl.active;
        m.N = pl.N; m.M = M; m.Lcap = Lcap; m.Tp = Tp; m.V = V; m.p = p; m.max_len = max_len; m.max_pos = e->cfg.max_pos;
        m.ctc_weight = ctc_weight; m.length_bonus = length_bonus;
        launch_joint_merge(m, B, st);
        if (ctc) launch_prefix_advance(pr, pl.tok[cur ^ 1], pl.anc[cur ^ 1], Lcap, p, nullptr, r[cur], r[cur ^ 1], st);
        cur ^= 1;
        steps = p + 1;
        if (poll > 0 && steps % poll == 0 && steps < pl.Lrun) {
            int active = 1;
            HIPCHK(hipMemcpyAsync(&active, pl.active, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (active <= 0) break;
        }
    }
    launch_step_result(pl.tok[cur], pl.score[cur], enc_lens_dev, tokens_dev, lens_dev, scores_dev, pl.S, pl.N, Lcap, Tp, V, steps,
                       max_len, e->cfg.max_pos, st);
    if (att_or_null) HIPCHK(hipMemcpyAsync(att_or_null, att[cur], S * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (ctc_or_null) HIPCHK(hipMemcpyAsync(ctc_or_null, psi[cur], S * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (lm_or_null) HIPCHK(hipMemcpyAsync(lm_or_null, lms[cur], S * sizeof(float), hipMemcpyDeviceToDevice, st));
    LAUNCHCHK();
    if (steps_host_or_null) *steps_host_or_null = steps;
    return 0;
}

int masr_joint_decode(masr_engine* e, const float* enc_dev, const int32_t* enc_lens_dev, int32_t B, int32_t Tp, const float* post_dev,
                      int32_t input_is_log, int32_t beam_size, int32_t ctc_candidates, float ctc_weight, float length_bonus,
                      int32_t max_len, int32_t* tokens_dev, int32_t Lcap, int32_t* lens_dev, float* scores_dev, float* att_or_null,
                      float* ctc_or_null, int32_t* steps_host_or_null, void* stream) {
    return joint_decode_impl("masr_joint_decode", e, enc_dev, enc_lens_dev, B, Tp, post_dev, input_is_log, beam_size, ctc_candidates,
                             ctc_weight, length_bonus, nullptr, 0.f, max_len, tokens_dev, Lcap, lens_dev, scores_dev, att_or_null,
                             ctc_or_null, nullptr, steps_host_or_null, stream);
}

int masr_joint_decode_lm(masr_engine* e, const float* enc_dev, const int32_t* enc_lens_dev, int32_t B, int32_t Tp, const float* post_dev,
                         int32_t input_is_log, int32_t beam_size, int32_t ctc_candidates, float ctc_weight, float length_bonus,
                         masr_lm* lm_or_null, float lm_weight, int32_t max_len, int32_t* tokens_dev, int32_t Lcap, int32_t* lens_dev,
                         float* scores_dev, float* att_or_null, float* ctc_or_null, float* lm_or_null_out, int32_t* steps_host_or_null,
                         void* stream) {
    return joint_decode_impl("masr_joint_decode_lm", e, enc_dev, enc_lens_dev, B, Tp, post_dev, input_is_log, beam_size,
                             ctc_candidates, ctc_weight, length_bonus, lm_or_null, lm_weight, max_len, tokens_dev, Lcap, lens_dev,
                             scores_dev, att_or_null, ctc_or_null, lm_or_null_out, steps_host_or_null, stream);
}

int masr_op_lm_scores(masr_engine* e, masr_lm* lm, const int32_t* prefix_host, const int32_t* prefix_lens_host, const int32_t* cand_host,
                      int32_t R, int32_t L, int32_t M, float* out_host, void* stream) {
    const std::string w("masr_op_lm_scores");
    if (!lm || !prefix_host || !prefix_lens_host || !cand_host || !out_host) return fail(w + ": null argument");
    if (R < 1 || R > 65535) return fail(w + ": R = " + std::to_string(R) + " rows is outside 1 .. 65535");
    if (L < 1) return fail(w + ": L must be at least 1");
    if (M < 1 || M > 64) return fail(w + ": M = " + std::to_string(M) + " candidates per row is outside 1 .. 64");
    if (lm_word_based(lm))
        return fail(w + ": word-based language models are searched on host threads (masr_beam_search_batch_lm): the joint search "
                    "scores vocabulary tokens");
    if (!e || !e->finalized) return fail("engine not finalized");
    const int V = e->cfg.vocab_size;
    if (lm_vocab_size(lm) != V)
        return fail(w + ": the language model was loaded for a vocabulary of " + std::to_string(lm_vocab_size(lm)) +
                    " tokens, the engine has " + std::to_string(V));
    for (int s = 0; s < R; ++s) {
        if (prefix_lens_host[s] < 0 || prefix_lens_host[s] > L)
            return fail(w + ": prefix " + std::to_string(s) + " has length " + std::to_string(prefix_lens_host[s]) + ", outside 0 .. L");
        for (int i = 0; i < prefix_lens_host[s]; ++i) {
            const int t = prefix_host[(size_t)s * L + i];
            if (t < 0 || t >= V)
                return fail(w + ": token id " + std::to_string(t) + " of prefix " + std::to_string(s) + " is outside the vocabulary");
        }
        for (int m = 0; m < M; ++m) {
            const int t = cand_host[(size_t)s * M + m];
            if (t < 0 || t >= V)
                return fail(w + ": candidate id " + std::to_string(t) + " of row " + std::to_string(s) + " is outside the vocabulary");
        }
    }
    ENTER(e);
    hipStream_t st = (hipStream_t)stream;
    CallGuard call_guard(e, st);
    LmView lmv{};
    if (lm_device_view(lm, &lmv)) return fail(w + ": " + masr_lm_last_error());
    if (lmv.max_order < 1 || lmv.max_order > 5)          // (before anything is queued: the launcher refuses the same)
        return fail(w + ": language model order " + std::to_string(lmv.max_order) + " is outside 1 .. 5");
    // host table: tok [R, L] (zeros behind a prefix' length) | lens [R] | cand [R, M]; behind it on the device the scores [R, M]
    const size_t nR = (size_t)R;
    std::vector<int> tab(nR * L + nR + nR * M, 0);
    int *h_tok = tab.data(), *h_len = h_tok + nR * L, *h_cand = h_len + nR;
    for (int s = 0; s < R; ++s) {
        h_len[s] = prefix_lens_host[s];
        for (int i = 0; i < prefix_lens_host[s]; ++i) h_tok[(size_t)s * L + i] = prefix_host[(size_t)s * L + i];
    }
    memcpy(h_cand, cand_host, nR * M * sizeof(int));
    CHK(e->jt_tab.ensure((tab.size() + nR * M) * sizeof(int)));
    int* d = e->jt_tab.as<int>();
    float* d_out = reinterpret_cast<float*>(d + tab.size());
    // (the call waits for the stream before `tab` goes)
    HIPCHK(hipMemcpyAsync(d, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, st));
    (void)launch_joint_lm_score(lmv, d + nR * L + nR, M, d, L, 0, d + nR * L, nullptr, R, 1, V, d_out, st);
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(out_host, d_out, nR * M * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int masr_op_ctc_prefix_scores(masr_engine* e, const float* post_dev, int32_t input_is_log, const int32_t* frames_host, int32_t B,
                              int32_t Tp, const int32_t* row_utt_host, const int32_t* prefix_host, const int32_t* prefix_lens_host,
                              int32_t R, int32_t L, const int32_t* cand_host, int32_t M, float* psi_prefix_host, float* psi_cand_host,
                              void* stream) {
    const std::string w("masr_op_ctc_prefix_scores");
    if (!post_dev || !frames_host || !row_utt_host || !prefix_host || !prefix_lens_host || !cand_host || !psi_prefix_host ||
        !psi_cand_host)
        return fail(w + ": null argument");
    if (B <= 0 || Tp <= 0) return fail(w + ": B and Tp must be positive");
    if (R < 1 || R > 65535) return fail(w + ": R = " + std::to_string(R) + " rows is outside 1 .. 65535");
    if (L < 1) return fail(w + ": L must be at least 1");
    if (M < 1 || M > 64) return fail(w + ": M = " + std::to_string(M) + " candidates per row is outside 1 .. 64");
    if (!e || !e->finalized) return fail("engine not finalized");
    const int V = e->cfg.vocab_size;
    for (int b = 0; b < B; ++b)
        if (frames_host[b] < 1 || frames_host[b] > Tp)
            return fail(w + ": utterance " + std::to_string(b) + " has " + std::to_string(frames_host[b]) + " frames, outside 1 .. Tp");
    int maxlen = 0;
    for (int s = 0; s < R; ++s) {
        if (row_utt_host[s] < 0 || row_utt_host[s] >= B)
            return fail(w + ": row " + std::to_string(s) + " names utterance " + std::to_string(row_utt_host[s]) + ", outside 0 .. B - 1");
        if (prefix_lens_host[s] < 0 || prefix_lens_host[s] > L)
            return fail(w + ": prefix " + std::to_string(s) + " has length " + std::to_string(prefix_lens_host[s]) + ", outside 0 .. L");
        maxlen = std::max(maxlen, prefix_lens_host[s]);
        for (int i = 0; i < prefix_lens_host[s]; ++i) {
            const int t = prefix_host[(size_t)s * L + i];
            if (t < 1 || t >= V - 1)
                return fail(w + ": token id " + std::to_string(t) + " of prefix " + std::to_string(s) +
                            " is outside 1 .. vocabulary - 2 (a prefix holds neither blank nor eos)");
        }
        for (int m = 0; m < M; ++m) {
            const int t = cand_host[(size_t)s * M + m];
            if (t < 0 || t >= V)
                return fail(w + ": candidate id " + std::to_string(t) + " of row " + std::to_string(s) + " is outside the vocabulary");
        }
    }
    ENTER(e);
    hipStream_t st = (hipStream_t)stream;
    CallGuard call_guard(e, st);
    // host tables: tok [R, L] | lens [R] | lens - 1 [R] | utt [R] | frames [B] | cand [R, M] | the token of every row at every
    // position [maxlen, R]; behind them psi of the prefixes [R] and of the candidates [R, M]
    const size_t nR = (size_t)R;
    std::vector<int> tab(nR * L + 3 * nR + B + nR * M + (size_t)maxlen * nR, 0);
    int *h_tok = tab.data(), *h_len = h_tok + nR * L, *h_lm1 = h_len + nR, *h_utt = h_lm1 + nR, *h_fr = h_utt + nR, *h_cand = h_fr + B,
        *h_at = h_cand + nR * M;
    for (int s = 0; s < R; ++s) {
        h_len[s] = prefix_lens_host[s];
        h_lm1[s] = prefix_lens_host[s] - 1;
        h_utt[s] = row_utt_host[s];
        for (int i = 0; i < prefix_lens_host[s]; ++i) {
            h_tok[(size_t)s * L + i] = prefix_host[(size_t)s * L + i];
            h_at[(size_t)i * nR + s] = prefix_host[(size_t)s * L + i];
        }
    }
    memcpy(h_fr, frames_host, (size_t)B * sizeof(int));
    memcpy(h_cand, cand_host, nR * M * sizeof(int));
    const size_t rows = nR * 2 * Tp;
    CHK(e->jt_r.ensure(2 * rows * sizeof(float)));
    CHK(e->jt_tab.ensure((tab.size() + nR + nR * M) * sizeof(int)));
    int* d = e->jt_tab.as<int>();
    int *d_tok = d, *d_len = d_tok + nR * L, *d_lm1 = d_len + nR, *d_utt = d_lm1 + nR, *d_fr = d_utt + nR, *d_cand = d_fr + B,
        *d_at = d_cand + nR * M;
    float *d_psi = reinterpret_cast<float*>(d + tab.size()), *d_psic = d_psi + nR;
    // (the call waits for the stream before `tab` goes)
    HIPCHK(hipMemcpyAsync(d, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_psi, 0, nR * sizeof(float), st));            // psi of the empty prefix
    float* r[2] = {e->jt_r.as<float>(), e->jt_r.as<float>() + rows};
    PrefixRows pr{};
    pr.post = post_dev; pr.enc_lens = d_fr; pr.row_utt = d_utt; pr.done = nullptr;
    pr.S = R; pr.N = 1; pr.V = V; pr.Tp = Tp; pr.input_is_log = input_is_log ? 1 : 0;
    launch_prefix_init(pr, r[0], st);
    int cur = 0;
    for (int p = 0; p <= maxlen; ++p) {
        // a row reports the candidates' psi behind its last token, and its own psi as the extension that made it
        launch_prefix_score(pr, d_cand, M, d_tok, L, p, d_len, r[cur], d_psic, st);
        if (p == maxlen) break;
        launch_prefix_score(pr, d_at + (size_t)p * nR, 1, d_tok, L, p, d_lm1, r[cur], d_psi, st);
        launch_prefix_advance(pr, d_tok, d_tok, L, p, d_len, r[cur], r[cur ^ 1], st);     // (N = 1: every row is its own parent)
        cur ^= 1;
    }
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(psi_prefix_host, d_psi, nR * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(psi_cand_host, d_psic, nR * M * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int masr_decoder_info(masr_engine* e, int32_t* enabled, int32_t* num_blocks, int32_t* r_num_blocks, int64_t* weight_bytes,
                      int64_t* workspace_bytes) {
    if (!e) return fail("null engine");
    if (enabled) *enabled = e->dec.enabled ? 1 : 0;
    if (num_blocks) *num_blocks = e->dec.nl;
    if (r_num_blocks) *r_num_blocks = e->dec.nr;
    if (weight_bytes) *weight_bytes = (int64_t)e->dec.weight_bytes;
    if (workspace_bytes) *workspace_bytes = (int64_t)e->decoder_bytes();
    return 0;
}

}  // extern "C"
