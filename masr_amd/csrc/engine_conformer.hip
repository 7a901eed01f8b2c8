// libmasr_hip.so -- engine, Conformer (model_kind 0; finalize also for the Efficient Conformer, which shares the key names): weights, the fused
// full-context forward, the width-generic layer and the chunk step.  Host code only (file map: engine_state.h).
#include "engine_encoder.h"

namespace masr {

int finalize_conformer(masr_engine* e, hipStream_t s) {
    const int d = e->cfg.d_model, dff = e->cfg.d_ff, L = e->cfg.num_blocks, V = e->cfg.vocab_size, F = e->cfg.n_mels;
    const int il = e->input_layer, H = e->cfg.heads, dk = d / H;
    CHK(upload_conv_frontend(e, "encoder.embed.conv.0", "encoder.embed.conv.2", il == IL_CONV2D6 ? 5 : 3,
                             il == IL_CONV2D8 ? "encoder.embed.conv.4" : nullptr));
    // embed.out.0 (conv2d) / embed.linear (conv2d6, conv2d8)
    if (il != IL_CONV2D && e->host.count("encoder.embed.out.0.weight"))
        return fail("input_layer conv2d6 / conv2d8 but the checkpoint holds encoder.embed.out.0 (a conv2d front-end)");
    if (il == IL_CONV2D && e->host.count("encoder.embed.linear.weight"))
        return fail("input_layer conv2d but the checkpoint holds encoder.embed.linear (a conv2d6 / conv2d8 front-end)");
    if (il != IL_CONV2D8 && e->host.count("encoder.embed.conv.4.weight"))
        return fail("the checkpoint holds a third subsampling conv (encoder.embed.conv.4, conv2d8) but input_layer is not conv2d8");
    CHK(upload_embed_proj(e, il == IL_CONV2D ? "encoder.embed.out.0" : "encoder.embed.linear", sub_bins(il, F)));
    CHK(upload_pos_table(e));
    e->layers.assign(L, LayerW{});
    for (int i = 0; i < L; ++i) {
        LayerW& w = e->layers[i];
        const std::string p = "encoder.encoders." + std::to_string(i) + ".";
        CHK(up_wb(e, p + "norm_ff_macaron", {d}, &w.ln_ffm_w, &w.ln_ffm_b));
        CHK(up_wb(e, p + "norm_mha", {d}, &w.ln_mha_w, &w.ln_mha_b));
        CHK(up_wb(e, p + "norm_conv", {d}, &w.ln_conv_w, &w.ln_conv_b));
        CHK(up_wb(e, p + "norm_ff", {d}, &w.ln_ff_w, &w.ln_ff_b));
        CHK(up_wb(e, p + "norm_final", {d}, &w.ln_fin_w, &w.ln_fin_b));
        if (e->conv_bn) {
            // cnn_module_norm: batch_norm (conformer/convolution.py:60-67): eval-mode BatchNorm1d folded into y = x * scale + shift
            const HostTensor* bn[4];
            CHK(get_conv_bn(e, p, bn));
            // (the reference's own float32 steps, so that y = fma(x, scale, shift) is its eval-mode batch_norm bit for bit:
            //  invstd = 1 / sqrt(var + eps), scale = weight * invstd, shift = fma(-mean, scale, bias).  The Squeezeformer's fold
            //  (engine_squeezeformer.hip) divides and subtracts instead -- other float32 roundings: the two are not to be merged)
            std::vector<float> sc(d), sh(d);
            for (int c = 0; c < d; ++c) {
                const float invstd = 1.0f / sqrtf(bn[3]->v[c] + 1e-5f);
                sc[c] = bn[0]->v[c] * invstd;
                sh[c] = fmaf(-bn[2]->v[c], sc[c], bn[1]->v[c]);
            }
            CHK(upload(e, sc, &w.cln_w));
            CHK(upload(e, sh, &w.cln_b));
        } else {
            CHK(up_wb(e, p + "conv_module.norm", {d}, &w.cln_w, &w.cln_b));
        }
        CHK(up_wb(e, p + "feed_forward_macaron.w_1", {dff, d}, &w.ffm_w1, &w.ffm_b1));
        CHK(up_wb(e, p + "feed_forward_macaron.w_2", {d, dff}, &w.ffm_w2, &w.ffm_b2));
        CHK(up_wb(e, p + "feed_forward.w_1", {dff, d}, &w.ff_w1, &w.ff_b1));
        CHK(up_wb(e, p + "feed_forward.w_2", {d, dff}, &w.ff_w2, &w.ff_b2));
        CHK(upload_qkv(e, p, &w.wqkv, &w.bqkv));
        CHK(up_wb(e, p + "self_attn.linear_out", {d, d}, &w.wo, &w.bo));
        const int gk = layer_grouped(e, i) ? dk * e->group_size : dk;
        if (e->pos_enc == POS_ENC_REL) {
            for (const char* key : {"self_attn.linear_pos.weight", "self_attn.pos_bias_u", "self_attn.pos_bias_v"})
                if (!e->host.count(p + key))
                    return fail("pos_enc_layer_type rel_pos but the checkpoint has no " + p + key +
                                " (a checkpoint trained with abs_pos / no_pos: plain MultiHeadedAttention)");
            CHK(up(e, p + "self_attn.linear_pos.weight", {d, d}, &w.wpos));
            CHK(up(e, p + "self_attn.pos_bias_u", {H, gk}, &w.pos_u));
            CHK(up(e, p + "self_attn.pos_bias_v", {H, gk}, &w.pos_v));
        } else {
            // plain MultiHeadedAttention (conformer/attention.py:10-167) has none of the three; a checkpoint that holds one was
            // trained with rel_pos
            for (const char* key : {"self_attn.linear_pos.weight", "self_attn.pos_bias_u", "self_attn.pos_bias_v"})
                if (e->host.count(p + key))
                    return fail(std::string("pos_enc_layer_type ") + (e->pos_enc == POS_ENC_ABS ? "abs_pos" : "no_pos") +
                                " but the checkpoint holds " + p + key + " (a checkpoint trained with rel_pos)");
        }
        CHK(up_wb(e, p + "conv_module.pointwise_conv1", {2 * d, d, 1}, &w.pw1_w, &w.pw1_b));   // rows: value c, gate d + c
        if (d == 256 && e->act == ENC_ACT_SWISH) {   // [Wo; W_pw1] and [bo; b_pw1]: one continuous weight stream for the fused kernel of the offline path
            const HostTensor *a, *b, *c2, *d2;
            CHK(get(e, p + "self_attn.linear_out.weight", {d, d}, &a));
            CHK(get(e, p + "self_attn.linear_out.bias", {d}, &b));
            CHK(get(e, p + "conv_module.pointwise_conv1.weight", {2 * d, d, 1}, &c2));
            CHK(get(e, p + "conv_module.pointwise_conv1.bias", {2 * d}, &d2));
            std::vector<float> cw(a->v), cb(b->v);
            cw.insert(cw.end(), c2->v.begin(), c2->v.end());
            cb.insert(cb.end(), d2->v.begin(), d2->v.end());
            CHK(upload(e, cw, &w.chain_w));
            CHK(upload(e, cb, &w.chain_b));
        }
        CHK(upload_gconst(e, s, w.pw1_b, d != 256, &w.gconst));
        CHK(upload_depthwise(e, p, layer_kernel(e, i), &w.dw_w, &w.dw_b));
        CHK(up_wb(e, p + "conv_module.pointwise_conv2", {d, d, 1}, &w.pw2_w, &w.pw2_b));
        if (e->pos_enc == POS_ENC_REL) CHK(build_ptab(e, s, w.wpos, &w.ptab));
    }
    CHK(up_wb(e, "encoder.after_norm", {d}, &e->after_w, &e->after_b));
    CHK(up_wb(e, "ctc.ctc_lo", {V, d}, &e->ctc_w, &e->ctc_b));
    return 0;
}

// abs_pos (PositionalEncoding.forward, embedding.py:39-56): x * sqrt(d) + pe[offset : offset + Tq] -- embed() has multiplied, this
// adds the sinusoid rows in a launch of its own (multiply, round, add, round: the reference's two operations).  offs: the device
// offsets of the sequences (chunk steps: each stream's own), nullptr = 0 for all (full context).  The callers have checked
// offset + Tq against max_pos.  rel_pos hands the same rows to the layers instead; no_pos adds nothing.
static void add_abs_pos(masr_engine* e, hipStream_t s, int nseq, int Tq, const int* offs) {
    if (e->pos_enc != POS_ENC_ABS) return;
    launch_add_pos_rows(e->x.as<float>(), e->pe, offs, nseq, Tq, e->cfg.d_model, e->cfg.max_pos, s);
}
// which attention instantiation a Conformer layer runs (common.h AttPos)
static int att_pos(const masr_engine* e) { return e->pos_enc == POS_ENC_REL ? ATT_REL_POS : ATT_NO_POS; }

// Width-generic Conformer path (masr_create admits it for model_kind 0 only): output_size 512 / attention_heads 8, and output_size
// 256 / 4 with an activation_type other than swish.  The layer of conformer/encoder.py:88-167 with every step as its own launch --
// the row kernels of wide.hip, the tiled GEMM of gemm_f32.hip for every product and the attention kernels with heads of 64.  No
// packed weight copies for the layers, none of the fused row-block kernels (they are built for K = 256 and for Swish), so none of
// their masr_debug_set switches applies here; the subsampling front end has no activation_type and runs as on the fused path.
// The activation (e->act) sits in two places: the epilogue of the first GEMM of wide_ffn and the tail of the depthwise kernel.
bool is_wide(const masr_engine* e) { return e->cfg.model_kind == 0 && (e->cfg.d_model != 256 || e->act != ENC_ACT_SWISH); }

static int ensure_wide_ws(masr_engine* e, int nseq, int Tq) {
    CHK(ensure_layer_ws(e, nseq, Tq));
    // hidden rows of an FFN [M, d_ff] or the value | gate rows of pointwise_conv1 over the padded layout [Mp, 2 d]
    const size_t Mp = (size_t)nseq * (Tq + e->cfg.cnn_kernel - 1);
    return e->hid.ensure(Mp * std::max(e->cfg.d_ff, 2 * e->cfg.d_model) * sizeof(float));
}

// x <- x + 0.5 * (W2 . act(W1 . LayerNorm(x) + b1) + b2), act = the engine's activation_type
static int wide_ffn(masr_engine* e, hipStream_t s, int M, const float* lnw, const float* lnb, const float* w1, const float* b1,
             const float* w2, const float* b2) {
    const int d = e->cfg.d_model, dff = e->cfg.d_ff;
    float *x = e->x.as<float>(), *ln = e->ln.as<float>(), *hid = e->hid.as<float>();
    WIDECHK(PROF_WIDE_LN, launch_layernorm_wide(x, lnw, lnb, ln, M, d, 1e-5f, 0, 0, nullptr, s));
    gemm(e, s, ln, d, w1, b1, hid, dff, M, dff, d, gemm_act_of(e->act), 1.f, nullptr, 0, PROF_FFN1);
    gemm(e, s, hid, dff, w2, b2, x, d, M, d, dff, ACT_NONE, 0.5f, x, d, PROF_FFN1);
    return 0;
}

// one layer on x [nseq * Tq, d] in place.  Offline (cache_rd == nullptr): seqs point into the qkv buffer, lens mask the padded
// frames, the conv module's history is the constant glu(bias) row (causal build) or zero padding on both sides.  Chunk step: the
// k | v columns are appended to the streams' caches, the conv module reads its history rows from cache_rd and writes cache_wr.
static int wide_layer(masr_engine* e, hipStream_t s, const LayerW& w, int nseq, int Tq, const int* lens, const AttSeq* seqs, int chunk,
               float* const* cache_rd, float* const* cache_wr) {
    const int d = e->cfg.d_model, H = e->cfg.heads, K = e->cfg.cnn_kernel, pad = K - 1, M = nseq * Tq;
    const bool stream = cache_rd != nullptr;
    float *x = e->x.as<float>(), *ln = e->ln.as<float>(), *hid = e->hid.as<float>(), *glu = e->glu.as<float>();
    CHK(wide_ffn(e, s, M, w.ln_ffm_w, w.ln_ffm_b, w.ffm_w1, w.ffm_b1, w.ffm_w2, w.ffm_b2));
    // self-attention: x <- x + Wo . att(LayerNorm(x))
    WIDECHK(PROF_WIDE_LN, launch_layernorm_wide(x, w.ln_mha_w, w.ln_mha_b, ln, M, d, 1e-5f, 0, 0, nullptr, s));
    gemm(e, s, ln, d, w.wqkv, w.bqkv, e->qkv.as<float>(), 3 * d, M, 3 * d, d, ACT_NONE, 1.f, nullptr, 0);
    if (stream) WIDECHK(PROF_WIDE_CACHE, launch_kv_append_wide(seqs, e->qkv.as<float>(), nseq, Tq, d, s));
    {
        ProfScope ps(e, s, PROF_ATT, 6.0 * d * (double)Tq * Tq * nseq);
        launch_attention(seqs, nseq, Tq, H, 3 * d, stream ? 2 * d : 3 * d, w.ptab, w.pos_u, w.pos_v, chunk, 1, s, d, att_pos(e));
    }
    gemm(e, s, e->att.as<float>(), d, w.wo, w.bo, x, d, M, d, d, ACT_NONE, 1.f, x, d);
    // conv module: x <- x + mask(pw2(act(LayerNorm(dwconv(GLU(pw1(mask(LayerNorm(x)))))))))
    const int in_pad = stream ? pad : 0, Mp = nseq * (Tq + in_pad);
    if (stream) {
        WIDECHK(PROF_WIDE_CACHE, launch_conv_hist_wide(x, w.ln_conv_w, w.ln_conv_b, cache_rd, cache_wr, e->lnpad.as<float>(), nseq, Tq, pad, d, 1e-5f, s));
    } else {
        WIDECHK(PROF_WIDE_LN, launch_layernorm_wide(x, w.ln_conv_w, w.ln_conv_b, ln, M, d, 1e-5f, Tq, 0, lens, s));
    }
    gemm(e, s, stream ? e->lnpad.as<float>() : ln, d, w.pw1_w, w.pw1_b, hid, 2 * d, Mp, 2 * d, d, ACT_NONE, 1.f, nullptr, 0);
    WIDECHK(PROF_WIDE_GLU, launch_glu_wide(hid, glu, Mp, d, s));
    WIDECHK(PROF_WIDE_DWCONV, launch_dwconv_ln_silu_wide(glu, w.dw_w, w.dw_b, w.cln_w, w.cln_b, e->dwo.as<float>(), nseq, Tq, d, K, in_pad,
                                       (stream || e->cfg.causal) ? pad : pad / 2, 1e-5f,
                                       (!stream && e->cfg.causal) ? w.gconst : nullptr, gemm_act_of(e->act), s));
    gemm(e, s, e->dwo.as<float>(), d, w.pw2_w, w.pw2_b, x, d, M, d, d, ACT_NONE, 1.f, x, d, PROF_GEMM, lens, lens ? Tq : 0);
    CHK(wide_ffn(e, s, M, w.ln_ff_w, w.ln_ff_b, w.ff_w1, w.ff_b1, w.ff_w2, w.ff_b2));
    WIDECHK(PROF_WIDE_LN, launch_layernorm_wide(x, w.ln_fin_w, w.ln_fin_b, x, M, d, 1e-5f, 0, 0, nullptr, s));
    return 0;
}

// ConformerEncoder.forward on the width-generic layer (masr_encode_full): feats [B, T, n_mels] -> enc_out [B * T', d]
int encode_full_wide(masr_engine* e, hipStream_t s, const float* feats, const int* lens, int B, int T, float* enc_out, int chunk) {
    const int d = e->cfg.d_model;
    if (!wide_supported(d)) return fail("no kernels for output_size " + std::to_string(d));
    int Tq = 0;
    CHK(embed(e, s, feats, B, T, &Tq));
    if (Tq >= e->cfg.max_pos) return fail("sequence longer than max_pos");   // embedding.py:48-50 assert
    add_abs_pos(e, s, B, Tq, nullptr);
    CHK(ensure_wide_ws(e, B, Tq));
    CHK(e->attseq.ensure(sizeof(AttSeq) * B));
    launch_attseq_full_wide(e->attseq.as<AttSeq>(), e->qkv.as<float>(), e->att.as<float>(), lens, B, Tq, d, s);
    for (const LayerW& w : e->layers) CHK(wide_layer(e, s, w, B, Tq, lens, e->attseq.as<AttSeq>(), chunk, nullptr, nullptr));
    WIDECHK(PROF_WIDE_LN, launch_layernorm_wide(e->x.as<float>(), e->after_w, e->after_b, enc_out, B * Tq, d, 1e-5f, 0, 0, nullptr, s));
    LAUNCHCHK();
    return 0;
}

// ConformerEncoder.forward on the fused kernels (masr_encode_full: output_size 256, swish).  chunk: decoding_chunk_size in the
// streaming-trained build, 0 otherwise
int encode_full_conformer(masr_engine* e, hipStream_t s, const float* feats_dev, const int* feat_lens_dev, int B, int T,
                                 float* enc_out_dev, int chunk) {
    const int d = e->cfg.d_model, H = e->cfg.heads, pad = e->cfg.cnn_kernel - 1;
    int Tq = 0;
    CHK(embed(e, s, feats_dev, B, T, &Tq));
    if (Tq >= e->cfg.max_pos) return fail("sequence longer than max_pos");   // embedding.py:48-50 assert
    add_abs_pos(e, s, B, Tq, nullptr);
    const int M = B * Tq;
    CHK(ensure_layer_ws(e, B, Tq));
    CHK(e->attseq.ensure(sizeof(AttSeq) * B));
    float* x = e->x.as<float>();
    EncodeCtx ctx{B, Tq, feat_lens_dev};
    launch_attseq_full(e->attseq.as<AttSeq>(), e->qkv.as<float>(), e->att.as<float>(), feat_lens_dev, B, Tq, 4, s);
    if (!e->cfg.causal)     // symmetric conv: the (K-1)/2 pad rows on both sides of every sequence stay zero for all layers
        HIPCHK(hipMemsetAsync(e->glu.p, 0, (size_t)B * (Tq + pad) * d * sizeof(float), s));
    const LayerW* prev = nullptr;                 // layer whose norm_final is still pending (it rides on the next FFN launch)
    const bool few_rows = few_row_blocks(knobs(), M);
    for (const LayerW& w : e->layers) {
        // first macaron FFN with the attention block's LayerNorm + fused QKV projection as its tail stage (full kernel only)
        FfnArgs f1 = ffn_macaron(w, M);
        f1.tail = qkv_tail(e, w, e->qkv.as<float>(), 3 * d);
        if (prev) { f1.tail.pre_lnw = prev->ln_fin_w; f1.tail.pre_lnb = prev->ln_fin_b; }
        const FfnDone r1 = ffn(e, s, f1);
        CHK(r1);
        if (!r1.tail_done) mhsa(e, s, w, M);
        // attention and the chain kernel behind it as ONE launch (32 queries x all four heads per workgroup; key 34 = 0: two launches)
        // (the experimental one-launch kernel carries the positional term only)
        const bool fuse_ac = knobs().attn_chain && !few_rows && !knobs().no_chain && H == 4 && d == 256 && knobs().rowgemm_packed &&
                             e->pos_enc == POS_ENC_REL;
        if (fuse_ac) {
            AttnChainArgs a{};
            a.seqs = e->attseq.as<AttSeq>(); a.nseq = B; a.q_stride = 3 * d; a.kv_stride = 3 * d;
            a.chunk_size = chunk; a.pos_stride = 1;
            a.ptab = w.ptab; a.bias_u = w.pos_u; a.bias_v = w.pos_v;
            a.Wp = packed_rows_of(e, w.chain_w, 3 * d, s); a.bias = w.chain_b; a.lnw = w.ln_conv_w; a.lnb = w.ln_conv_b;
            a.R = x; a.R2 = x; a.C = e->glu.as<float>(); a.lens = feat_lens_dev; a.seq_t = Tq; a.mstride = 4;
            a.out_pad_l = e->cfg.causal ? pad : pad / 2; a.out_pad_tot = pad; a.eps = 1e-5f;
            if (!a.Wp) return fail("packed chain weights: allocation failed");
            ProfScope ps(e, s, PROF_ATT, 6.0 * d * (double)Tq * Tq * B + 2.0 * M * (double)(3 * d) * d);
            launch_attn_chain(a, Tq, s);
        } else {
            ProfScope ps(e, s, PROF_ATT, 6.0 * d * (double)Tq * Tq * B);
            launch_attention(e->attseq.as<AttSeq>(), B, Tq, H, 3 * d, 3 * d, w.ptab, w.pos_u, w.pos_v, chunk, 1, s, 256, att_pos(e));   // use_dynamic_chunk only in the streaming build
        }
        if (few_rows) {
            // few row blocks (one utterance, a handful of short ones): latency-cut kernels of the chunk steps -- the row-block
            // chain kernel would put [out-proj -> LN -> pw1] of a row block on ONE workgroup (28.6 us at 7 row blocks against
            // 7.4 + 7.7 us for the two K-split launches whose columns spread over the chip); norm_final rides on the split
            // FFN's reduction
            mhsa_out(e, s, w, M);
            const bool fuse = knobs().split_head && e->cfg.cnn_kernel == 15 && knobs().ffn_packed >= 2 && !knobs().no_ffn_head;
            CHK(conv_module(e, s, w, ctx, false, 0, 4, false, fuse));
            FfnArgs f2 = ffn_final(w, M, x);
            if (fuse) f2.head = conv_head(e, w, feat_lens_dev, Tq, e->cfg.cnn_kernel, 4);
            CHK(ffn(e, s, f2));
            continue;                              // (prev stays null: nothing deferred)
        } else if (knobs().no_chain) {
            mhsa_out(e, s, w, M);
            CHK(conv_module(e, s, w, ctx, false));
            CHK(ffn(e, s, ffn_final(w, M)));
        } else {
            // out-projection + residual + LayerNorm + pointwise_conv1 + GLU in one kernel; the rest of the conv module
            // (depthwise conv, LayerNorm or folded BatchNorm, SiLU, pointwise_conv2, residual) is the head stage of the second FFN kernel
            if (!fuse_ac) mhsa_out_pw1(e, s, w, ctx);
            FfnArgs f2 = ffn_final(w, M);
            f2.head = conv_head(e, w, feat_lens_dev, Tq, e->cfg.cnn_kernel, 4);
            CHK(ffn(e, s, f2));
        }
        prev = &w;                                 // norm_final deferred to the next layer's first FFN launch
    }
    if (prev) launch_layernorm(x, prev->ln_fin_w, prev->ln_fin_b, x, M, 1e-5f, 0, 0, nullptr, s);
    launch_layernorm(x, e->after_w, e->after_b, enc_out_dev, M, 1e-5f, 0, 0, nullptr, s);
    LAUNCHCHK();
    return 0;
}

// Conformer chunk step, n streams in lock-step: ConformerEncoder.forward_chunk (conformer/encoder.py:355-420), on the fused
// kernels or (is_wide) on the width-generic layer.  Unlike the other families' steps this one has never refused a stream id given
// twice in one call (distinct_streams): whether it should is a behaviour decision of its own.
int encode_chunk_conformer(masr_engine* e, hipStream_t s, std::vector<Stream*>& st, const float* feats_dev, int Tc,
                                  float* probs_dev, int32_t* argmax_dev, float* maxprob_dev, float* enc_out_dev) {
    const int n = (int)st.size();
    const int d = e->cfg.d_model, H = e->cfg.heads, L = e->cfg.num_blocks, pad = e->cfg.cnn_kernel - 1;
    int Tq = 0;
    CHK(embed(e, s, feats_dev, n, Tc, &Tq));
    for (int i = 0; i < n; ++i)
        if (st[i]->offset + Tq > st[i]->cap) return fail("stream exceeds its max_frames_out / max_pos");
    const int M = n * Tq;
    const bool wide = is_wide(e);        // output_size 512 or a non-swish activation: the same descriptors and caches, every layer as separate launches
    if (wide && !wide_supported(d)) return fail("no kernels for output_size " + std::to_string(d));
    CHK(wide ? ensure_wide_ws(e, n, Tq) : ensure_layer_ws(e, n, Tq));
    CHK(e->attseq.ensure(sizeof(AttSeq) * (size_t)n * L));
    // descriptors for all layers in one H2D copy
    std::vector<AttSeq> hs((size_t)n * L);
    for (int l = 0; l < L; ++l)
        for (int i = 0; i < n; ++i) {
            float* cache = st[i]->att.as<float>() + (size_t)l * st[i]->cap * 2 * d;
            // keys the chunk attends over: the last cache_t1 cached rows + its own (encoder.py:390-395,397-410: the reference
            // trims its cache tensor to required_cache_size after every step; here the rows stay where they were appended and
            // the window moves).  The positional index of the first key is offset - cache_t1.
            const int cache_t1 = st[i]->cache_t1;
            const int first = st[i]->offset - cache_t1;
            hs[(size_t)l * n + i] = interleaved_seq(e->qkv.as<float>() + (size_t)i * Tq * 3 * d, cache, d, first, cache_t1, Tq,
                                                    e->att.as<float>() + (size_t)i * Tq * d, first, st[i]->offset);
        }
    const std::vector<float*> hp = cnn_cache_table(st, L, (size_t)pad * d);    // cnn cache base of (layer, stream): current (read) | next (written)
    CHK(e->cnnptrs.ensure(sizeof(float*) * hp.size()));
    std::vector<int> ho;                          // abs_pos: pe[offset : offset + Tq] of every stream (embedding.py:52-54)
    if (e->pos_enc == POS_ENC_ABS) {
        for (int i = 0; i < n; ++i) ho.push_back(st[i]->offset);
        CHK(e->posoff.ensure(sizeof(int) * ho.size()));
    }
    CHK(upload_chunk_tables(e, s, hs, hp, e->posoff.p, ho.data(), sizeof(int) * ho.size()));
    add_abs_pos(e, s, n, Tq, e->posoff.as<int>());
    float* x = e->x.as<float>();
    EncodeCtx ctx{n, Tq, nullptr};
    for (int l = 0; l < L; ++l) {
        if (wide) {
            float* const* cp = e->cnnptrs.as<float*>() + (size_t)l * n;
            CHK(wide_layer(e, s, e->layers[l], n, Tq, nullptr, e->attseq.as<AttSeq>() + (size_t)l * n, 0, cp, cp + (size_t)L * n));
            continue;
        }
        const LayerW& w = e->layers[knobs().hot_weights ? 0 : l];
        CHK(ffn(e, s, ffn_macaron(w, M)));
        mhsa(e, s, w, M, e->attseq.as<AttSeq>() + (size_t)l * n, Tq);     // q -> qkv buffer, k|v rows -> the streams' caches
        launch_attention(e->attseq.as<AttSeq>() + (size_t)l * n, n, Tq, H, 3 * d, 2 * d, w.ptab, w.pos_u, w.pos_v, 0, 1, s, 256, att_pos(e));
        mhsa_out(e, s, w, M);
        float* const* cptr = e->cnnptrs.as<float*>() + (size_t)l * n;
        // [depthwise conv -> LN -> SiLU -> pointwise_conv2 + residual] rides on the second FFN launch as its head stage (on the
        // d_ff-split launch of few streams every slice repeats it on the row block's rows; one launch less on the step's chain)
        const bool fuse = knobs().split_head && e->cfg.cnn_kernel == 15 && knobs().ffn_packed >= 2 && !knobs().no_ffn_head;
        CHK(conv_module_stream(e, s, w, n, Tq, cptr, cptr + (size_t)L * n, e->cfg.cnn_kernel, fuse));
        FfnArgs f2 = ffn_final(w, M, x);
        if (fuse) {
            f2.head = conv_head(e, w, nullptr, Tq, e->cfg.cnn_kernel, 4);
            f2.head.gconst = nullptr;      // the history rows are real here: the streams' cnn caches
        }
        CHK(ffn(e, s, f2));
    }
    CHK(e->enc.ensure((size_t)M * d * sizeof(float)));
    if (wide) WIDECHK(PROF_WIDE_LN, launch_layernorm_wide(x, e->after_w, e->after_b, e->enc.as<float>(), M, d, 1e-5f, 0, 0, nullptr, s));
    else launch_layernorm(x, e->after_w, e->after_b, e->enc.as<float>(), M, 1e-5f, 0, 0, nullptr, s);
    CHK(chunk_ctc(e, s, e->enc.as<float>(), M, probs_dev, argmax_dev, maxprob_dev, enc_out_dev));
    for (int i = 0; i < n; ++i) {
        st[i]->cache_t1 = chunk_window(*st[i], Tq).next_cache_t1;
        st[i]->offset += Tq;
        std::swap(st[i]->cnn, st[i]->cnn2);
    }
    return 0;
}

}  // namespace masr
