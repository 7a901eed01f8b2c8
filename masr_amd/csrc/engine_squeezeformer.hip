// libmasr_hip.so -- engine, Squeezeformer (model_kind 1): weights, full-context forward and chunk step.  Host code only (file map: engine_state.h).
#include "engine_encoder.h"

namespace masr {

// reference: masr/model_utils/squeezeformer/{encoder,attention,convolution,positionwise,subsampling,time_reduction}.py
// the fused Squeezeformer stages cover these sizes (launch_sqz_stage's own checks, sqz_layer.hip): anything else takes the separate launches
static bool sqz_stage_supported(const masr_engine* e) {
    const int K = e->cfg.cnn_kernel;
    return e->cfg.d_model == 256 && e->cfg.d_ff % 128 == 0 && e->cfg.d_ff >= 256 && (K == 31 || K == 15);
}

// Squeezeformer (post-LN): adaptive scale / bias in front of the block, the whole block added, `post` = the LayerNorm behind it
static FfnArgs ffn_sqz(int M, const float* s, const float* b, const float* w1, const float* b1, const float* w2, const float* b2,
                const float* post_w, const float* post_b, float* post_y) {
    FfnArgs a = ffn_of(M, s, b, w1, b1, w2, b2);
    a.scale = 1.0f; a.affine = 1; a.post = {post_w, post_b, post_y};
    return a;
}
static FfnArgs ffn_sqz1(const SqLayerW& w, int M, float* y) { return ffn_sqz(M, w.f1_s, w.f1_b, w.f1_w1, w.f1_b1, w.f1_w2, w.f1_b2, w.ln2_w, w.ln2_b, y); }
static FfnArgs ffn_sqz2(const SqLayerW& w, int M, float* y) { return ffn_sqz(M, w.f2_s, w.f2_b, w.f2_w1, w.f2_b1, w.f2_w2, w.f2_b2, w.ln4_w, w.ln4_b, y); }

int finalize_squeezeformer(masr_engine* e, hipStream_t s) {
    const int d = e->cfg.d_model, dff = e->cfg.d_ff, L = e->cfg.num_blocks, V = e->cfg.vocab_size, K = e->cfg.cnn_kernel,
              H = e->cfg.heads, dk = d / H;
    const HostTensor* t;
    CHK(upload_conv_frontend(e, "encoder.embed.pw_conv", "encoder.embed.dw_conv", 3, nullptr));
    CHK(upload_embed_proj(e, "encoder.embed.input_proj.0", sub_bins(IL_CONV2D, e->cfg.n_mels)));
    CHK(upload_pos_table(e));
    CHK(up_wb(e, "encoder.preln", {d}, &e->preln_w, &e->preln_b));
    e->sq_layers.assign(L, SqLayerW{});
    for (int i = 0; i < L; ++i) {
        SqLayerW& w = e->sq_layers[i];
        const std::string p = "encoder.encoders." + std::to_string(i) + ".";
        auto vec = [&](const std::string& n, float** out) -> int { return up(e, p + n, {d}, out); };
        CHK(vec("self_attn.ada_scale", &w.att_s));
        CHK(vec("self_attn.ada_bias", &w.att_b));
        CHK(upload_qkv(e, p, &w.wqkv, &w.bqkv));
        CHK(up_wb(e, p + "self_attn.linear_out", {d, d}, &w.wo, &w.bo));
        CHK(up(e, p + "self_attn.linear_pos.weight", {d, d}, &w.wpos));
        CHK(up(e, p + "self_attn.pos_bias_u", {H, dk}, &w.pos_u));
        CHK(up(e, p + "self_attn.pos_bias_v", {H, dk}, &w.pos_v));
        CHK(build_ptab(e, s, w.wpos, &w.ptab));
        CHK(vec("layer_norm1.weight", &w.ln1_w)); CHK(vec("layer_norm1.bias", &w.ln1_b));
        CHK(vec("layer_norm2.weight", &w.ln2_w)); CHK(vec("layer_norm2.bias", &w.ln2_b));
        CHK(vec("layer_norm3.weight", &w.ln3_w)); CHK(vec("layer_norm3.bias", &w.ln3_b));
        CHK(vec("layer_norm4.weight", &w.ln4_w)); CHK(vec("layer_norm4.bias", &w.ln4_b));
        CHK(vec("ffn1.ada_scale", &w.f1_s)); CHK(vec("ffn1.ada_bias", &w.f1_b));
        CHK(up_wb(e, p + "ffn1.w_1", {dff, d}, &w.f1_w1, &w.f1_b1));
        CHK(up_wb(e, p + "ffn1.w_2", {d, dff}, &w.f1_w2, &w.f1_b2));
        CHK(vec("ffn2.ada_scale", &w.f2_s)); CHK(vec("ffn2.ada_bias", &w.f2_b));
        CHK(up_wb(e, p + "ffn2.w_1", {dff, d}, &w.f2_w1, &w.f2_b1));
        CHK(up_wb(e, p + "ffn2.w_2", {d, dff}, &w.f2_w2, &w.f2_b2));
        CHK(vec("conv_module.ada_scale", &w.cv_s)); CHK(vec("conv_module.ada_bias", &w.cv_b));
        CHK(up_wb(e, p + "conv_module.pointwise_conv1", {2 * d, d, 1}, &w.pw1_w, &w.pw1_b));
        // streaming-trained build (causal conv): the K-1 zero frames padded in front of pointwise_conv1 become glu(bias)
        CHK(upload_gconst(e, s, w.pw1_b, false, &w.gconst));
        CHK(upload_depthwise(e, p, K, &w.dw_w, &w.dw_b));
        {   // eval-mode BatchNorm1d folded: y = x * scale + shift, scale = w / sqrt(var + eps), shift = b - mean * scale.  (The
            // Conformer's fold, engine_conformer.hip, multiplies by 1 / sqrt and takes one fma, to match its reference bit for bit:
            // other float32 roundings than these -- the two are not to be merged)
            const HostTensor* bn[4];
            CHK(get_conv_bn(e, p, bn));
            std::vector<float> sc(d), sh(d);
            for (int c = 0; c < d; ++c) {
                sc[c] = bn[0]->v[c] / sqrtf(bn[3]->v[c] + 1e-5f);
                sh[c] = bn[1]->v[c] - bn[2]->v[c] * sc[c];
            }
            CHK(upload(e, sc, &w.bn_scale));
            CHK(upload(e, sh, &w.bn_shift));
        }
        CHK(up_wb(e, p + "conv_module.pointwise_conv2", {d, d, 1}, &w.pw2_w, &w.pw2_b));
    }
    {
        // TimeReductionLayer1D: depthwise k = 5, stride 2, padding 3; TimeReductionLayerStream (streaming-trained build,
        // squeezeformer/model.py:37-41): k = 1, stride 2, no padding == the k = 5 kernel with only tap 3 (t = 2j) non-zero
        const int tk = e->cfg.causal ? 1 : 5;
        CHK(get(e, "encoder.time_reduction_layer.dw_conv.weight", {d, 1, tk}, &t));
        std::vector<float> wd((size_t)5 * d, 0.f);
        for (int c = 0; c < d; ++c)
            for (int j = 0; j < tk; ++j) wd[(size_t)(tk == 1 ? 3 : j) * d + c] = t->v[(size_t)c * tk + j];
        CHK(upload(e, wd, &e->tr_dw_w));
        CHK(up(e, "encoder.time_reduction_layer.dw_conv.bias", {d}, &e->tr_dw_b));
        CHK(up_wb(e, "encoder.time_reduction_layer.pw_conv", {d, d, 1}, &e->tr_pw_w, &e->tr_pw_b));
        CHK(up_wb(e, "encoder.time_recover_layer", {d, d}, &e->rec_w, &e->rec_b));
    }
    CHK(up_wb(e, "ctc.ctc_lo", {V, d}, &e->ctc_w, &e->ctc_b));
    if (sqz_stage_supported(e)) {
        // the fused stages' fragment-order weight copies are made HERE, once, behind this call's synchronisation: a forward pass on
        // any stream then only reads the caches (they used to be filled by whichever stream ran the first pass, with nothing
        // ordering a second stream's reads behind that pack kernel)
        for (int i = 0; i < L; ++i) {
            const SqLayerW& w = e->sq_layers[i];
            const float *p1, *p2;
            CHK(packed_ffn_of(e, w.f1_w1, w.f1_w2, s, &p1, &p2));
            CHK(packed_ffn_of(e, w.f2_w1, w.f2_w2, s, &p1, &p2));
            if (!packed_rows_of(e, w.wo, d, s) || !packed_rows_of(e, w.pw1_w, 2 * d, s) || !packed_rows_of(e, w.pw2_w, d, s) ||
                !packed_rows_of(e, w.wqkv, 3 * d, s))
                return fail("squeezeformer: packing the layer's weights failed");
        }
    }
    return 0;
}

// SqueezeformerEncoder.forward, streaming = False (squeezeformer/encoder.py:168-216)
int encode_full_squeezeformer(masr_engine* e, hipStream_t s, const float* feats, const int* lens, int B, int T,
                                     float* enc_out, int chunk) {
    const int d = e->cfg.d_model, H = e->cfg.heads, K = e->cfg.cnn_kernel, half = (K - 1) / 2, pad = K - 1;
    int T0 = 0;
    // Row blocks / tiles that hold padded frames only are not computed (the valid frames' results do not depend on them: pad masks,
    // klen; reference encoder.py:168-216 computes and masks them): conv2, the input projection, attention (queries and keys stop at the
    // valid length) and the fused stage kernels -- a length-sorted batch padded to its longest utterance costs its VALID frames, so
    // one pass can take utterances of any lengths.  Off (masr_debug_set key 38 = 0) when the caller decodes the padded frames too.
    const bool skip = e->skip_padding != 0 && lens != nullptr;
    const int skm = skip ? e->skip_padding : 0;        // (bits, for A/B: 1 stage kernels, 2 conv2 + input projection, 4 attention)
    CHK(embed(e, s, feats, B, T, &T0, (skm & 2) ? lens : nullptr));
    if (T0 >= e->cfg.max_pos) return fail("sequence longer than max_pos");
    CHK(ensure_layer_ws(e, B, T0));
    CHK(e->attseq.ensure(sizeof(AttSeq) * B));
    CHK(e->xsave.ensure((size_t)B * T0 * d * sizeof(float)));
    CHK(e->xred.ensure((size_t)B * ((T0 + 1) / 2) * d * sizeof(float)));
    float* x = e->x.as<float>();
    launch_layernorm(x, e->preln_w, e->preln_b, x, B * T0, 1e-5f, 0, 0, nullptr, s);
    int Tq = T0, mstride = 4, pstride = 1;
    const bool causal = e->cfg.causal != 0;   // streaming-trained build: K-1 history rows in front (constant glu(bias))
    const int pad_l = causal ? K - 1 : half;
    auto new_resolution = [&]() -> int {     // zero the symmetric pad rows of the GLU buffer, rebuild the descriptors
        if (!causal) HIPCHK(hipMemsetAsync(e->glu.p, 0, (size_t)B * (Tq + pad) * d * sizeof(float), s));
        launch_attseq_full(e->attseq.as<AttSeq>(), e->qkv.as<float>(), e->att.as<float>(), lens, B, Tq, mstride, s, (skm & 4) ? 1 : 0);
        return 0;
    };
    CHK(new_resolution());
    const int L = e->cfg.num_blocks;
    bool qkv_ready = false;       // the previous layer's fused end stage has already written this layer's q | k | v
    for (int i = 0; i < L; ++i) {
        const SqLayerW& w = e->sq_layers[i];
        if (i == e->reduce_idx) {
            // TimeReductionLayer1D (time_reduction.py:53-76): keep x for the recovery, halve the frame rate
            HIPCHK(hipMemcpyAsync(e->xsave.p, x, (size_t)B * Tq * d * sizeof(float), hipMemcpyDeviceToDevice, s));
            launch_time_reduce_dw(x, e->tr_dw_w, e->tr_dw_b, lens, e->xred.as<float>(), B, Tq, mstride, s);
            const int Lr = (Tq + 1) / 2;
            rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_STORE, rg_args(e->xred.as<float>(), d, e->tr_pw_w, e->tr_pw_b, x, d, B * Lr, d));
            Tq = Lr; mstride = 8; pstride = 2;
            CHK(new_resolution());
        }
        if (i == e->recover_idx && e->reduce_idx >= 0) {
            // x = saved + Linear(repeat_interleave(x, 2))[:, :T0]   (encoder.py:199-205)
            rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_STORE, rg_args(x, d, e->rec_w, e->rec_b, e->xred.as<float>(), d, B * Tq, d));
            launch_recover_add(e->xsave.as<float>(), e->xred.as<float>(), x, B, T0, Tq, s);
            Tq = T0; mstride = 4; pstride = 1;
            CHK(new_resolution());
        }
        const int M = B * Tq;
        // Fused layer (sqz_layer.hip): attention + two row-block kernels.  Taken when the row blocks fill the chip (below that the
        // d_ff-split FFN and the K-split projections of the unfused sequence are the faster launches); bit-identical either way.
        const bool fused = knobs().sqz_fused_blocks > 0 && (M + 31) / 32 >= knobs().sqz_fused_blocks && sqz_stage_supported(e);
        // x = LN1(x + MHSA(ada(x)))
        if (!qkv_ready) qkv_proj(e, s, RG_PRO_AFFINE, w.att_s, w.att_b, w.wqkv, w.bqkv, M);
        qkv_ready = false;
        {
            ProfScope ps(e, s, PROF_ATT, 6.0 * d * (double)Tq * Tq * B);
            // (chunk > 0: decoding_chunk_size of the streaming-trained build; the kernel thins the mask by the layer's rate)
            launch_attention(e->attseq.as<AttSeq>(), B, Tq, H, 3 * d, 3 * d, w.ptab, w.pos_u, w.pos_v, chunk, pstride, s, 256, ATT_REL_POS);
        }
        if (fused) {
            // the next layer's QKV projection rides on this layer's last launch unless the frame rate changes in between
            const bool next_same = i + 1 < L && i + 1 != e->reduce_idx && !(i + 1 == e->recover_idx && e->reduce_idx >= 0);
            SqzStageArgs a{};
            a.x = x; a.out = x; a.att = e->att.as<float>();
            a.head_w = packed_rows_of(e, w.wo, d, s); a.head_b = w.bo;
            a.ln_a_w = w.ln1_w; a.ln_a_b = w.ln1_b; a.ln_b_w = w.ln2_w; a.ln_b_b = w.ln2_b;
            a.ffn_s = w.f1_s; a.ffn_b = w.f1_b; a.b1 = w.f1_b1; a.b2 = w.f1_b2;
            CHK(packed_ffn_of(e, w.f1_w1, w.f1_w2, s, &a.w1, &a.w2));
            a.tail_w = packed_rows_of(e, w.pw1_w, 2 * d, s); a.tail_b = w.pw1_b; a.tail_s = w.cv_s; a.tail_sb = w.cv_b; a.tail_n = 2 * d;
            a.glu_out = e->glu.as<float>(); a.glu_pad_l = pad_l; a.glu_pad_tot = pad;
            a.lens = lens; a.M = M; a.dff = e->cfg.d_ff; a.seq_t = Tq; a.mstride = mstride; a.ktaps = K; a.eps = 1e-5f; a.skip_pad = skm & 1;
            if (!a.head_w || !a.tail_w) return fail("squeezeformer: packing the layer's weights failed");
            {
                ProfScope ps(e, s, PROF_FFN_TAIL, 4.0 * M * (double)e->cfg.d_ff * d + 2.0 * M * (double)(3 * d) * d);
                if (!launch_sqz_stage(a, 0, s)) return fail("squeezeformer: the fused mid stage rejected the sizes");
            }
            SqzStageArgs b{};
            b.x = x; b.out = i == L - 1 ? enc_out : x; b.glu = e->glu.as<float>();
            b.head_w = packed_rows_of(e, w.pw2_w, d, s); b.head_b = w.pw2_b;
            b.dw_w = w.dw_w; b.dw_b = w.dw_b; b.bn_scale = w.bn_scale; b.bn_shift = w.bn_shift; b.gconst = causal ? w.gconst : nullptr;
            b.gpad = causal ? nullptr : w.gconst; b.glu_pad_l = pad_l;
            b.ln_a_w = w.ln3_w; b.ln_a_b = w.ln3_b; b.ln_b_w = w.ln4_w; b.ln_b_b = w.ln4_b;
            b.ffn_s = w.f2_s; b.ffn_b = w.f2_b; b.b1 = w.f2_b1; b.b2 = w.f2_b2;
            CHK(packed_ffn_of(e, w.f2_w1, w.f2_w2, s, &b.w1, &b.w2));
            if (next_same) {
                const SqLayerW& nx = e->sq_layers[i + 1];
                b.tail_w = packed_rows_of(e, nx.wqkv, 3 * d, s); b.tail_b = nx.bqkv; b.tail_s = nx.att_s; b.tail_sb = nx.att_b;
                b.tail_n = 3 * d; b.tail_out = e->qkv.as<float>();
                if (!b.tail_w) return fail("squeezeformer: packing the layer's weights failed");
            }
            b.lens = lens; b.M = M; b.dff = e->cfg.d_ff; b.seq_t = Tq; b.mstride = mstride; b.ktaps = K; b.eps = 1e-5f; b.skip_pad = skm & 1;
            if (!b.head_w) return fail("squeezeformer: packing the layer's weights failed");
            {
                ProfScope ps(e, s, PROF_FFN_HEAD, 4.0 * M * (double)e->cfg.d_ff * d + 2.0 * M * (double)d * d +
                                                      (next_same ? 2.0 * M * (double)(3 * d) * d : 0.0));
                if (!launch_sqz_stage(b, 1, s)) return fail("squeezeformer: the fused end stage rejected the sizes");
            }
            qkv_ready = next_same;
            continue;
        }
        resid_gemm(e, s, e->att.as<float>(), w.wo, w.bo, x, M);
        launch_layernorm(x, w.ln1_w, w.ln1_b, x, M, 1e-5f, 0, 0, nullptr, s);
        // x = LN2(x + FFN1(ada(x)))   (the post-LayerNorm rides on the d_ff-split reduction where ffn_plan.h runs the block split;
        // otherwise ffn() launches it)
        CHK(ffn(e, s, ffn_sqz1(w, M, x)));
        // x = LN3(x + Conv(ada(x)))   symmetric depthwise conv: (K-1)/2 zero rows on both sides of the GLU output
        {
            RowGemmArgs g = rg_args(x, d, w.pw1_w, w.pw1_b, e->glu.as<float>(), d, M, 2 * d);
            g.lnw = w.cv_s; g.lnb = w.cv_b; g.lens = lens; g.seq_t = Tq; g.mstride = mstride; g.out_seq_t = Tq;
            g.out_pad_l = pad_l; g.out_pad_tot = pad;
            rowgemm(e, s, RG_PRO_AFFINE, RG_EPI_GLU, g);
        }
        DWCHK(launch_dwconv_bn_silu(e->glu.as<float>(), w.dw_w, w.dw_b, w.bn_scale, w.bn_shift, e->dwo.as<float>(), B, Tq, K, s,
                                    causal ? w.gconst : nullptr), K);
        resid_gemm(e, s, e->dwo.as<float>(), w.pw2_w, w.pw2_b, x, M, lens, Tq, mstride);
        launch_layernorm(x, w.ln3_w, w.ln3_b, x, M, 1e-5f, 0, 0, nullptr, s);
        // x = LN4(x + FFN2(ada(x)))
        CHK(ffn(e, s, ffn_sqz2(w, M, i == L - 1 ? enc_out : x)));
    }
    LAUNCHCHK();
    return 0;
}

// Squeezeformer chunk step (streaming-trained build), n streams in lock-step: SqueezeformerEncoder.forward_chunk
// (squeezeformer/encoder.py:240-362) with required_cache_size < 0.  Every layer keeps its key/value cache at its OWN frame
// rate (the reference stores the half-rate layers repeat-interleaved and reads every second entry back, :338-347), the cnn
// cache holds the last K-1 adaptive-scaled input rows of the conv module.  TimeReductionLayerStream (k = 1, stride 2) and the
// recovery are chunk-local.
int encode_chunk_squeezeformer(masr_engine* e, hipStream_t s, std::vector<Stream*>& st, const float* feats, int Tc,
                                      float* probs_dev, int32_t* argmax_dev, float* maxprob_dev, float* enc_out_dev) {
    const int n = (int)st.size();
    const int d = e->cfg.d_model, H = e->cfg.heads, L = e->cfg.num_blocks, K = e->cfg.cnn_kernel, pad = K - 1;
    int T0 = 0;
    CHK(embed(e, s, feats, n, Tc, &T0));
    const int Tr = (T0 + 1) / 2;
    for (int i = 0; i < n; ++i)
        if (st[i]->offset + T0 > st[i]->cap) return fail("stream exceeds its max_frames_out / max_pos");
    CHK(ensure_layer_ws(e, n, T0));
    CHK(e->xsave.ensure((size_t)n * T0 * d * sizeof(float)));
    CHK(e->xred.ensure((size_t)n * Tr * d * sizeof(float)));
    CHK(e->attseq.ensure(sizeof(AttSeq) * (size_t)n * L));
    auto reduced = [&](int l) { return e->reduce_idx >= 0 && l >= e->reduce_idx && l < e->recover_idx; };
    std::vector<AttSeq> hs((size_t)n * L);
    std::vector<ChunkWindow> win(n);
    std::vector<int> hfirst(n), hcount(n);
    for (int i = 0; i < n; ++i) {
        win[i] = chunk_window(*st[i], T0);
        // a half-rate layer reads pos_emb[::2] rows minus its queries: ceil((cache_t1 + T0) / 2) - Tr cached entries (encoder.py:338-342)
        CHK(half_rate_window(*st[i], (win[i].cache_t1 + T0 + 1) / 2 - Tr, &hfirst[i], &hcount[i]));
    }
    for (int l = 0; l < L; ++l) {
        const int Tl = reduced(l) ? Tr : T0;
        for (int i = 0; i < n; ++i) {
            const int off = reduced(l) ? st[i]->offset_r : st[i]->offset;
            const int first = reduced(l) ? hfirst[i] : win[i].first_full;       // first cache row attended over
            const int ncached = reduced(l) ? hcount[i] : win[i].cache_t1;
            float* cache = st[i]->att.as<float>() + (size_t)l * st[i]->cap * 2 * d;
            // pos0: key j of a half-rate layer sits at position first_full + 2 j (pos_emb[:, ::2])
            hs[(size_t)l * n + i] = interleaved_seq(e->qkv.as<float>() + (size_t)i * Tl * 3 * d, cache, d, first, ncached, Tl,
                                                    e->att.as<float>() + (size_t)i * Tl * d, win[i].first_full, off);
        }
    }
    const std::vector<float*> hp = cnn_cache_table(st, L, (size_t)pad * d);    // cnn cache bases: current (read) | next (written)
    CHK(e->cnnptrs.ensure(sizeof(float*) * hp.size()));
    CHK(upload_chunk_tables(e, s, hs, hp));
    float* x = e->x.as<float>();
    launch_layernorm(x, e->preln_w, e->preln_b, x, n * T0, 1e-5f, 0, 0, nullptr, s);
    CHK(e->enc.ensure((size_t)n * T0 * d * sizeof(float)));
    int Tq = T0;
    for (int l = 0; l < L; ++l) {
        const SqLayerW& w = e->sq_layers[l];
        if (l == e->reduce_idx) {
            HIPCHK(hipMemcpyAsync(e->xsave.p, x, (size_t)n * T0 * d * sizeof(float), hipMemcpyDeviceToDevice, s));
            launch_time_reduce_dw(x, e->tr_dw_w, e->tr_dw_b, nullptr, e->xred.as<float>(), n, T0, 4, s);
            rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_STORE, rg_args(e->xred.as<float>(), d, e->tr_pw_w, e->tr_pw_b, x, d, n * Tr, d));
            Tq = Tr;
        }
        if (l == e->recover_idx && e->reduce_idx >= 0) {
            rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_STORE, rg_args(x, d, e->rec_w, e->rec_b, e->xred.as<float>(), d, n * Tq, d));
            launch_recover_add(e->xsave.as<float>(), e->xred.as<float>(), x, n, T0, Tq, s);
            Tq = T0;
        }
        const int M = n * Tq;
        const AttSeq* seqs = e->attseq.as<AttSeq>() + (size_t)l * n;
        qkv_proj(e, s, RG_PRO_AFFINE, w.att_s, w.att_b, w.wqkv, w.bqkv, M, seqs, Tq);
        launch_attention(seqs, n, Tq, H, 3 * d, 2 * d, w.ptab, w.pos_u, w.pos_v, 0, reduced(l) ? 2 : 1, s, 256, ATT_REL_POS);
        resid_gemm(e, s, e->att.as<float>(), w.wo, w.bo, x, M);
        launch_layernorm(x, w.ln1_w, w.ln1_b, x, M, 1e-5f, 0, 0, nullptr, s);
        CHK(ffn(e, s, ffn_sqz1(w, M, x)));
        // conv module: [cnn cache | ada(x)] -> pointwise_conv1 + GLU -> causal depthwise + BatchNorm + SiLU -> pointwise_conv2
        float* const* cptr = e->cnnptrs.as<float*>() + (size_t)l * n;
        {   // [cnn cache | ada_scale * x + ada_bias] -> pointwise_conv1 + GLU (+ the new cache) in one launch where the small-M
            // kernel applies, else history / affine rows first
            RowGemmArgs a{};
            a.A = x; a.lda = d; a.lnw = w.cv_s; a.lnb = w.cv_b; a.W = w.pw1_w; a.bias = w.pw1_b; a.C = e->glu.as<float>();
            a.ldc = d; a.M = n * (Tq + pad); a.N = 2 * d; a.alpha = 1.f; a.eps = 1e-5f; a.mstride = 4; a.seq_t = Tq; a.pad = pad;
            a.cache_rd = cptr; a.cache_wr = cptr + (size_t)L * n; a.hist_affine = 1;
            ProfScope ps(e, s, PROF_GEMM, 2.0 * a.M * (double)(2 * d) * d);
            if (!launch_rowgemm(a, RG_PRO_HIST, RG_EPI_GLU, s)) {
                launch_conv_hist(x, w.cv_s, w.cv_b, cptr, cptr + (size_t)L * n, e->lnpad.as<float>(), n, Tq, pad, 1, 1e-5f, s);
                a.A = e->lnpad.as<float>();
                launch_rowgemm(a, RG_PRO_PLAIN, RG_EPI_GLU, s);
            }
        }
        DWCHK(launch_dwconv_bn_silu(e->glu.as<float>(), w.dw_w, w.dw_b, w.bn_scale, w.bn_shift, e->dwo.as<float>(), n, Tq, K, s), K);
        resid_gemm(e, s, e->dwo.as<float>(), w.pw2_w, w.pw2_b, x, M);
        launch_layernorm(x, w.ln3_w, w.ln3_b, x, M, 1e-5f, 0, 0, nullptr, s);
        CHK(ffn(e, s, ffn_sqz2(w, M, l == L - 1 ? e->enc.as<float>() : x)));
    }
    CHK(chunk_ctc(e, s, e->enc.as<float>(), n * T0, probs_dev, argmax_dev, maxprob_dev, enc_out_dev));
    advance_half_rate(st, win, T0, Tr);
    return 0;
}

}  // namespace masr
