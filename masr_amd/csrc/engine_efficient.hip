// libmasr_hip.so -- engine, Efficient Conformer (model_kind 2): full-context forward and chunk step (weights: engine_conformer.hip).  Host code only (file map: engine_state.h).
#include "engine_encoder.h"

namespace masr {

// Efficient Conformer, full-context forward (efficient_conformer/encoder.py:213-265): Conformer layers with
// grouped attention in the first n_group_layers blocks, a stride-2 conv block at stride_idx (AvgPool residual),
// half frame rate + kernel 7 afterwards.  Weights share the Conformer key names (masr_finalize).
int encode_full_efficient(masr_engine* e, hipStream_t s, const float* feats, const int* lens, int B, int T,
                                 float* enc_out, int chunk) {
    const int d = e->cfg.d_model, H = e->cfg.heads, G = e->group_size;
    const bool causal = e->cfg.causal != 0;
    int T0 = 0;
    CHK(embed(e, s, feats, B, T, &T0));
    if (T0 >= e->cfg.max_pos) return fail("sequence longer than max_pos");
    CHK(ensure_layer_ws(e, B, T0));
    const int Tg = (T0 + G - 1) / G, Tpad = Tg * G;
    const size_t plane = (size_t)B * Tpad * d;
    CHK(e->attseq.ensure(sizeof(AttSeq) * 2 * B));
    CHK(e->qplanes.ensure(3 * plane * sizeof(float)));
    CHK(e->attp.ensure(plane * sizeof(float)));
    CHK(e->xsave.ensure((size_t)B * ((T0 + 1) / 2) * d * sizeof(float)));
    float* x = e->x.as<float>();
    float* qp = e->qplanes.as<float>();
    AttSeq* seq_g = e->attseq.as<AttSeq>();
    AttSeq* seq_r = seq_g + B;
    HIPCHK(hipMemsetAsync(qp, 0, 3 * plane * sizeof(float), s));     // time padding rows of q/k/v stay zero (pad4group)
    int Tq = T0, mstride = 4, pstride = 1;
    launch_attseq_grouped(seq_g, qp, qp + plane, qp + 2 * plane, e->attp.as<float>(), lens, B, Tg, G, mstride, s);
    launch_attseq_full(seq_r, e->qkv.as<float>(), e->att.as<float>(), lens, B, Tq, mstride, s);
    // streaming: False build (symmetric conv): the (K - 1) / 2 zero rows on both sides of every sequence in the GLU buffer are
    // cleared once per frame rate / kernel size (the layers only ever write the real rows)
    if (!causal) HIPCHK(hipMemsetAsync(e->glu.p, 0, (size_t)B * (Tq + e->cfg.cnn_kernel - 1) * d * sizeof(float), s));
    const int L = e->cfg.num_blocks;
    for (int i = 0; i < L; ++i) {
        const LayerW& w = e->layers[i];
        int M = B * Tq;
        const int Ki = layer_kernel(e, i);
        // enough row blocks for the full (non d_ff-split) FFN launch: the Conformer's fused launches (key 31 = 0: separate ones)
        const bool fused = knobs().efficient_fused && !knobs().no_chain && !knobs().no_ffn_head && i != e->stride_idx &&
                           ffn_full_row_blocks(knobs(), M) && (Ki == 15 || Ki == 7) && d == 256;
        const EncodeCtx ctx0{B, Tq, lens};
        // regular layers: LayerNorm + fused QKV projection ride on the first FFN kernel (tail stage), like the Conformer
        FfnArgs f1 = ffn_macaron(w, M);
        if (!layer_grouped(e, i)) {
            f1.tail = qkv_tail(e, w, e->qkv.as<float>(), 3 * d);
        } else if (knobs().efficient_fused) {
            // grouped layers: the same tail stage writes q | k | v PLANAR into the time-padded buffers of the grouped attention
            // (round 4; ffn_pc.hip only -- ffn_plan.h keeps the separate projection where the two-chain kernel is switched on)
            f1.tail = qkv_tail(e, w, qp, d);
            f1.tail.plane_stride = (long)plane; f1.tail.seq_t = Tq; f1.tail.pad_t = Tpad - Tq;
        }
        const FfnDone r1 = ffn(e, s, f1);
        CHK(r1);
        if (layer_grouped(e, i)) {
            if (Tq != T0) return fail("grouped attention after the stride layer is not supported");
            // q | k | v -> planar, time-padded buffers; attention over T/3 positions with d_k' = 192
            if (!r1.tail_done)
                {
                    RowGemmArgs g = rg_args(x, d, w.wqkv, w.bqkv, qp, d, M, 3 * d);
                    g.lnw = w.ln_mha_w; g.lnb = w.ln_mha_b; g.mstride = mstride; g.out_seq_t = Tq; g.out_pad_tot = Tpad - Tq;
                    g.plane_cols = d; g.plane_stride = (long)plane;
                    rowgemm(e, s, RG_PRO_LN, RG_EPI_STORE, g);
                }
            {
                ProfScope ps(e, s, PROF_ATT, 6.0 * d * (double)Tq * Tq * B / G);
                launch_attention_grouped(seq_g, B, Tg, H, G, w.ptab, Tq, w.pos_u, w.pos_v, s, chunk);
            }
            if (fused) mhsa_out_pw1(e, s, w, ctx0, mstride, Ki, e->attp.as<float>(), Tq, Tpad);
            else resid_gemm(e, s, e->attp.as<float>(), w.wo, w.bo, x, M, nullptr, 0, mstride, Tq, Tpad);
        } else {
            if (!r1.tail_done) mhsa(e, s, w, M);
            {
                ProfScope ps(e, s, PROF_ATT, 6.0 * d * (double)Tq * Tq * B);
                launch_attention(seq_r, B, Tq, H, 3 * d, 3 * d, w.ptab, w.pos_u, w.pos_v, chunk, pstride, s, 256, ATT_REL_POS);
            }
            if (fused) mhsa_out_pw1(e, s, w, ctx0, mstride, Ki);
            else mhsa_out(e, s, w, M);
        }
        if (fused) {
            // like the offline Conformer layer: [out-proj + residual -> LN -> pw1 -> GLU] was one kernel; the rest of the conv
            // module is the head stage of the second FFN launch (15 taps before, 7 behind the stride layer)
            FfnArgs f2 = ffn_final(w, M);
            f2.head = conv_head(e, w, lens, Tq, Ki, mstride);
            CHK(ffn(e, s, f2));
            launch_layernorm(x, w.ln_fin_w, w.ln_fin_b, x, M, 1e-5f, 0, 0, nullptr, s);
            continue;
        }
        if (i == e->stride_idx) {
            // StrideConformerEncoderLayer (encoder.py:454-545): x = AvgPool(x) + conv_module_stride2(LN(x))
            const int K = layer_kernel(e, i), pad = K - 1, T2 = (Tq + 1) / 2;
            if (causal)      // the K - 1 history rows go through pointwise_conv1 + GLU like the reference's left padding
                {
                    RowGemmArgs g = rg_args(x, d, w.pw1_w, w.pw1_b, e->glu.as<float>(), d, B * (Tq + pad), 2 * d);
                    g.lnw = w.ln_conv_w; g.lnb = w.ln_conv_b; g.lens = lens; g.seq_t = Tq; g.pad = pad; g.mstride = mstride;
                    rowgemm(e, s, RG_PRO_LN_PAD, RG_EPI_GLU, g);
                }
            else             // symmetric: the real rows land between (K - 1) / 2 zero rows on either side (same stride-2 window sum)
                {
                    RowGemmArgs g = rg_args(x, d, w.pw1_w, w.pw1_b, e->glu.as<float>(), d, M, 2 * d);
                    g.lnw = w.ln_conv_w; g.lnb = w.ln_conv_b; g.lens = lens; g.seq_t = Tq; g.mstride = mstride;
                    g.out_seq_t = Tq; g.out_pad_l = pad / 2; g.out_pad_tot = pad;
                    rowgemm(e, s, RG_PRO_LN_PAD, RG_EPI_GLU, g);
                }
            if (e->conv_bn)
                launch_dwconv_stride2_bn_silu(e->glu.as<float>(), w.dw_w, w.dw_b, w.cln_w, w.cln_b, e->dwo.as<float>(), B, Tq, K, s);
            else
                launch_dwconv_stride2_ln_silu(e->glu.as<float>(), w.dw_w, w.dw_b, w.cln_w, w.cln_b, e->dwo.as<float>(), B, Tq, K,
                                              1e-5f, s);
            launch_avgpool2(x, e->xsave.as<float>(), B, Tq, s);
            Tq = T2; mstride *= 2; pstride *= 2; M = B * Tq;
            if (!causal && i + 1 < L)     // half rate, kernel 7 from here on: a new padded layout (no layer behind a stride layer that is last)
                HIPCHK(hipMemsetAsync(e->glu.p, 0, (size_t)B * (Tq + layer_kernel(e, i + 1) - 1) * d * sizeof(float), s));
            resid_gemm(e, s, e->dwo.as<float>(), w.pw2_w, w.pw2_b, e->xsave.as<float>(), M, lens, Tq, mstride);
            launch_attseq_full(seq_r, e->qkv.as<float>(), e->att.as<float>(), lens, B, Tq, mstride, s);
        } else {
            CHK(conv_module(e, s, w, ctx0, false, layer_kernel(e, i), mstride));
        }
        CHK(ffn(e, s, ffn_final(w, M)));
        launch_layernorm(x, w.ln_fin_w, w.ln_fin_b, x, M, 1e-5f, 0, 0, nullptr, s);
    }
    launch_layernorm(x, e->after_w, e->after_b, enc_out, B * Tq, 1e-5f, 0, 0, nullptr, s);
    LAUNCHCHK();
    return 0;
}

// Efficient-Conformer chunk step, n streams in lock-step: EfficientConformerEncoder.forward_chunk
// (efficient_conformer/encoder.py:267-392) with required_cache_size < 0.  Grouped layers keep PLANAR key / value caches at the
// input frame rate (the flat regrouping runs over cache + chunk), layers behind the stride layer keep interleaved k|v rows
// at half the rate (the reference stores them repeat-interleaved, :370); cnn caches hold each layer's own K-1 rows.
int encode_chunk_efficient(masr_engine* e, hipStream_t s, std::vector<Stream*>& st, const float* feats, int Tc,
                                  float* probs_dev, int32_t* argmax_dev, float* maxprob_dev, float* enc_out_dev) {
    const int n = (int)st.size();
    const int d = e->cfg.d_model, H = e->cfg.heads, L = e->cfg.num_blocks, G = e->group_size;
    // conv2d8 gives 7 frames per 67-frame window: the half-rate layers' caches of an odd chunk do not line up with the next
    // chunk's positions, and the reference's chunk forward fails there (a size mismatch in the attention scores).  conv2d keeps
    // its behaviour (only a short last chunk is odd); conv2d6 gives 10 frames per window.
    for (int i = 0; i < n; ++i)
        if (e->input_layer != IL_CONV2D && st[i]->offset % 2 != 0)
            return fail("efficient_conformer: a chunk after one of an odd number of encoder frames (conv2d8: 7 per 67-frame window) "
                        "is not defined by the reference; use conv2d or conv2d6 for chunked streaming");
    int T0 = 0;
    CHK(embed(e, s, feats, n, Tc, &T0));
    const int T2 = (T0 + 1) / 2, Tg = (T0 + G - 1) / G, Tpad = Tg * G;
    for (int i = 0; i < n; ++i)
        if (st[i]->offset + T0 + G > st[i]->cap) return fail("stream exceeds its max_frames_out / max_pos");
    CHK(ensure_layer_ws(e, n, T0));
    const size_t plane = (size_t)n * Tpad * d;
    CHK(e->qplanes.ensure(3 * plane * sizeof(float)));
    CHK(e->attp.ensure(plane * sizeof(float)));
    CHK(e->xsave.ensure((size_t)n * T2 * d * sizeof(float)));
    CHK(e->attseq.ensure(sizeof(AttSeq) * (size_t)n * L));
    float* qp = e->qplanes.as<float>();
    HIPCHK(hipMemsetAsync(qp, 0, 3 * plane * sizeof(float), s));      // time padding rows of the new q / k / v stay zero
    // (masr_create keeps stride_idx in [0, L): one layer halves the rate, so the step always ends on n * T2 rows)
    auto rate = [&](int l) { return l > e->stride_idx ? 2 : 1; };
    const int padmax = e->cfg.cnn_kernel - 1;
    std::vector<AttSeq> hs((size_t)n * L);
    std::vector<PlaneCopy> pcs((size_t)n * e->n_group_layers);
    std::vector<ChunkWindow> win(n);
    std::vector<int> hfirst(n), hcount(n);
    for (int i = 0; i < n; ++i) {
        win[i] = chunk_window(*st[i], T0);
        // layers behind the stride layer read att_cache[:, :, ::2]: ceil(cache_t1 / 2) entries (encoder.py:353)
        CHK(half_rate_window(*st[i], (win[i].cache_t1 + 1) / 2, &hfirst[i], &hcount[i]));
    }
    for (int l = 0; l < L; ++l) {
        if (layer_grouped(e, l) && rate(l) != 1) return fail("grouped attention after the stride layer is not supported");
        for (int i = 0; i < n; ++i) {
            AttSeq& a = hs[(size_t)l * n + i];
            float* cache = st[i]->att.as<float>() + (size_t)l * st[i]->cap * 2 * d;
            if (layer_grouped(e, l)) {
                // the flat regrouping [T, 256] -> [T / 3, 4, 192] runs over (kept cache + chunk): it starts at the first kept row
                float* kpl = cache;
                float* vpl = cache + (size_t)st[i]->cap * d;
                a.q = qp + (size_t)i * Tpad * d;
                a.k = kpl + (size_t)win[i].first_full * d;
                a.v = vpl + (size_t)win[i].first_full * d;
                a.out = e->attp.as<float>() + (size_t)i * Tpad * d;
                a.nq = Tg;
                a.nk = (win[i].cache_t1 + T0 + G - 1) / G;
                a.klen = a.nk;
                a.pos0 = win[i].first_full;
                a.q_abs0 = 0;
                a.pad_ = win[i].cache_t1 + T0;                 // true number of keys (rows of P behind it read as zero)
                PlaneCopy& c = pcs[(size_t)l * n + i];
                c.src_k = qp + plane + (size_t)i * Tpad * d;
                c.src_v = qp + 2 * plane + (size_t)i * Tpad * d;
                c.dst_k = kpl + (size_t)st[i]->offset * d;
                c.dst_v = vpl + (size_t)st[i]->offset * d;
            } else {
                const int Tl = rate(l) == 2 ? T2 : T0;
                const int off = rate(l) == 2 ? st[i]->offset_r : st[i]->offset;
                const int first = rate(l) == 2 ? hfirst[i] : win[i].first_full;
                const int ncached = rate(l) == 2 ? hcount[i] : win[i].cache_t1;
                a = interleaved_seq(e->qkv.as<float>() + (size_t)i * Tl * 3 * d, cache, d, first, ncached, Tl,
                                    e->att.as<float>() + (size_t)i * Tl * d, win[i].first_full, off);
            }
        }
    }
    const std::vector<float*> hp = cnn_cache_table(st, L, (size_t)padmax * d);   // cnn cache bases: current (read) | next (written)
    CHK(e->cnnptrs.ensure(sizeof(float*) * hp.size() + sizeof(PlaneCopy) * pcs.size()));
    PlaneCopy* pc_dev = reinterpret_cast<PlaneCopy*>(e->cnnptrs.as<float*>() + hp.size());
    CHK(upload_chunk_tables(e, s, hs, hp, pc_dev, pcs.data(), sizeof(PlaneCopy) * pcs.size()));
    float* x = e->x.as<float>();
    for (int l = 0; l < L; ++l) {
        const LayerW& w = e->layers[l];
        const int Tq = rate(l) == 2 ? T2 : T0;
        int M = n * Tq;
        const AttSeq* seqs = e->attseq.as<AttSeq>() + (size_t)l * n;
        CHK(ffn(e, s, ffn_macaron(w, M)));
        if (layer_grouped(e, l)) {
            {
                RowGemmArgs g = rg_args(x, d, w.wqkv, w.bqkv, qp, d, M, 3 * d);
                g.lnw = w.ln_mha_w; g.lnb = w.ln_mha_b; g.out_seq_t = Tq; g.out_pad_tot = Tpad - Tq; g.plane_cols = d;
                g.plane_stride = (long)plane;
                rowgemm(e, s, RG_PRO_LN, RG_EPI_STORE, g);
            }
            launch_kv_append_planar(pc_dev + (size_t)l * n, n, Tq, s);
            launch_attention_grouped(seqs, n, Tg, H, G, w.ptab, 0, w.pos_u, w.pos_v, s);
            resid_gemm(e, s, e->attp.as<float>(), w.wo, w.bo, x, M, nullptr, 0, 4, Tq, Tpad);
        } else {
            mhsa(e, s, w, M, seqs, Tq);                 // k | v rows go straight to the streams' caches
            launch_attention(seqs, n, Tq, H, 3 * d, 2 * d, w.ptab, w.pos_u, w.pos_v, 0, rate(l), s, 256, ATT_REL_POS);
            mhsa_out(e, s, w, M);
        }
        const int K = layer_kernel(e, l), pad = K - 1;
        float* const* cptr = e->cnnptrs.as<float*>() + (size_t)l * n;
        if (l == e->stride_idx) {
            launch_cnn_cache_move(cptr, e->lnpad.as<float>(), n, Tq, pad, 0, s);
            // StrideConformerEncoderLayer (encoder.py:454-545): x = AvgPool(x) + conv_module_stride2([cache | LN(x)])
            launch_layernorm(x, w.ln_conv_w, w.ln_conv_b, e->lnpad.as<float>(), M, 1e-5f, Tq, pad, nullptr, s);
            rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_GLU,
                    rg_args(e->lnpad.as<float>(), d, w.pw1_w, w.pw1_b, e->glu.as<float>(), d, n * (Tq + pad), 2 * d));
            launch_cnn_cache_move(cptr + (size_t)L * n, e->lnpad.as<float>(), n, Tq, pad, 1, s);
            if (e->conv_bn)
                launch_dwconv_stride2_bn_silu(e->glu.as<float>(), w.dw_w, w.dw_b, w.cln_w, w.cln_b, e->dwo.as<float>(), n, Tq, K, s);
            else
                launch_dwconv_stride2_ln_silu(e->glu.as<float>(), w.dw_w, w.dw_b, w.cln_w, w.cln_b, e->dwo.as<float>(), n, Tq, K,
                                              1e-5f, s);
            launch_avgpool2(x, e->xsave.as<float>(), n, Tq, s);
            M = n * T2;
            resid_gemm(e, s, e->dwo.as<float>(), w.pw2_w, w.pw2_b, e->xsave.as<float>(), M);
        } else {
            CHK(conv_module_stream(e, s, w, n, Tq, cptr, cptr + (size_t)L * n, K));
        }
        CHK(ffn(e, s, ffn_final(w, M, x)));
    }
    CHK(e->enc.ensure((size_t)n * T2 * d * sizeof(float)));
    launch_layernorm(x, e->after_w, e->after_b, e->enc.as<float>(), n * T2, 1e-5f, 0, 0, nullptr, s);
    CHK(chunk_ctc(e, s, e->enc.as<float>(), n * T2, probs_dev, argmax_dev, maxprob_dev, enc_out_dev));
    advance_half_rate(st, win, T0, T2);
    return 0;
}

}  // namespace masr
