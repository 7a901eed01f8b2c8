// libmasr_hip.so -- engine, what the attention families share: the GEMM and row-block calls, the FFN block, the subsampling front-end, the conv
// module and the attention projections, the finalize pieces and the chunk steps' tables.  Host code only (file map: engine_state.h).
#include "engine_encoder.h"

namespace masr {

void gemm(masr_engine* e, hipStream_t s, const float* A, int lda, const float* W, const float* bias, float* C, int ldc,
          int M, int N, int K, int act, float alpha, const float* R, int ldr, int kind,
          const int* lens, int mask_tp) {
    GemmArgs a{};
    a.A = A; a.W = W; a.bias = bias; a.C = C; a.R = R; a.lens = lens;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc; a.ldr = ldr;
    a.act = act; a.alpha = alpha; a.mask_tp = mask_tp;
    ProfScope ps(e, s, kind, 2.0 * M * (double)N * K);
    if (knobs().bf16x3 && launch_gemm_bf16x3(a, A_PLAIN, s)) return;
    launch_gemm(a, A_PLAIN, EPI_STD, s);
}

void gemm_rows(masr_engine* e, hipStream_t s, const float* pool, int lda, const int64_t* rows, int64_t n_rows, const float* W,
               const float* bias, float* C, int ldc, int M, int N, int K) {
    GemmArgs a{};
    a.A = pool; a.W = W; a.bias = bias; a.C = C; a.rows = rows; a.n_rows = n_rows;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc;
    a.act = ACT_NONE; a.alpha = 1.f;
    ProfScope ps(e, s, PROF_GEMM, 2.0 * M * (double)N * K);
    launch_gemm(a, A_ROWS, EPI_STD, s);
}

int enc_dim(const masr_engine* e) {      // width of the encoder output rows
    return e->cfg.model_kind == 3 ? e->cfg.d_model * (e->cfg.causal ? 1 : 2) : e->cfg.d_model;
}
int layer_kernel(const masr_engine* e, int i) {          // efficient conformer: kernel // stride after the stride layer
    return (e->cfg.model_kind == 2 && e->stride_idx >= 0 && i > e->stride_idx) ? e->cfg.cnn_kernel / 2 : e->cfg.cnn_kernel;
}
bool layer_grouped(const masr_engine* e, int i) { return e->cfg.model_kind == 2 && i < e->n_group_layers; }

// the common prefix of a row-block launch, C[M, N] = A[M, 256] . W[N, 256]^T + bias, with the defaults every launch but the odd one
// takes (alpha 1, LayerNorm eps 1e-5, 4 feature frames per encoder frame in the pad masks); the rest is filled in by field name
RowGemmArgs rg_args(const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int M, int N) {
    RowGemmArgs a{};
    a.A = A; a.lda = lda; a.W = W; a.bias = bias; a.C = C; a.ldc = ldc; a.M = M; a.N = N;
    a.alpha = 1.f; a.eps = 1e-5f; a.mstride = 4;
    return a;
}
void rowgemm(masr_engine* e, hipStream_t s, int pro, int epi, RowGemmArgs a, int kind) {
    // full row-block launches (the K-split kernel of few row blocks reads W itself) take the packed copy of their weights
    if (knobs().rowgemm_packed && a.M >= 112 * 32 && pro != RG_PRO_HIST && pro != RG_PRO_DWCONV && (epi == RG_EPI_CTC || a.N % 256 == 0))
        a.Wp = packed_rows_of(e, a.W, a.N, s);
    ProfScope ps(e, s, kind, 2.0 * a.M * (double)a.N * 256);
    launch_rowgemm(a, pro, epi, s);
}

// x <- R + mask(A . W^T + bias) on M rows of d: the out-projection and pointwise_conv2 launches (mask: frames at or past lens
// of sequences of mask_tp frames, mstride feature frames per encoder frame; a_seq_t rows of A per sequence every a_seq_stride)
void resid_gemm(masr_engine* e, hipStream_t s, const float* A, const float* W, const float* bias, const float* R, int M,
                const int* lens, int mask_tp, int mstride, int a_seq_t, int a_seq_stride) {
    const int d = e->cfg.d_model;
    RowGemmArgs g = rg_args(A, d, W, bias, e->x.as<float>(), d, M, d);
    g.R = R; g.ldr = d; g.lens = lens; g.mask_tp = mask_tp; g.mstride = mstride; g.a_seq_t = a_seq_t; g.a_seq_stride = a_seq_stride;
    rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_RESID, g);
}

// the FFNs of a layer as ffn() calls on M rows: a call site adds what it wants beside the block (post, tail, head)
FfnArgs ffn_of(int M, const float* lnw, const float* lnb, const float* w1, const float* b1, const float* w2, const float* b2) {
    FfnArgs a;
    a.M = M; a.lnw = lnw; a.lnb = lnb; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
    return a;
}
FfnArgs ffn_macaron(const LayerW& w, int M) { return ffn_of(M, w.ln_ffm_w, w.ln_ffm_b, w.ffm_w1, w.ffm_b1, w.ffm_w2, w.ffm_b2); }
// (y: where the layer's norm_final goes when it rides on this call -- a.post; nullptr: the caller runs or defers it)
FfnArgs ffn_final(const LayerW& w, int M, float* y) {
    FfnArgs a = ffn_of(M, w.ln_ff_w, w.ln_ff_b, w.ff_w1, w.ff_b1, w.ff_w2, w.ff_b2);
    a.post = {w.ln_fin_w, w.ln_fin_b, y};
    return a;
}
// tail stage of a layer's first FFN: the attention block's LayerNorm + fused QKV projection into out [M, ldo]
FfnTail qkv_tail(const masr_engine* e, const LayerW& w, float* out, int ldo) {
    FfnTail t{};
    t.lnw = w.ln_mha_w; t.lnb = w.ln_mha_b; t.W = w.wqkv; t.bias = w.bqkv; t.out = out; t.N = 3 * e->cfg.d_model; t.ldo = ldo;
    return t;
}

// head stage of a layer's second FFN: the conv module behind pointwise_conv1 + GLU, on the offline GLU buffer (whose causal
// history rows are the constant glu(bias), not materialised)
FfnHead conv_head(const masr_engine* e, const LayerW& w, const int* lens, int Tq, int ktaps, int mstride) {
    FfnHead h{};
    h.glu = e->glu.as<float>(); h.dw_w = w.dw_w; h.dw_b = w.dw_b; h.lnw = w.cln_w; h.lnb = w.cln_b;
    h.gconst = e->cfg.causal ? w.gconst : nullptr; h.W = w.pw2_w; h.bias = w.pw2_b;
    h.lens = lens; h.seq_t = Tq; h.ktaps = ktaps; h.mstride = mstride; h.norm = e->conv_bn ? 1 : 0;
    return h;
}

// The fused FFN block on the engine's residual stream e->x (a.x and a.dff are filled in here).  ffn_plan.h chooses the kernel;
// a.post: fused into the split-mode reduction of small M, otherwise launched behind the block; a.tail (fused QKV projection,
// ffn_pc.hip TAIL): see FfnDone; a.head: the kernel's head stage or two launches of its own in front of the block
FfnDone ffn(masr_engine* e, hipStream_t s, FfnArgs a) {
    const int d = e->cfg.d_model, M = a.M;
    float* x = a.x = e->x.as<float>();
    a.dff = e->cfg.d_ff;
    const FfnTail tail = a.tail;          // as asked for: a.tail / a.head become what the kernel is to run, with W in its order
    const FfnHead head = a.head;
    const FfnPlan plan = ffn_plan(knobs(), d, a.dff, M, {a.affine, tail.W ? tail.N : 0, tail.plane_stride > 0, head.glu ? head.ktaps : 0, head.norm});
    if (!plan.tail_in_kernel) a.tail = FfnTail{};
    if (!plan.head_in_kernel) a.head = FfnHead{};
    if (head.glu && !plan.head_in_kernel) {
        // the rest of the conv module as its own two launches: depthwise conv + LayerNorm + SiLU, pointwise_conv2 + mask + residual
        CHK(e->dwo.ensure((size_t)M * d * sizeof(float)));
        if (head.norm == 1)
            DWCHK(launch_dwconv_bn_silu(head.glu, head.dw_w, head.dw_b, head.lnw, head.lnb, e->dwo.as<float>(), M / head.seq_t, head.seq_t,
                                        head.ktaps, s, head.gconst), head.ktaps);
        else
            DWCHK(launch_dwconv_ln_silu(head.glu, head.dw_w, head.dw_b, head.lnw, head.lnb, e->dwo.as<float>(), M / head.seq_t, head.seq_t,
                                        head.ktaps, 1e-5f, s, head.gconst), head.ktaps);
        resid_gemm(e, s, e->dwo.as<float>(), head.W, head.bias, x, M, head.lens, head.lens ? head.seq_t : 0, head.mstride);
    }
    if (tail.W && tail.pre_lnw && !plan.tail_in_kernel)          // the deferred LayerNorm of the previous layer, as its own launch
        launch_layernorm(x, tail.pre_lnw, tail.pre_lnb, x, M, 1e-5f, 0, 0, nullptr, s);
    if (plan.nsplit > 1) {
        CHK(e->ffpart.ensure((size_t)plan.nsplit * M * d * sizeof(float)));
        a.partial = e->ffpart.as<float>(); a.nsplit = plan.nsplit;
    }
    if (plan.split_head) {
        CHK(e->xh.ensure((size_t)M * d * sizeof(float)));
        a.head.xout = e->xh.as<float>();
    }
    ProfScope ps(e, s, plan.prof, 4.0 * M * (double)a.dff * d + (plan.tail_in_kernel ? 2.0 * M * (double)tail.N * d : 0.0) +
                                      (plan.head_in_kernel ? 2.0 * M * (double)d * d : 0.0));
    // each kernel reads fragment-ordered copies of its own (built on first use, + 4 MB per FFN), and so do the row-local stages
    // that ride on the launch.  done: what the launcher says it ran -- 1 the post LayerNorm (split reduction), 2 the tail, 4 the head
    int done = 0;
    switch (plan.kernel) {
    case FFN_X3: {
        const size_t bytes = ffn_x3_packed_elems(a.dff) * sizeof(unsigned short);      // (hi, lo) pieces
        const float *w1 = a.w1, *w2 = a.w2;
        const PackedW* pk = packed_of(e, PACK_FFN_X3, w1, bytes, bytes, s, [&](const PackedW& p, hipStream_t st) {
            launch_pack_ffn_x3(w1, w2, p.a.as<unsigned short>(), p.b.as<unsigned short>(), a.dff, st);
        });
        if (!pk) return 1;
        a.w1 = pk->a.as<float>(); a.w2 = pk->b.as<float>();
        if (!launch_ffn_x3(a, s)) return fail("ffn(): the split-bf16 FFN kernel rejected the sizes");
        break;
    }
    case FFN_COOP: {
        // ffn_pc.hip's copies (W2 is shared with it) + the 16 x 16 x 4 fragment order of W1
        const float* w1 = a.w1;
        CHK(packed_ffn_of(e, w1, a.w2, s, &a.w1, &a.w2));
        const PackedW* pc = packed_of(e, PACK_FFN_COOP_W1, w1, (size_t)a.dff * d * sizeof(float), 0, s,
                                      [&](const PackedW& p, hipStream_t st) { launch_pack_ffn_coop_w1(w1, p.a.as<float>(), a.dff, st); });
        if (!pc) return 1;
        a.w1 = pc->a.as<float>();
        launch_ffn_coop(a, s);
        launch_ffn_reduce(a, s);
        done = 1;
        break;
    }
    case FFN_DUAL:
        CHK(packed_ffn_of(e, a.w1, a.w2, s, &a.w1, &a.w2, PACK_FFN_DUAL, launch_pack_ffn_dual));
        if (plan.tail_in_kernel) {
            const PackedW* tw = packed_of(e, PACK_ROWS_DUAL, tail.W, (size_t)768 * d * sizeof(float), 0, s,
                                          [&](const PackedW& p, hipStream_t st) { launch_pack_rows_dual(tail.W, p.a.as<float>(), st); });
            if (!tw) return 1;
            a.tail.W = tw->a.as<float>();
        }
        if (plan.head_in_kernel && !(a.head.W = packed_rows_of(e, head.W, d, s))) return 1;
        if ((done = launch_ffn_dual(a, s)) < 0) return fail("ffn(): the two-chain FFN kernel rejected the launch");
        break;
    case FFN_ROWS16:
        CHK(packed_ffn_of(e, a.w1, a.w2, s, &a.w1, &a.w2, PACK_FFN16, launch_pack_ffn16));
        if (plan.tail_in_kernel && !(a.tail.W = packed_rows_of(e, tail.W, tail.N, s, PACK_ROWS16))) return 1;
        if (plan.head_in_kernel && !(a.head.W = packed_rows_of(e, head.W, d, s, PACK_ROWS16))) return 1;
        if ((done = launch_ffn16(a, s)) < 0) return fail("ffn(): the 16-row FFN kernel rejected the launch");
        break;
    case FFN_PC:
        if ((a.packed = plan.packed)) {
            CHK(packed_ffn_of(e, a.w1, a.w2, s, &a.w1, &a.w2));
            if (plan.tail_in_kernel && tail.N % 256 == 0 && !(a.tail.W = packed_rows_of(e, tail.W, tail.N, s))) return 1;
            if (plan.head_in_kernel && !(a.head.W = packed_rows_of(e, head.W, d, s))) return 1;
        }
        if ((done = launch_ffn_fused(a, s)) < 0) return fail("ffn(): launch rejected");
        break;
    }
    if (plan.head_in_kernel && !(done & 4)) return fail("ffn(): head stage was not launched");
    if (a.post.y && !(done & 1)) launch_layernorm(x, a.post.lnw, a.post.lnb, a.post.y, M, 1e-5f, 0, 0, nullptr, s);
    FfnDone r;
    r.tail_done = done == 2; r.head_done = plan.head_in_kernel;
    return r;
}

// W [N = 256, K] in the row-block kernel's fragment order (gemm_f32.hip conv2_rows_kernel): the subsampling convs and the embed projection
static const float* packed_conv2_rows_of(masr_engine* e, const float* W, int N, int K, hipStream_t s) {
    const PackedW* pk = packed_of(e, PACK_CONV2_ROWS, W, (size_t)N * K * sizeof(float), 0, s,
                                  [&](const PackedW& p, hipStream_t st) { launch_pack_conv2_rows(W, p.a.as<float>(), K, st); });
    return pk ? pk->a.as<float>() : nullptr;
}

// one subsampling conv over channels-last activations as an implicit GEMM (a: geometry, C, lens; amode A_CONV2 / A_CONV5):
// full-width row blocks with the weights packed at first use, split K for few rows.  feats [nseq, a.Tin, n_mels] given: the
// conv reads conv1's output (computed in the row blocks' gather, or by conv1 into x1 first); else it reads x_in.
static int subsampling_conv(masr_engine* e, hipStream_t s, GemmArgs a, int amode, int nseq, const float* feats, const float* x_in) {
    const int d = e->cfg.d_model;
    const int tiles = ((a.M + 63) / 64) * ((a.N + 63) / 64);
    if (tiles >= 640 && knobs().conv2_rows && a.N == 256) {   // full-width row blocks: the weights in the kernel's fragment order, packed at first use
        if (!(a.Wp = packed_conv2_rows_of(e, a.W, a.N, a.K, s))) return 1;
        if (feats && amode == A_CONV2 && knobs().conv1_fused && !knobs().bf16x3 && gemm_conv2_rows(a)) {    // conv1 computed in the row blocks' A gather: no x1, no conv1 launch
            a.feats = feats; a.mean = e->cmvn_mean; a.istd = e->cmvn_istd; a.c1w = e->conv1_w; a.c1b = e->conv1_b;
            a.Fin = e->cfg.n_mels;
        }
    }
    if (!a.feats) {
        if (feats) {        // conv1 as its own launch into x1
            CHK(e->x1.ensure((size_t)nseq * a.T1 * a.F1 * d * sizeof(float)));
            // (conv1_kernel's thread = output channel: more than 256 channels take the wide kernel)
            (d > 256 ? launch_conv1_wide : launch_conv1)(feats, e->cmvn_mean, e->cmvn_istd, e->conv1_w, e->conv1_b, e->x1.as<float>(),
                                                         nseq, a.Tin, e->cfg.n_mels, d, s);
            a.A = e->x1.as<float>();
        } else {
            a.A = x_in;
        }
    }
    ProfScope ps(e, s, PROF_CONV2, 2.0 * a.M * (double)a.N * a.K);
    if (knobs().bf16x3 && amode == A_CONV2 && tiles >= 640 && launch_gemm_bf16x3(a, A_CONV2, s)) {
        // exploratory split-bf16 mode
    } else if (tiles < 640) {
        // streaming chunk steps: ~1 workgroup of 4 waves per CU leaves the load -> LDS -> MFMA chain of every 32-wide K slab
        // exposed (2.5 us per slab, 72 slabs); split K so that ~4-5 workgroups per CU overlap each other's latencies
        const int nsplit = std::min(8, std::max(2, 1280 / tiles));
        CHK(e->ffpart.ensure((size_t)nsplit * a.M * a.N * sizeof(float)));
        launch_gemm_splitk(a, e->ffpart.as<float>(), nsplit, s, amode);
    } else {
        launch_gemm(a, amode, EPI_STD, s);
    }
    return 0;
}

// feats [nseq, T, 80] -> x [nseq*Tq, d] (embed incl. x*sqrt(d)).  skip_lens: lengths in conv2d units (sub_lens)
int embed(masr_engine* e, hipStream_t s, const float* feats, int nseq, int T, int* Tq_out, const int* skip_lens) {
    const int il = e->input_layer, d = e->cfg.d_model, F = e->cfg.n_mels, F1 = (F - 1) / 2, F2 = sub_bins(il, F);
    const int T1 = (T - 1) / 2, Tq = sub_frames(il, T);
    if (T < sub_min_frames(il) || Tq <= 0)
        return fail("input too short for the subsampling front-end (need >= " + std::to_string(sub_min_frames(il)) + " frames)");
    // conv2d8: the second conv runs as conv2d's (19 bins, T1 -> (T1 - 1) / 2 frames), the third on its output
    const int Fc = il == IL_CONV2D8 ? (F1 - 1) / 2 : F2, Tc = il == IL_CONV2D8 ? (T1 - 1) / 2 : Tq;
    const int M = nseq * Tq;
    CHK(e->x2.ensure((size_t)nseq * Tc * Fc * d * sizeof(float)));
    CHK(e->x.ensure((size_t)M * d * sizeof(float)));
    {
        const int ks = il == IL_CONV2D6 ? 5 : 3;
        GemmArgs a{};
        a.W = e->conv2_w; a.bias = e->conv2_b; a.C = e->x2.as<float>();
        a.M = nseq * Tc * Fc; a.N = d; a.K = ks * ks * d; a.ldc = d; a.act = ACT_RELU; a.alpha = 1.f;
        a.T1 = T1; a.F1 = F1; a.T2 = Tc; a.F2 = Fc; a.Cc = d; a.Tin = T;
        // tiles of padded frames only: not computed (conv2d8: on the last conv only -- the padding of its input is read).  Only the
        // Squeezeformer passes skip_lens today, always conv2d: the conv2d6 / conv2d8 cases are kept exact but are not reached
        if (skip_lens && il != IL_CONV2D8) { a.lens = skip_lens; a.skip_rps = Tc * Fc; a.skip_div = Fc; }
        CHK(subsampling_conv(e, s, a, il == IL_CONV2D6 ? A_CONV5 : A_CONV2, nseq, feats, nullptr));
    }
    if (il == IL_CONV2D8) {     // third conv: 3x3 stride 2 over the second one's output [nseq, Tc, 19, d]
        CHK(e->x3.ensure((size_t)M * F2 * d * sizeof(float)));
        GemmArgs a{};
        a.W = e->conv3_w; a.bias = e->conv3_b; a.C = e->x3.as<float>();
        a.M = M * F2; a.N = d; a.K = 9 * d; a.ldc = d; a.act = ACT_RELU; a.alpha = 1.f;
        a.T1 = Tc; a.F1 = Fc; a.T2 = Tq; a.F2 = F2; a.Cc = d;
        if (skip_lens) { a.lens = skip_lens; a.skip_rps = Tq * F2; a.skip_div = F2; }
        CHK(subsampling_conv(e, s, a, A_CONV2, nseq, nullptr, e->x2.as<float>()));
    }
    const float* const xs = il == IL_CONV2D8 ? e->x3.as<float>() : e->x2.as<float>();
    {   // Conformer: (W.x + b) * sqrt(d)  (embedding.py:97);  Squeezeformer: W.(x * sqrt(d)) + b  (subsampling.py:72-75)
        GemmArgs a{};
        a.A = xs; a.lda = F2 * d; a.W = e->embed_w; a.bias = e->embed_b; a.C = e->x.as<float>(); a.ldc = d;
        // (no_pos: NoPositionalEncoding returns x as it is -- no xscale, embedding.py:104-117)
        a.M = M; a.N = d; a.K = F2 * d; a.act = ACT_NONE; a.alpha = e->pos_enc == POS_ENC_NONE ? 1.f : sqrtf((float)d);
        a.bias_after_alpha = e->cfg.model_kind == 1 ? 1 : 0;
        if (skip_lens) { a.lens = skip_lens; a.skip_rps = Tq; a.skip_div = 1; }
        ProfScope ps(e, s, PROF_GEMM, 2.0 * M * (double)d * F2 * d);
        const int tiles = ((M + 63) / 64) * ((d + 63) / 64);
        const long wide = (long)((M + 63) / 64) * ((d + 127) / 128);      // 64x128 tiles of the unsplit launch
        const long t128 = (long)((M + 127) / 128) * ((d + 127) / 128);
        if (knobs().bf16x3 && tiles >= 128 && launch_gemm_bf16x3(a, A_PLAIN, s)) {
            // exploratory split-bf16 mode: 5x less matrix-pipe time, no K split needed
        } else if (knobs().embed_split && tiles >= 128 && t128 >= 100 && t128 <= 128) {
            // B = 32 x 10 s: 124 tiles of 128x128 -- four K quarters on 8-wave workgroups = 496 workgroups, two per CU, four
            // waves per SIMD: 163 + 11 us (GEMM + reduction) against 180 + 9 us for two K halves on 64x128 tiles and 203 us unsplit
            // (full-width 64-row blocks with the weights packed at first use, the same K quarters: 124 x 4 = 496 workgroups, key 42)
            if (knobs().embed_rows && d == 256 && (F2 * d) % 32 == 0 && !(a.Wp = packed_conv2_rows_of(e, e->embed_w, a.N, a.K, s))) return 1;
            CHK(e->ffpart.ensure((size_t)4 * M * d * sizeof(float)));
            launch_gemm_splitk(a, e->ffpart.as<float>(), 4, s);
        } else if (knobs().embed_split && tiles >= 128 && wide >= 200 && wide <= 320) {
            // about one 4-wave workgroup per CU: two K halves put two waves on every SIMD
            CHK(e->ffpart.ensure((size_t)2 * M * d * sizeof(float)));
            launch_gemm_splitk(a, e->ffpart.as<float>(), 2, s);
        } else if (tiles < 128) {              // few rows, K = 4864: split K so that ~256 workgroups share the weight stream
            const int nsplit = std::min(F2 * d / 32, std::max(2, 256 / tiles));
            CHK(e->ffpart.ensure((size_t)nsplit * M * d * sizeof(float)));
            launch_gemm_splitk(a, e->ffpart.as<float>(), nsplit, s);
        } else {
            launch_gemm(a, A_PLAIN, EPI_STD, s);
        }
    }
    *Tq_out = Tq;
    return 0;
}

int ensure_layer_ws(masr_engine* e, int nseq, int Tq) {
    const int d = e->cfg.d_model, pad = e->cfg.cnn_kernel - 1;
    const size_t M = (size_t)nseq * Tq;
    CHK(e->ln.ensure(M * d * sizeof(float)));
    CHK(e->qkv.ensure(M * 3 * d * sizeof(float)));
    CHK(e->att.ensure(M * d * sizeof(float)));
    CHK(e->lnpad.ensure((size_t)nseq * (Tq + pad) * d * sizeof(float)));
    CHK(e->glu.ensure((size_t)nseq * (Tq + pad) * d * sizeof(float)));
    CHK(e->dwo.ensure(M * d * sizeof(float)));
    return 0;
}

// conv module on x (in place residual).
//  offline  (hist == false): LayerNorm + zero history rows + pad masking are fused into the pointwise_conv1
//                            GEMM's A-tile prologue (rowgemm PRO_LN_PAD); lnpad is not used.
//  streaming (hist == true): lnpad rows [0,pad) of every sequence already hold the cnn cache; LayerNorm writes
//                            the new rows behind them (needed for the next cache) and the GEMM reads lnpad.
int conv_module(masr_engine* e, hipStream_t s, const LayerW& w, const EncodeCtx& c, bool hist, int K, int mstride,
                bool pw1_done, bool pw2_later) {
    if (K <= 0) K = e->cfg.cnn_kernel;
    const int d = e->cfg.d_model, pad = K - 1;
    const int M = c.nseq * c.Tq, Mp = c.nseq * (c.Tq + pad);
    float* x = e->x.as<float>();
    if (pw1_done) {
        // glu buffer already filled by mhsa_out_pw1 (fused out-projection -> LayerNorm -> pointwise_conv1 -> GLU)
    } else if (hist) {
        launch_layernorm(x, w.ln_conv_w, w.ln_conv_b, e->lnpad.as<float>(), M, 1e-5f, c.Tq, pad, c.lens, s);
        rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_GLU,
                rg_args(e->lnpad.as<float>(), d, w.pw1_w, w.pw1_b, e->glu.as<float>(), d, Mp, 2 * d));
    } else {
        // only the real rows go through the GEMM (M = nseq*Tq: 248 workgroups at B=32 x 10 s, one per CU); they land in the
        // padded layout, whose history rows are the constant glu(bias) that the depthwise kernel substitutes itself
        // (non-causal build, streaming: False: the depthwise Conv1d pads the GLU output with (K-1)/2 zero rows on both sides --
        //  those rows of the glu buffer are zeroed once per call by the caller)
        {
            RowGemmArgs g = rg_args(x, d, w.pw1_w, w.pw1_b, e->glu.as<float>(), d, M, 2 * d);
            g.lnw = w.ln_conv_w; g.lnb = w.ln_conv_b; g.lens = c.lens; g.seq_t = c.Tq; g.mstride = mstride; g.out_seq_t = c.Tq;
            g.out_pad_l = e->cfg.causal ? pad : pad / 2; g.out_pad_tot = pad;
            rowgemm(e, s, RG_PRO_LN_PAD, RG_EPI_GLU, g);
        }
    }
    if (pw2_later) return 0;       // the rest of the module is the head stage of the FFN launch that follows
    const float* gconst = (hist || !e->cfg.causal) ? nullptr : w.gconst;
    {
        // few row blocks: depthwise conv + LayerNorm + SiLU as the prologue of the K-split pointwise_conv2 launch (the chunk
        // steps' kernel; the unmaterialised history rows of the offline causal build are substituted there too)
        RowGemmArgs a{};
        a.A = e->glu.as<float>(); a.lda = d; a.lnw = w.cln_w; a.lnb = w.cln_b; a.dw_w = w.dw_w; a.dw_b = w.dw_b; a.gconst = gconst;
        a.W = w.pw2_w; a.bias = w.pw2_b; a.C = x; a.ldc = d; a.R = x; a.ldr = d; a.M = M; a.N = d; a.alpha = 1.f; a.eps = 1e-5f;
        a.mstride = mstride; a.seq_t = c.Tq; a.pad = pad; a.lens = c.lens; a.mask_tp = c.lens ? c.Tq : 0;
        ProfScope ps(e, s, PROF_GEMM, 2.0 * M * (double)d * d);
        if (!e->conv_bn && knobs().few_rows_path && launch_rowgemm(a, RG_PRO_DWCONV, RG_EPI_RESID, s)) return 0;
    }
    if (e->conv_bn)        // BatchNorm build: the depthwise kernel's BN variant (the Squeezeformer's), then pointwise_conv2
        DWCHK(launch_dwconv_bn_silu(e->glu.as<float>(), w.dw_w, w.dw_b, w.cln_w, w.cln_b, e->dwo.as<float>(), c.nseq, c.Tq, K, s, gconst), K);
    else
        DWCHK(launch_dwconv_ln_silu(e->glu.as<float>(), w.dw_w, w.dw_b, w.cln_w, w.cln_b, e->dwo.as<float>(), c.nseq, c.Tq, K,
                                    1e-5f, s, gconst), K);
    resid_gemm(e, s, e->dwo.as<float>(), w.pw2_w, w.pw2_b, x, M, c.lens, c.lens ? c.Tq : 0, mstride);
    return 0;
}

// Streaming conv module of the Conformer family (LayerNorm conv norm), two launches on the small-M kernel:
//   [cnn cache | LayerNorm(new rows)] -> pointwise_conv1 + GLU        (+ the new cache)          (rowgemm_small PRO_HIST)
//   causal depthwise conv + LayerNorm + SiLU -> pointwise_conv2 + residual                       (rowgemm_small PRO_DWCONV)
// (convolution.py:98-131).  Where the small-M kernel does not apply (>= 2048 rows, frames per chunk not a multiple of 4) the
// same steps run as separate launches: conv_hist, pointwise_conv1, dwconv_ln_silu, pointwise_conv2.
int conv_module_stream(masr_engine* e, hipStream_t s, const LayerW& w, int n, int Tq, float* const* cache_rd,
                       float* const* cache_wr, int K, bool pw2_later) {
    const int d = e->cfg.d_model, pad = K - 1, M = n * Tq, Mp = n * (Tq + pad);
    float* x = e->x.as<float>();
    {
        RowGemmArgs a{};
        a.A = x; a.lda = d; a.lnw = w.ln_conv_w; a.lnb = w.ln_conv_b; a.W = w.pw1_w; a.bias = w.pw1_b;
        a.C = e->glu.as<float>(); a.ldc = d; a.M = Mp; a.N = 2 * d; a.alpha = 1.f; a.eps = 1e-5f; a.mstride = 4;
        a.seq_t = Tq; a.pad = pad; a.cache_rd = cache_rd; a.cache_wr = cache_wr;
        ProfScope ps(e, s, PROF_GEMM, 2.0 * Mp * (double)(2 * d) * d);
        if (!launch_rowgemm(a, RG_PRO_HIST, RG_EPI_GLU, s)) {
            launch_conv_hist(x, w.ln_conv_w, w.ln_conv_b, cache_rd, cache_wr, e->lnpad.as<float>(), n, Tq, pad, 0, 1e-5f, s);
            a.A = e->lnpad.as<float>();
            launch_rowgemm(a, RG_PRO_PLAIN, RG_EPI_GLU, s);
        }
    }
    if (pw2_later) return 0;       // depthwise conv ... pointwise_conv2: head stage of the FFN launch that follows
    {
        RowGemmArgs a{};
        a.A = e->glu.as<float>(); a.lda = d; a.lnw = w.cln_w; a.lnb = w.cln_b; a.dw_w = w.dw_w; a.dw_b = w.dw_b;
        a.W = w.pw2_w; a.bias = w.pw2_b; a.C = x; a.ldc = d; a.R = x; a.ldr = d; a.M = M; a.N = d; a.alpha = 1.f;
        a.eps = 1e-5f; a.mstride = 4; a.seq_t = Tq; a.pad = pad;
        ProfScope ps(e, s, PROF_GEMM, 2.0 * M * (double)d * d);
        // (BatchNorm build: the small-M kernel's depthwise prologue carries the LayerNorm variant only -- the depthwise kernel's BN
        //  variant, then pointwise_conv2 on the small-M kernel)
        if (e->conv_bn || !launch_rowgemm(a, RG_PRO_DWCONV, RG_EPI_RESID, s)) {
            if (e->conv_bn)
                DWCHK(launch_dwconv_bn_silu(e->glu.as<float>(), w.dw_w, w.dw_b, w.cln_w, w.cln_b, e->dwo.as<float>(), n, Tq, K, s, nullptr), K);
            else
                DWCHK(launch_dwconv_ln_silu(e->glu.as<float>(), w.dw_w, w.dw_b, w.cln_w, w.cln_b, e->dwo.as<float>(), n, Tq, K, 1e-5f, s,
                                            nullptr), K);
            a.A = e->dwo.as<float>();
            launch_rowgemm(a, RG_PRO_PLAIN, RG_EPI_RESID, s);
        }
    }
    return 0;
}

// multi-head self-attention block on x (in place residual); seqs describe where K/V live
// kv_seqs (streaming): the k | v columns are appended to the streams' caches by the projection itself
void qkv_proj(masr_engine* e, hipStream_t s, int pro, const float* lnw, const float* lnb, const float* wqkv, const float* bqkv, int M,
              const AttSeq* kv_seqs, int kv_tq) {
    const int d = e->cfg.d_model;
    RowGemmArgs g = rg_args(e->x.as<float>(), d, wqkv, bqkv, e->qkv.as<float>(), 3 * d, M, 3 * d);
    g.lnw = lnw; g.lnb = lnb; g.kv_seqs = kv_seqs; g.kv_tq = kv_tq;
    rowgemm(e, s, pro, RG_EPI_STORE, g);
}
void mhsa(masr_engine* e, hipStream_t s, const LayerW& w, int M, const AttSeq* kv_seqs, int kv_tq) {
    qkv_proj(e, s, RG_PRO_LN, w.ln_mha_w, w.ln_mha_b, w.wqkv, w.bqkv, M, kv_seqs, kv_tq);
}
void mhsa_out(masr_engine* e, hipStream_t s, const LayerW& w, int M) {
    resid_gemm(e, s, e->att.as<float>(), w.wo, w.bo, e->x.as<float>(), M);
}

// offline conformer layer: attention out-projection + residual and the conv module's LayerNorm + pointwise_conv1 + GLU in ONE
// kernel (rowgemm EPI_CHAIN): the updated rows go to x (global) and, without leaving the CU, through the second GEMM
// K: the layer's depthwise kernel size (Efficient Conformer: 15 before, 7 behind the stride layer); att / a_seq_t / a_seq_stride: the
// attention output when it lives in a per-sequence padded buffer (grouped attention's planes)
void mhsa_out_pw1(masr_engine* e, hipStream_t s, const LayerW& w, const EncodeCtx& c, int mstride, int K,
                  const float* att, int a_seq_t, int a_seq_stride) {
    const int d = e->cfg.d_model, pad = (K > 0 ? K : e->cfg.cnn_kernel) - 1, M = c.nseq * c.Tq;
    float* x = e->x.as<float>();
    RowGemmArgs a{};
    a.A = att ? att : e->att.as<float>(); a.lda = d; a.a_seq_t = a_seq_t; a.a_seq_stride = a_seq_stride; a.lnw = w.ln_conv_w; a.lnb = w.ln_conv_b; a.W = w.chain_w; a.bias = w.chain_b;
    a.C = e->glu.as<float>(); a.ldc = d; a.M = M; a.N = 3 * d; a.R = x; a.R2 = x; a.ldr = d; a.alpha = 1.f;
    a.lens = c.lens; a.seq_t = c.Tq; a.mstride = mstride; a.eps = 1e-5f;
    a.out_seq_t = c.Tq; a.out_pad_l = e->cfg.causal ? pad : pad / 2; a.out_pad_tot = pad;
    if (knobs().rowgemm_packed) a.Wp = packed_rows_of(e, w.chain_w, 3 * d, s);
    ProfScope ps(e, s, PROF_GEMM, 2.0 * M * (double)(3 * d) * d);
    launch_rowgemm(a, RG_PRO_PLAIN, RG_EPI_CHAIN, s);
}

// ---- finalize: what the Conformer families and the Squeezeformer upload alike ---------------------------------------------------
// One subsampling conv [co,ci,ks,ks] -> [co][ci / 32][kh*ks+kw][ci % 32]: the implicit GEMM walks the ks^2 window positions of
// one 32-channel block in consecutive K slabs, so the overlapping input columns of neighbouring positions (kw = 2 of one output,
// kw = 0 of the next) are re-read a slab or two later -- out of L1 / L2 instead of HBM
static int upload_conv_kxk(masr_engine* e, const std::string& name, int d, int ks, float** wd, float** bd) {
    const int kk = ks * ks;
    const HostTensor* t;
    CHK(get(e, name + ".weight", {d, d, ks, ks}, &t));
    std::vector<float> w((size_t)d * kk * d);
    for (int co = 0; co < d; ++co)
        for (int ci = 0; ci < d; ++ci)
            for (int k = 0; k < kk; ++k)
                w[(size_t)co * kk * d + (size_t)(ci / 32) * kk * 32 + k * 32 + ci % 32] = t->v[((size_t)co * d + ci) * kk + k];
    CHK(upload(e, w, wd));
    return up(e, name + ".bias", {d}, bd);
}

// global CMVN, conv1 [d,1,3,3] -> [9][d], conv2 of ks x ks (3, or 5 for conv2d6) and, c3 given, the third conv of conv2d8;
// d channels (0: output_size; DeepSpeech2: 32)
int upload_conv_frontend(masr_engine* e, const std::string& c1, const std::string& c2, int ks, const char* c3, int d) {
    const int F = e->cfg.n_mels;
    if (d <= 0) d = e->cfg.d_model;
    const HostTensor* t;
    CHK(up(e, "encoder.global_cmvn.mean", {F}, &e->cmvn_mean));
    CHK(up(e, "encoder.global_cmvn.istd", {F}, &e->cmvn_istd));
    CHK(get(e, c1 + ".weight", {d, 1, 3, 3}, &t));
    std::vector<float> w(9 * d);
    for (int c = 0; c < d; ++c)
        for (int k = 0; k < 9; ++k) w[k * d + c] = t->v[c * 9 + k];
    CHK(upload(e, w, &e->conv1_w));
    CHK(up(e, c1 + ".bias", {d}, &e->conv1_b));
    CHK(upload_conv_kxk(e, c2, d, ks, &e->conv2_w, &e->conv2_b));
    if (c3) CHK(upload_conv_kxk(e, c3, d, 3, &e->conv3_w, &e->conv3_b));
    return 0;
}

// the projection behind the convs [d][c*F2+f] -> [d][f*d + c]   (subsampling.py:110, 151, 206 flatten channel-major)
int upload_embed_proj(masr_engine* e, const std::string& proj, int F2) {
    const int d = e->cfg.d_model;
    const HostTensor* t;
    CHK(get(e, proj + ".weight", {d, (int64_t)d * F2}, &t));
    std::vector<float> w((size_t)d * d * F2);
    for (int o = 0; o < d; ++o)
        for (int c = 0; c < d; ++c)
            for (int f = 0; f < F2; ++f) w[(size_t)o * d * F2 + f * d + c] = t->v[(size_t)o * d * F2 + c * F2 + f];
    CHK(upload(e, w, &e->embed_w));
    return up(e, proj + ".bias", {d}, &e->embed_b);
}

// positional table (conformer/embedding.py:31-37), or the one the caller loaded as __pos_table__
int upload_pos_table(masr_engine* e) {
    const int d = e->cfg.d_model;
    auto it = e->host.find("__pos_table__");
    if (it != e->host.end()) {
        if ((int64_t)it->second.v.size() != (int64_t)e->cfg.max_pos * d) return fail("__pos_table__ has wrong size");
        return upload(e, it->second.v, &e->pe);
    }
    std::vector<float> pe((size_t)e->cfg.max_pos * d);
    for (int i = 0; i < d; i += 2) {
        const float div = expf((float)i * (float)(-(log(10000.0) / d)));
        for (int p = 0; p < e->cfg.max_pos; ++p) {
            pe[(size_t)p * d + i] = sinf((float)p * div);
            pe[(size_t)p * d + i + 1] = cosf((float)p * div);
        }
    }
    return upload(e, pe, &e->pe);
}

// the eval-mode BatchNorm1d of the layer's conv module: weight, bias, running_mean, running_var (the folds differ by family)
int get_conv_bn(masr_engine* e, const std::string& p, const HostTensor* bn[4]) {
    const char* nm[4] = {"weight", "bias", "running_mean", "running_var"};
    for (int j = 0; j < 4; ++j) CHK(get(e, p + "conv_module.norm." + nm[j], {e->cfg.d_model}, &bn[j]));
    return 0;
}

// fused QKV projection [3d, d] of the layer under key prefix p
int upload_qkv(masr_engine* e, const std::string& p, float** wqkv, float** bqkv) {
    const int d = e->cfg.d_model;
    const HostTensor* t;
    std::vector<float> wq((size_t)3 * d * d), bq(3 * d);
    const char* nm[3] = {"linear_q", "linear_k", "linear_v"};
    for (int j = 0; j < 3; ++j) {
        CHK(get(e, p + "self_attn." + nm[j] + ".weight", {d, d}, &t));
        memcpy(&wq[(size_t)j * d * d], t->v.data(), sizeof(float) * d * d);
        CHK(get(e, p + "self_attn." + nm[j] + ".bias", {d}, &t));
        memcpy(&bq[j * d], t->v.data(), sizeof(float) * d);
    }
    CHK(upload(e, wq, wqkv));
    return upload(e, bq, bqkv);
}

// depthwise [d,1,K] -> [K][d]
int upload_depthwise(masr_engine* e, const std::string& p, int K, float** dw_w, float** dw_b) {
    const int d = e->cfg.d_model;
    const HostTensor* t;
    CHK(get(e, p + "conv_module.depthwise_conv.weight", {d, 1, K}, &t));
    std::vector<float> wd((size_t)K * d);
    for (int c = 0; c < d; ++c)
        for (int j = 0; j < K; ++j) wd[(size_t)j * d + c] = t->v[(size_t)c * K + j];
    CHK(upload(e, wd, dw_w));
    return up(e, p + "conv_module.depthwise_conv.bias", {d}, dw_b);
}

// positional keys p_j = W_pos * PE(j) for every position, once (attention.py:229-231), on the caller's stream
int build_ptab(masr_engine* e, hipStream_t s, const float* wpos, float** ptab) {
    const int d = e->cfg.d_model;
    void* pt = nullptr;
    HIPCHK(hipMalloc(&pt, (size_t)e->cfg.max_pos * d * sizeof(float)));
    e->owned.push_back(pt);
    *ptab = (float*)pt;
    gemm(e, s, e->pe, d, wpos, nullptr, *ptab, d, e->cfg.max_pos, d, d, ACT_NONE, 1.f, nullptr, 0, PROF_NONE);
    return 0;
}

// glu(bias): what the zero left-padding of the causal conv turns into behind pointwise_conv1 + GLU (wide: the kernel of wide.hip)
int upload_gconst(masr_engine* e, hipStream_t s, const float* pw1_b, bool wide, float** gconst) {
    const int d = e->cfg.d_model;
    std::vector<float> z(d, 0.f);
    CHK(upload(e, z, gconst));
    if (wide) launch_glu_const_wide(pw1_b, *gconst, d, s);
    else launch_glu_const(pw1_b, *gconst, s);
    return 0;
}

ChunkWindow chunk_window(const Stream& st, int T0) {
    ChunkWindow w;
    w.cache_t1 = st.cache_t1;
    w.first_full = st.offset - st.cache_t1;
    const int key_size = st.cache_t1 + T0;
    w.ncs = st.history < 0 ? 0 : st.history == 0 ? key_size : std::max(key_size - st.history, 0);
    w.next_cache_t1 = key_size - w.ncs;
    return w;
}
// half-rate layers: the reference stores their cache repeat-interleaved at the input rate and reads every second entry back, so a
// step sees `want` entries starting at first_half; they must be exactly the entries appended since (true for chunks of an even
// number of frames; the reference itself fails or drops the newest entry otherwise)
int half_rate_window(const Stream& st, int want, int* first, int* count) {
    const int avail = st.offset_r - st.first_half;
    if (want != avail)
        return fail("bounded attention history: the half-rate cache window is not contiguous with the new frames (odd chunk lengths "
                    "with required_cache_size >= 0 are not supported)");
    *first = st.first_half;
    *count = avail;
    return 0;
}

// ---- the tables and the tail the chunk steps of the families share --------------------------------------------------------
// The attention descriptor of one stream in one layer whose cache holds interleaved k | v rows of 2 d floats: Tl new queries at q
// attend over the ncached rows from cache row `first` on and over themselves.
AttSeq interleaved_seq(const float* q, float* cache, int d, int first, int ncached, int Tl, float* out, int pos0, int q_abs0) {
    AttSeq a;
    a.q = q;
    a.k = cache + (size_t)first * 2 * d;
    a.v = a.k + d;
    a.out = out;
    a.nq = Tl;
    a.nk = ncached + Tl;           // (the new rows are appended at k + (nk - nq) rows: the cache row of the first new frame)
    a.klen = a.nk;
    a.pos0 = pos0;
    a.q_abs0 = q_abs0;
    a.pad_ = 0;
    return a;
}

// [read | written]: per (layer, stream) the base of the layer's rows in the stream's cnn cache, then the same in its second half
std::vector<float*> cnn_cache_table(const std::vector<Stream*>& st, int L, size_t layer_floats) {
    const size_t n = st.size();
    std::vector<float*> hp(n * L * 2);
    for (int l = 0; l < L; ++l)
        for (size_t i = 0; i < n; ++i) {
            hp[(size_t)l * n + i] = st[i]->cnn.as<float>() + (size_t)l * layer_floats;
            hp[(size_t)(L + l) * n + i] = st[i]->cnn2.as<float>() + (size_t)l * layer_floats;     // written half of the double buffer
        }
    return hp;
}

// The step's tables to the device through the pinned staging area, in one go: the descriptors to e->attseq, the cnn cache pointers to
// e->cnnptrs and, where a step has one, a third table (the PlaneCopy rows, the abs_pos offsets) to third_dev.
int upload_chunk_tables(masr_engine* e, hipStream_t s, const std::vector<AttSeq>& hs, const std::vector<float*>& hp,
                               void* third_dev, const void* third, size_t third_bytes) {
    CHK(e->stage.begin(sizeof(AttSeq) * hs.size() + sizeof(float*) * hp.size() + third_bytes + 64));
    CHK(e->stage.push(e->attseq.p, hs.data(), sizeof(AttSeq) * hs.size(), s));
    CHK(e->stage.push(e->cnnptrs.p, hp.data(), sizeof(float*) * hp.size(), s));
    if (third_bytes) CHK(e->stage.push(third_dev, third, third_bytes, s));
    CHK(e->stage.end(s));
    return 0;
}

// behind a step of T0 input-rate frames (Tr at the half rate) of the Squeezeformer or the Efficient Conformer
void advance_half_rate(std::vector<Stream*>& st, const std::vector<ChunkWindow>& win, int T0, int Tr) {
    for (size_t i = 0; i < st.size(); ++i) {
        st[i]->offset += T0;
        st[i]->offset_r += Tr;
        st[i]->cache_t1 = win[i].next_cache_t1;
        st[i]->first_half += win[i].ncs / 2;
        std::swap(st[i]->cnn, st[i]->cnn2);
    }
}


}  // namespace masr
