// libmasr_hip.so -- engine, DeepSpeech2 (model_kind 3): weights, forward and chunk step.  Host code only (file map: engine_state.h).
#include "engine_encoder.h"

namespace masr {

// reference: masr/model_utils/deepspeech2/{model.py:64-108, encoder.py:36-129, conv.py:5-22}
int finalize_ds2(masr_engine* e) {
    const int H = e->cfg.d_model, L = e->cfg.num_blocks, ndir = e->cfg.causal ? 1 : 2, V = e->cfg.vocab_size;
    const int F = e->cfg.n_mels, F1 = (F - 1) / 2, F2 = (F1 - 1) / 2, C = 32, D = H * ndir;
    // Conv2dSubsampling4Pure: 32 channels, so the shared [co][ci / 32][k][ci % 32] order is plain [co][k][ci]
    CHK(upload_conv_frontend(e, "encoder.conv.conv.0", "encoder.conv.conv.2", 3, nullptr, C));
    // use_gru: True wraps nn.GRU in the reference's own GRU module (deepspeech2/gru.py): one more ".rnn" in every key
    const bool gru = e->ds2_gru;
    const int G = gru ? 3 : 4;                        // gates per unit: r, z, n  |  i, f, g, o
    const std::string cell = gru ? "rnn.rnn." : "rnn.";
    {
        const bool has_gru = e->host.count("encoder.rnns.0.rnn.rnn.weight_ih_l0") > 0;
        const bool has_lstm = e->host.count("encoder.rnns.0.rnn.weight_ih_l0") > 0;
        if (gru && !has_gru && has_lstm)
            return fail("deepspeech2: encoder_conf.use_gru is True but the checkpoint holds LSTM layers (encoder.rnns.0.rnn.weight_ih_l0)");
        if (!gru && has_gru)
            return fail("deepspeech2: encoder_conf.use_gru is False but the checkpoint holds GRU layers (encoder.rnns.0.rnn.rnn.weight_ih_l0)");
    }
    e->ds2_layers.assign(L, Ds2LayerW{});
    for (int i = 0; i < L; ++i) {
        Ds2LayerW& w = e->ds2_layers[i];
        const std::string p = "encoder.rnns." + std::to_string(i) + ".";
        const int kin = i == 0 ? C * F2 : D;
        w.kin = kin;
        std::vector<float> wih((size_t)ndir * G * H * kin), bih((size_t)ndir * G * H), whh((size_t)ndir * G * H * H);
        std::vector<float> bhn(gru ? (size_t)ndir * H : 0);
        for (int dir = 0; dir < ndir; ++dir) {
            const std::string suf = dir ? "_reverse" : "";
            const HostTensor *a, *b, *c, *d;
            CHK(get(e, p + cell + "weight_ih_l0" + suf, {G * H, kin}, &a));
            CHK(get(e, p + cell + "weight_hh_l0" + suf, {G * H, H}, &b));
            CHK(get(e, p + cell + "bias_ih_l0" + suf, {G * H}, &c));
            CHK(get(e, p + cell + "bias_hh_l0" + suf, {G * H}, &d));
            float* dst = wih.data() + (size_t)dir * G * H * kin;
            if (i == 0) {   // conv output is channels-last here: column f*32 + c  <-  reference column c*F2 + f (conv.py:20)
                for (int r = 0; r < G * H; ++r)
                    for (int c2 = 0; c2 < C; ++c2)
                        for (int f = 0; f < F2; ++f) dst[(size_t)r * kin + f * C + c2] = a->v[(size_t)r * kin + c2 * F2 + f];
            } else {
                std::copy(a->v.begin(), a->v.end(), dst);
            }
            std::copy(b->v.begin(), b->v.end(), whh.begin() + (size_t)dir * G * H * H);
            // GRU: b_hr and b_hz fold into the input projection, b_hn stays with the recurrent product (r * (W_hn h + b_hn))
            for (int r = 0; r < G * H; ++r) bih[(size_t)dir * G * H + r] = c->v[r] + (gru && r >= 2 * H ? 0.f : d->v[r]);
            if (gru) std::copy(d->v.begin() + 2 * H, d->v.end(), bhn.begin() + (size_t)dir * H);
        }
        CHK(upload(e, wih, &w.wih));
        CHK(upload(e, bih, &w.bih));
        CHK(upload(e, whh, &w.whh));
        if (gru) CHK(upload(e, bhn, &w.bhn));
        CHK(up_wb(e, p + "layer_norm", {D}, &w.ln_w, &w.ln_b));
    }
    CHK(up_wb(e, "decoder.ctc_lo", {V, D}, &e->ctc_w, &e->ctc_b));
    return 0;
}

// feats [nseq, T, 80] -> enc_out [nseq*Tq, D].  lens: device feature lengths (full utterances) or nullptr (chunks:
// every row is valid, inference_predictor.py:70).  st: per-sequence streams carrying (h, c) of every layer, or nullptr.
int ds2_forward(masr_engine* e, hipStream_t s, const float* feats, const int* lens, int nseq, int T, float* enc_out,
                       Stream** st, int* Tq_out) {
    const int H = e->cfg.d_model, L = e->cfg.num_blocks, ndir = e->cfg.causal ? 1 : 2, D = H * ndir, C = 32;
    const int F = e->cfg.n_mels, F1 = (F - 1) / 2, F2 = (F1 - 1) / 2;
    const int T1 = (T - 1) / 2, Tq = (T1 - 1) / 2;
    if (T < 7 || Tq <= 0) return fail("input too short for Conv2dSubsampling4Pure (need >= 7 frames)");
    if (st && ndir != 1) return fail("deepspeech2: stateful chunks need the uni-directional (streaming) model");
    const int M = nseq * Tq;
    const bool gru = e->ds2_gru;
    const int G = gru ? 3 : 4;                        // gates per unit
    CHK(e->x1.ensure((size_t)nseq * T1 * F1 * C * sizeof(float)));
    CHK(e->x2.ensure((size_t)M * F2 * C * sizeof(float)));
    CHK(e->gx.ensure((size_t)M * ndir * G * H * sizeof(float)));
    CHK(e->rnn_out.ensure((size_t)M * D * sizeof(float)));
    CHK(e->ln.ensure((size_t)M * D * sizeof(float)));
    CHK(e->hstate.ensure((size_t)2 * ndir * nseq * H * sizeof(float)));
    CHK(e->cstate.ensure((size_t)ndir * nseq * H * sizeof(float)));
    const int* xl = nullptr;
    if (lens) {
        CHK(e->ds2_lens.ensure(sizeof(int) * nseq));
        launch_ds2_lens(lens, nseq, Tq, e->ds2_lens.as<int>(), s);
        xl = e->ds2_lens.as<int>();
    }
    launch_conv1(feats, e->cmvn_mean, e->cmvn_istd, e->conv1_w, e->conv1_b, e->x1.as<float>(), nseq, T, F, C, s);
    {
        GemmArgs a{};
        a.A = e->x1.as<float>(); a.W = e->conv2_w; a.bias = e->conv2_b; a.C = e->x2.as<float>();
        a.M = M * F2; a.N = C; a.K = 9 * C; a.ldc = C; a.act = ACT_RELU; a.alpha = 1.f;
        a.T1 = T1; a.F1 = F1; a.T2 = Tq; a.F2 = F2; a.Cc = C;
        ProfScope ps(e, s, PROF_CONV2, 2.0 * a.M * (double)a.N * a.K);
        launch_gemm(a, A_CONV2, EPI_STD, s);
    }
    const float* in = e->x2.as<float>();
    const size_t hsz = (size_t)ndir * nseq * H;
    float* hbuf = e->hstate.as<float>();
    float* cbuf = e->cstate.as<float>();
    for (int l = 0; l < L; ++l) {
        const Ds2LayerW& w = e->ds2_layers[l];
        gemm(e, s, in, w.kin, w.wih, w.bih, e->gx.as<float>(), ndir * G * H, M, ndir * G * H, w.kin, ACT_NONE, 1.f, nullptr, 0);
        if (st) {
            for (int i = 0; i < nseq; ++i) {
                const float* hc = st[i]->cnn.as<float>() + (size_t)l * 2 * H;
                HIPCHK(hipMemcpyAsync(hbuf + (size_t)i * H, hc, sizeof(float) * H, hipMemcpyDeviceToDevice, s));
                if (!gru) HIPCHK(hipMemcpyAsync(cbuf + (size_t)i * H, hc + H, sizeof(float) * H, hipMemcpyDeviceToDevice, s));
            }
        } else {
            HIPCHK(hipMemsetAsync(hbuf, 0, sizeof(float) * hsz, s));
            if (!gru) HIPCHK(hipMemsetAsync(cbuf, 0, sizeof(float) * hsz, s));
        }
        // (the whole sequence of a layer as one cooperative launch with W_hh resident in registers and a barrier in global memory
        //  per step was built and measured in round 6: 10.0 against 6.0 ms at B = 1, 26.4 against 25.7 ms at B = 32 --
        //  tools/studies/lstm_seq_study.hip)
        {   // PROF_RNN times exactly the Tq step launches of this layer
            ProfScope ps(e, s, PROF_RNN, 2.0 * nseq * (double)Tq * ndir * G * H * H);    // the step loop of one layer (Tq launches)
            for (int step = 0; step < Tq; ++step) {
                const float* hp = hbuf + (size_t)(step & 1) * hsz;
                float* hn = hbuf + (size_t)((step + 1) & 1) * hsz;
                const int miss = gru ? launch_gru_step(e->gx.as<float>(), w.whh, w.bhn, hp, hn, e->rnn_out.as<float>(), xl, nseq, Tq, H, step, ndir, s)
                                     : launch_lstm_step(e->gx.as<float>(), w.whh, hp, hn, cbuf, e->rnn_out.as<float>(), xl, nseq, Tq, H, step, ndir, s);
                if (miss) return fail("deepspeech2: no recurrent step kernel for rnn_size=" + std::to_string(H));
            }
        }
        if (st) {     // GRU: the reference returns final_state_c = final_state_h (gru.py), so h goes to both slots
            const float* hfin = hbuf + (size_t)(Tq & 1) * hsz;
            for (int i = 0; i < nseq; ++i) {
                float* hc = st[i]->cnn.as<float>() + (size_t)l * 2 * H;
                HIPCHK(hipMemcpyAsync(hc, hfin + (size_t)i * H, sizeof(float) * H, hipMemcpyDeviceToDevice, s));
                HIPCHK(hipMemcpyAsync(hc + H, (gru ? hfin : cbuf) + (size_t)i * H, sizeof(float) * H, hipMemcpyDeviceToDevice, s));
            }
        }
        float* out = l == L - 1 ? enc_out : e->ln.as<float>();
        launch_layernorm_generic(e->rnn_out.as<float>(), w.ln_w, w.ln_b, out, M, D, 1e-5f, s);
        in = out;
    }
    LAUNCHCHK();
    if (Tq_out) *Tq_out = Tq;
    return 0;
}

// DeepSpeech2 chunk step, n streams in lock-step (deepspeech2/model.py:79-108): chunk conv + LSTM stack with carried (h, c)
int encode_chunk_ds2(masr_engine* e, hipStream_t s, std::vector<Stream*>& st, const float* feats_dev, int Tc,
                            float* probs_dev, int32_t* argmax_dev, float* maxprob_dev, float* enc_out_dev) {
    const int n = (int)st.size();
    int Tq = 0;
    const int Tq3 = ((Tc - 1) / 2 - 1) / 2;
    if (Tq3 <= 0) return fail("chunk too short");
    CHK(e->enc.ensure((size_t)n * Tq3 * enc_dim(e) * sizeof(float)));
    CHK(ds2_forward(e, s, feats_dev, nullptr, n, Tc, e->enc.as<float>(), st.data(), &Tq));
    CHK(chunk_ctc(e, s, e->enc.as<float>(), n * Tq, probs_dev, argmax_dev, maxprob_dev, enc_out_dev));
    for (int i = 0; i < n; ++i) st[i]->offset += Tq;
    return 0;
}

}  // namespace masr
