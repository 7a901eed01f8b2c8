// libmasr_hip.so -- engine, feature front ends (fbank, MFCC, linear spectra), resampling and the offline hot path in one call.  Host code only (file map: engine_state.h).
#include "engine_encoder.h"

using namespace masr;

namespace masr {
// fbank tables (float32 arithmetic mirrors torchaudio's get_mel_banks / povey window); they do not
// depend on the model, so a weight-less engine can already run the feature front-end.
int build_fbank_tables(masr_engine* e) {
    {
        std::vector<float> win(400), tw512(2 * 257), melw((size_t)80 * 257, 0.f);
        std::vector<int> lo(80), hi(80);
        for (int i = 0; i < 400; ++i) {
            const double hann = 0.5 - 0.5 * cos(2.0 * M_PI * i / 399.0);
            win[i] = (float)pow(hann, 0.85);
        }
        for (int k = 0; k <= 256; ++k) {
            tw512[2 * k] = (float)cos(-2.0 * M_PI * k / 512.0);
            tw512[2 * k + 1] = (float)sin(-2.0 * M_PI * k / 512.0);
        }
        const double mel_low = 1127.0 * log(1.0 + 20.0 / 700.0), mel_high = 1127.0 * log(1.0 + 8000.0 / 700.0);
        const float delta = (float)((mel_high - mel_low) / 81.0), mlow = (float)mel_low;
        for (int m = 0; m < 80; ++m) {
            const float left = mlow + (float)m * delta, center = mlow + ((float)m + 1.0f) * delta,
                        right = mlow + ((float)m + 2.0f) * delta;
            lo[m] = 257;
            hi[m] = 0;
            for (int k = 0; k < 256; ++k) {
                const float freq = 31.25f * (float)k;
                const float mel = 1127.0f * logf(1.0f + freq / 700.0f);
                const float upv = (mel - left) / (center - left), down = (right - mel) / (right - center);
                const float wv = fmaxf(0.f, fminf(upv, down));
                melw[(size_t)m * 257 + k] = wv;
                if (wv > 0.f) {
                    lo[m] = std::min(lo[m], k);
                    hi[m] = std::max(hi[m], k + 1);
                }
            }
            if (lo[m] > hi[m]) lo[m] = hi[m] = 0;
        }
        // transposed weights [tap][filter] for the register-FFT kernel (tap i of filter m = bin lo[m] + i, zero past hi[m])
        constexpr int TAPS = 16;
        std::vector<float> melwt((size_t)TAPS * 80, 0.f);
        for (int m = 0; m < 80; ++m) {
            if (hi[m] - lo[m] > TAPS) return fail("fbank tables: a mel filter is wider than 16 bins");
            for (int i = 0; i < hi[m] - lo[m]; ++i) melwt[(size_t)i * 80 + m] = melw[(size_t)m * 257 + lo[m] + i];
        }
        // twiddles of the Stockham radix-4 passes Ns = 4, 16, 64 of the 256-point FFT, one row per lane j:
        // [pass][r - 1][j] = exp(-2 pi i r (j mod Ns) / (4 Ns)), r = 1..3
        std::vector<float> twr4((size_t)3 * 3 * 64 * 2);
        for (int p = 0; p < 3; ++p) {
            const int Ns = p == 0 ? 4 : p == 1 ? 16 : 64;
            for (int r = 1; r <= 3; ++r)
                for (int j = 0; j < 64; ++j) {
                    const double ang = -2.0 * M_PI * (double)(r * (j % Ns)) / (double)(4 * Ns);
                    twr4[(((size_t)p * 3 + (r - 1)) * 64 + j) * 2] = (float)cos(ang);
                    twr4[(((size_t)p * 3 + (r - 1)) * 64 + j) * 2 + 1] = (float)sin(ang);
                }
        }
        CHK(upload(e, win, &e->window));
        CHK(upload(e, tw512, &e->tw512));
        CHK(upload(e, melwt, &e->melwt));
        CHK(upload(e, twr4, &e->twr4));
        CHK(upload(e, lo, &e->mel_lo));

    }
    return 0;
}
}  // namespace masr

extern "C" {

int masr_fbank_batch(masr_engine* e, const void* samples_dev, int32_t sample_format, const int32_t* n_samples_dev,
                     int32_t B, int32_t n_max, int32_t use_db_normalization, float target_db, float* feats_dev,
                     int32_t* n_frames_dev, int16_t* norm_pcm_dev, float* gain_dev, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    if (sample_format != 0 && sample_format != 1) return fail("sample_format must be 0 (int16) or 1 (float32)");
    hipStream_t s = (hipStream_t)stream;
    const int T_max = n_max >= 400 ? 1 + (n_max - 400) / 160 : 0;
    CHK(e->gain.ensure(sizeof(float) * fbank_gain_scratch_floats(B)));
    float* gain = e->gain.as<float>();
    if (use_db_normalization == 2) {      // gains evaluated by the caller (masr_mean_square + the host's numpy, audio.py:287-304)
        if (!gain_dev) return fail("use_db_normalization = 2 needs the gains in gain_dev");
        HIPCHK(hipMemcpyAsync(gain, gain_dev, sizeof(float) * B, hipMemcpyDeviceToDevice, s));
    }
    {
        ProfScope ps(e, s, PROF_FBANK, 0.0);
        launch_fbank(samples_dev, sample_format, n_samples_dev, B, n_max, use_db_normalization, target_db, e->fbank_tables(),
                     feats_dev, T_max, gain, norm_pcm_dev, s);
    }
    if (gain_dev && use_db_normalization == 1)
        HIPCHK(hipMemcpyAsync(gain_dev, gain, sizeof(float) * B, hipMemcpyDeviceToDevice, s));
    if (n_frames_dev) launch_frame_counts(n_samples_dev, B, n_frames_dev, nullptr, 0, s);
    LAUNCHCHK();
    return 0;
}

int masr_mean_square(masr_engine* e, const void* samples_dev, int32_t sample_format, const int32_t* n_samples_dev, int32_t B,
                     int32_t n_max, float* mean_square_dev, void* stream) {
    if (!e || !mean_square_dev) return fail("null argument");
    ENTER(e);
    if (sample_format != 0 && sample_format != 1) return fail("sample_format must be 0 (int16) or 1 (float32)");
    DevBuf& ws = e->ms_ws[stream];
    CHK(ws.ensure(sizeof(float) * fbank_gain_scratch_floats(B)));
    launch_mean_square(samples_dev, sample_format, n_samples_dev, B, n_max, ws.as<float>(), mean_square_dev,
                       (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

// Device form of masr_resample_f32 for the rows of one source rate (resample.hip).  What the host loop refuses is refused here, before
// anything is launched: the host copy of the row table says which outputs every row has.
int masr_resample_rows(masr_engine* e, const void* src_dev, int32_t sample_format, int64_t src_stride, const int32_t* rows_host,
                       const int32_t* rows_dev, int32_t R, double ratio, const double* table_dev, int64_t nwin, int32_t num_table,
                       float* dst_dev, int32_t dst_rows, int64_t dst_stride, void* stream) {
    if (!e || !src_dev || !rows_host || !rows_dev || !dst_dev) return fail("masr_resample_rows: null argument");
    ENTER(e);
    if (sample_format != 0 && sample_format != 1) return fail("sample_format must be 0 (int16) or 1 (float32)");
    if (R < 0 || dst_rows <= 0 || dst_stride <= 0 || src_stride <= 0) return fail("masr_resample_rows: bad geometry");
    if (!(ratio > 0.0)) return fail("masr_resample_rows: ratio must be positive");
    if (!table_dev && ratio != 1.0) return fail("masr_resample_rows: no filter table for a ratio other than 1");
    double time_increment = 1.0;
    if (table_dev) {
        if (nwin <= 0 || nwin > (1 << 30) || num_table <= 0) return fail("masr_resample_rows: bad filter table");
        const double scale = ratio < 1.0 ? ratio : 1.0;
        if ((int64_t)(scale * (double)num_table) <= 0) return fail("masr_resample_rows: index_step <= 0 (ratio too small for the table)");
        time_increment = 1.0 / ratio;
    }
    for (int32_t i = 0; i < R; ++i) {
        const int64_t n_in = rows_host[3 * i], n_out = rows_host[3 * i + 1], row = rows_host[3 * i + 2];
        if (n_in <= 0 || n_in > src_stride || n_out < 0 || n_out > dst_stride || row < 0 || row >= dst_rows)
            return fail("masr_resample_rows: row " + std::to_string(i) + " does not fit its buffers");
        // the source index of an output grows with the output: the last one decides (resample.cpp: n >= n_orig)
        if (n_out > 0 && (int64_t)((double)(n_out - 1) * time_increment) >= n_in)
            return fail("masr_resample_rows: row " + std::to_string(i) + " asks for outputs beyond its input (n >= n_orig)");
    }
    launch_resample_rows(src_dev, sample_format, (long)src_stride, rows_dev, R, ratio, table_dev, (int)nwin, num_table, dst_dev,
                         (long)dst_stride, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

// The off-rate feeds of a streaming step in one launch (resample.hip resample_feeds_kernel): per feed the resample of the stream
// facade (masr/predict.py:260-281 -> AudioSegment.resample, masr/data_utils/audio.py:306-317).  masr_resample_plan (resample.cpp)
// refuses what the host loop refuses and what does not fit its buffers; the tile list the kernel indexes the feeds by is compared
// with the one the plan builds.  Nothing is launched for a refused call.
int masr_resample_feeds(masr_engine* e, const void* src_dev, int64_t src_bytes, const masr_resample_feed* feeds_host,
                        const masr_resample_feed* feeds_dev, int32_t n_feeds, const masr_resample_rate* rates_host,
                        const masr_resample_rate* rates_dev, int32_t n_rates, const int32_t* tiles_host, const int32_t* tiles_dev,
                        int64_t n_tiles, float* dst_dev, int32_t dst_rows, int64_t dst_stride, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    if (n_feeds == 0 && n_tiles == 0) return 0;
    if (!src_dev || !feeds_host || !feeds_dev || !rates_host || !rates_dev || !tiles_host || !tiles_dev || !dst_dev)
        return fail("masr_resample_feeds: null argument");
    int32_t bad = -1;
    const char* why = nullptr;
    int64_t want_tiles = 0;
    if (masr_resample_plan(feeds_host, n_feeds, rates_host, n_rates, src_bytes, dst_rows, dst_stride, nullptr, 0, &want_tiles, &bad, &why))
        return fail("masr_resample_feeds: " + (bad >= 0 ? "feed " + std::to_string(bad) + ": " : std::string()) + (why ? why : "refused"));
    if (want_tiles != n_tiles || n_tiles > 0x7fffffff) return fail("masr_resample_feeds: tile list is not the one masr_resample_plan builds (count)");
    int64_t at = 0;
    long lds = 0;
    for (int32_t k = 0; k < n_feeds; ++k) {
        for (int64_t t0 = 0; t0 < feeds_host[k].n_out; t0 += MASR_RESAMPLE_TILE, ++at)
            if (tiles_host[2 * at] != k || tiles_host[2 * at + 1] != (int32_t)t0)
                return fail("masr_resample_feeds: tile list is not the one masr_resample_plan builds (tile " + std::to_string(at) + ")");
        const long span = (long)masr_resample_tile_span(&rates_host[feeds_host[k].rate_slot]);
        if (span <= MASR_RESAMPLE_LDS_FLOATS && span > lds) lds = span;
    }
    launch_resample_feeds(src_dev, feeds_dev, n_feeds, rates_dev, tiles_dev, (long)n_tiles, (int)lds, dst_dev, (long)dst_stride,
                          (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

// kaldi.mfcc(num_mel_bins=80, num_ceps=n_ceps) on top of the fbank front-end (audio_featurizer.py:98-117).  The DCT / lifter
// tables follow torchaudio's float32 construction (functional.create_dct(norm='ortho') with column 0 = sqrt(1/80), transposed;
// lifter 1 + 0.5 * 22 * sin(pi * i / 22)).
int masr_mfcc_batch(masr_engine* e, const void* samples_dev, int32_t sample_format, const int32_t* n_samples_dev, int32_t B,
                    int32_t n_max, int32_t use_db_normalization, float target_db, int32_t n_ceps, float* mfcc_dev,
                    int32_t* n_frames_dev, float* gain_dev, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    if (n_ceps <= 0 || n_ceps > 80) return fail("n_ceps must be in [1, 80] (num_ceps <= num_mel_bins)");
    hipStream_t s = (hipStream_t)stream;
    if (e->dct_ceps != n_ceps) {
        std::vector<float> dct((size_t)80 * n_ceps), lif(n_ceps);
        const float step = (float)(M_PI / 80.0);
        for (int m = 0; m < 80; ++m)
            for (int c = 0; c < n_ceps; ++c) {
                float v = cosf((step * ((float)m + 0.5f)) * (float)c);
                if (c == 0) v *= (float)(1.0 / sqrt(2.0));
                v *= (float)sqrt(2.0 / 80.0);
                if (c == 0) v = (float)sqrt(1.0 / 80.0);
                dct[(size_t)m * n_ceps + c] = v;
            }
        for (int c = 0; c < n_ceps; ++c) lif[c] = 1.0f + 11.0f * sinf(((float)M_PI * (float)c) / 22.0f);
        HIPCHK(hipStreamSynchronize(s));
        CHK(upload(e, dct, &e->dct));           // (a changed n_ceps leaves the old table to the engine's owned list)
        CHK(upload(e, lif, &e->lifter));
        e->dct_ceps = n_ceps;
    }
    const int T_max = n_max >= 400 ? 1 + (n_max - 400) / 160 : 0;
    CHK(e->fb_scratch.ensure((size_t)B * std::max(T_max, 1) * 80 * sizeof(float)));
    CHK(masr_fbank_batch(e, samples_dev, sample_format, n_samples_dev, B, n_max, use_db_normalization, target_db,
                         e->fb_scratch.as<float>(), n_frames_dev, nullptr, gain_dev, stream));
    launch_mfcc(e->fb_scratch.as<float>(), (long)B * T_max, n_ceps, e->dct, e->lifter, mfcc_dev, s);
    LAUNCHCHK();
    return 0;
}

// AudioFeaturizer._compute_linear (audio_featurizer.py:73-95) for a padded batch: float32 (or int16 / 2^15) samples, optional
// dB normalisation (the same gain as the fbank path), [B, T, 161] log power spectra with T = (n_max - 320) / 160 + 1.
int masr_linear_batch(masr_engine* e, const void* samples_dev, int32_t sample_format, const int32_t* n_samples_dev, int32_t B,
                      int32_t n_max, int32_t use_db_normalization, float target_db, float* feats_dev, int32_t* n_frames_dev,
                      float* gain_dev, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    if (sample_format != 0 && sample_format != 1) return fail("sample_format must be 0 (int16) or 1 (float32)");
    hipStream_t s = (hipStream_t)stream;
    if (!e->lin_win) {
        std::vector<double> win(320), tw(640);
        double sumsq = 0.0;
        for (int i = 0; i < 320; ++i) {                 // np.hanning(320): 0.5 + 0.5 * cos(pi * (1 - M + 2 i) / (M - 1))
            win[i] = 0.5 + 0.5 * cos(M_PI * (double)(1 - 320 + 2 * i) / 319.0);
            sumsq += win[i] * win[i];
            tw[2 * i] = cos(2.0 * M_PI * i / 320.0);
            tw[2 * i + 1] = -sin(2.0 * M_PI * i / 320.0);
        }
        CHK(upload(e, win, &e->lin_win));
        CHK(upload(e, tw, &e->lin_tw));
        e->lin_scale = sumsq * 16000.0;
    }
    const int T_max = n_max >= 320 ? (n_max - 320) / 160 + 1 : 0;
    CHK(e->gain.ensure(sizeof(float) * fbank_gain_scratch_floats(B)));
    float* gain = e->gain.as<float>();
    if (use_db_normalization == 2) {
        if (!gain_dev) return fail("use_db_normalization = 2 needs the gains in gain_dev");
        HIPCHK(hipMemcpyAsync(gain, gain_dev, sizeof(float) * B, hipMemcpyDeviceToDevice, s));
    } else if (use_db_normalization)          // T_max = 0: only the RMS -> gain kernels of the fbank front-end run
        launch_fbank(samples_dev, sample_format, n_samples_dev, B, n_max, 1, target_db, e->fbank_tables(), nullptr, 0, gain, nullptr, s);
    launch_linear_spec(samples_dev, sample_format, n_samples_dev, B, n_max, use_db_normalization, gain, e->lin_win, e->lin_tw,
                       e->lin_scale, feats_dev, T_max, s);
    if (gain_dev && use_db_normalization == 1)
        HIPCHK(hipMemcpyAsync(gain_dev, gain, sizeof(float) * B, hipMemcpyDeviceToDevice, s));
    if (n_frames_dev) launch_linear_frame_counts(n_samples_dev, B, n_frames_dev, s);
    LAUNCHCHK();
    return 0;
}

// the offline hot path of one padded batch: samples -> features -> encoder -> CTC greedy -> collapse, either into three
// arrays (masr_transcribe_batch) or into packed rows (masr_transcribe_rows)
static int transcribe_impl(masr_engine* e, const void* samples_dev, int32_t fmt, const int32_t* n_samples_dev, int32_t B,
                           int32_t n_max, int32_t use_db_normalization, float target_db, const float* gain_dev,
                           int32_t decode_all_frames, int32_t* tokens_dev, int32_t* n_tokens_dev, float* score_dev,
                           int32_t* rows_dev, void* stream) {
    if (!e || !e->finalized) return fail("engine not finalized");
    ENTER(e);
    CallGuard call_guard(e, (hipStream_t)stream);
    if (n_max < 400) return fail("n_max < 400 samples: no frame");
    hipStream_t s = (hipStream_t)stream;
    const int d = enc_dim(e), F = e->cfg.n_mels;
    const int T = 1 + (n_max - 400) / 160, Tsub = sub_frames(e->input_layer, T);
    const bool halved = e->cfg.model_kind == 2 && e->stride_idx >= 0;      // efficient conformer: one more stride-2 stage
    const int Tq = halved ? (Tsub + 1) / 2 : Tsub;
    if (Tsub <= 0) return fail("utterances too short");
    // both forms of the collapse behind this pass (masr_ctc_collapse, launch_ctc_collapse_rows) take Tq frames per utterance: refused
    // here, before anything is computed (the Conformer families are bounded by max_pos as well, DeepSpeech2 by nothing else)
    if (Tq > CTC_COLLAPSE_MAX_FRAMES) return fail(std::string("masr_transcribe: ") + ctc_collapse_refusal);
    CHK(e->feats.ensure((size_t)B * T * F * sizeof(float)));
    CHK(e->nframes.ensure(sizeof(int) * 2 * B));
    CHK(e->enc.ensure((size_t)B * Tq * d * sizeof(float)));
    CHK(e->idx.ensure(sizeof(int) * B * Tq));
    CHK(e->maxp.ensure(sizeof(float) * B * Tq));
    int* nfr = e->nframes.as<int>();
    int* nenc = nfr + B;
    // (mode 2 reads the caller's gains: masr_fbank_batch copies them into its own scratch, the caller's array is not written)
    CHK(masr_fbank_batch(e, samples_dev, fmt, n_samples_dev, B, n_max, use_db_normalization, target_db,
                         e->feats.as<float>(), nullptr, nullptr, use_db_normalization == 2 ? const_cast<float*>(gain_dev) : nullptr,
                         stream));
    launch_frame_counts(n_samples_dev, B, nfr, nenc, halved ? 1 : 0, s, e->input_layer);
    {
        // decode_all_frames: the padded frames are decoded too (the reference's batch evaluation, trainer.py:340) -- then they
        // must be computed, whatever masr_debug_set key 38 says
        const int keep = e->skip_padding;
        if (decode_all_frames) e->skip_padding = 0;
        const int rc = masr_encode_full(e, e->feats.as<float>(), nfr, B, T, -1, e->enc.as<float>(), stream);
        e->skip_padding = keep;
        if (rc) return rc;
    }
    CHK(masr_ctc_greedy_frames(e, e->enc.as<float>(), B * Tq, e->idx.as<int>(), e->maxp.as<float>(), stream));
    if (rows_dev) {
        launch_ctc_collapse_rows(e->idx.as<int>(), e->maxp.as<float>(), decode_all_frames ? nullptr : nenc, B, Tq, 0, rows_dev, s);
        LAUNCHCHK();
        return 0;
    }
    CHK(masr_ctc_collapse(e, e->idx.as<int>(), e->maxp.as<float>(), decode_all_frames ? nullptr : nenc, B, Tq, 0,
                          tokens_dev, n_tokens_dev, score_dev, stream));
    return 0;
}

int masr_transcribe_batch(masr_engine* e, const int16_t* pcm_dev, const int32_t* n_samples_dev, int32_t B,
                          int32_t n_max, int32_t use_db_normalization, float target_db, int32_t decode_all_frames,
                          int32_t* tokens_dev, int32_t* n_tokens_dev, float* score_dev, void* stream) {
    if (use_db_normalization == 2) return fail("masr_transcribe_batch: supplied gains go through masr_transcribe_rows");
    return transcribe_impl(e, pcm_dev, 0, n_samples_dev, B, n_max, use_db_normalization, target_db, nullptr, decode_all_frames,
                           tokens_dev, n_tokens_dev, score_dev, nullptr, stream);
}

int masr_transcribe_rows(masr_engine* e, const void* samples_dev, int32_t sample_format, const int32_t* n_samples_dev, int32_t B,
                         int32_t n_max, int32_t use_db_normalization, float target_db, const float* gain_dev,
                         int32_t decode_all_frames, int32_t* rows_dev, void* stream) {
    if (!rows_dev) return fail("null argument");
    if (sample_format != 0 && sample_format != 1) return fail("sample_format: 0 = int16 PCM, 1 = float32");
    if (use_db_normalization == 2 && !gain_dev) return fail("use_db_normalization = 2 needs the gains in gain_dev");
    return transcribe_impl(e, samples_dev, sample_format, n_samples_dev, B, n_max, use_db_normalization, target_db, gain_dev,
                           decode_all_frames, nullptr, nullptr, nullptr, rows_dev, stream);
}

}  // extern "C"
