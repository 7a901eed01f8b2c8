// Host-side band-limited sinc interpolation (J. O. Smith's algorithm as published in resampy: resampy/interpn.py
// _resample_loop, resampy/core.py resample) -- the resampler behind the reference's AudioSegment.resample
// (masr/data_utils/audio.py:306-317).  Same arithmetic, operation by operation, as the numpy form in
// masr_amd/data_utils/resample.py (which documents the algorithm and the filter table): double index arithmetic, weight =
// win[k] + eta * dwin[k] as a separate multiply and add, every tap added to the float accumulator through double.  An
// input-format step in front of the hot path; third-party algorithm, parity unpinned (resampy is absent from the image).
#include <cstdint>

#include "../../include/masr_hip.h"

#pragma STDC FP_CONTRACT OFF

extern "C" int masr_resample_f32(const float* x, int64_t n_orig, double ratio, const double* win, const double* dwin, int64_t nwin,
                                 int32_t num_table, float* y, int64_t n_out) {
    if (!x || !win || !dwin || !y || n_orig <= 0 || n_out < 0 || nwin <= 0 || num_table <= 0 || !(ratio > 0.0)) return 1;
    const double scale = ratio < 1.0 ? ratio : 1.0;
    const double time_increment = 1.0 / ratio;
    const int64_t index_step = (int64_t)(scale * (double)num_table);
    if (index_step <= 0) return 1;
    for (int64_t t = 0; t < n_out; ++t) {
        const double time_register = (double)t * time_increment;
        const int64_t n = (int64_t)time_register;
        if (n >= n_orig) return 1;
        float acc = 0.f;
        double frac = scale * (time_register - (double)n);
        double index_frac = frac * (double)num_table;
        int64_t offset = (int64_t)index_frac;
        double eta = index_frac - (double)offset;
        int64_t lim = (nwin - offset) / index_step;
        const int64_t i_max = n + 1 < lim ? n + 1 : lim;
        for (int64_t i = 0; i < i_max; ++i) {
            const int64_t k = offset + i * index_step;
            volatile double prod = eta * dwin[k];
            const double weight = win[k] + prod;
            volatile double term = weight * (double)x[n - i];
            acc = (float)((double)acc + term);
        }
        frac = scale - frac;
        index_frac = frac * (double)num_table;
        offset = (int64_t)index_frac;
        eta = index_frac - (double)offset;
        lim = (nwin - offset) / index_step;
        const int64_t k_max = n_orig - n - 1 < lim ? n_orig - n - 1 : lim;
        for (int64_t k2 = 0; k2 < k_max; ++k2) {
            const int64_t k = offset + k2 * index_step;
            volatile double prod = eta * dwin[k];
            const double weight = win[k] + prod;
            volatile double term = weight * (double)x[n + k2 + 1];
            acc = (float)((double)acc + term);
        }
        y[t] = acc;
    }
    return 0;
}

// ---- many short feeds of mixed rates in one launch (resample.hip resample_feeds_kernel): the host side -----------------------------
// What masr_resample_rows derives per call, derived once per source rate.
extern "C" int masr_resample_rate_fill(double ratio, const double* table_dev, int64_t nwin, int32_t num_table, masr_resample_rate* out) {
    if (!out || !table_dev || !(ratio > 0.0) || nwin <= 0 || nwin > (1 << 30) || num_table <= 0) return 1;
    const double scale = ratio < 1.0 ? ratio : 1.0;
    const int64_t index_step = (int64_t)(scale * (double)num_table);
    if (index_step <= 0) return 1;
    out->ratio = ratio;
    out->time_increment = 1.0 / ratio;
    out->scale = scale;
    out->table_dev = table_dev;
    out->index_step = (int32_t)index_step;
    out->nwin = (int32_t)nwin;
    out->num_table = num_table;
    out->reserved = 0;
    return 0;
}

// floats that hold the inputs of one 256-output tile whatever its position: the tile's own span + both wings (+ rounding slack).
// The launcher stages a rate's tiles in LDS when this is at most MASR_RESAMPLE_LDS_FLOATS, and reads global memory beyond.
extern "C" int64_t masr_resample_tile_span(const masr_resample_rate* r) {
    if (!r || r->index_step <= 0) return -1;
    return (int64_t)((double)(MASR_RESAMPLE_TILE - 1) * r->time_increment) + 2 * (int64_t)(r->nwin / r->index_step) + 4;
}

extern "C" int masr_resample_plan(const masr_resample_feed* feeds, int32_t n_feeds, const masr_resample_rate* rates, int32_t n_rates,
                                  int64_t src_bytes, int32_t dst_rows, int64_t dst_stride, int32_t* tiles, int64_t tiles_cap,
                                  int64_t* n_tiles, int32_t* bad_feed, const char** why) {
    const char* dummy_why = nullptr;
    int32_t dummy_bad = -1;
    if (!why) why = &dummy_why;
    if (!bad_feed) bad_feed = &dummy_bad;
    *bad_feed = -1;
    *why = nullptr;
    if (n_tiles) *n_tiles = 0;
#define RS_REFUSE(k, text) \
    do {                   \
        *bad_feed = (k);   \
        *why = (text);     \
        return 1;          \
    } while (0)
    if (n_feeds < 0 || n_rates < 0 || (n_feeds > 0 && (!feeds || !rates)) || !n_tiles) RS_REFUSE(-1, "null or negative argument");
    if (src_bytes < 0 || dst_rows <= 0 || dst_stride <= 0) RS_REFUSE(-1, "bad geometry");
    for (int32_t j = 0; j < n_rates; ++j) {
        masr_resample_rate want;
        const masr_resample_rate& r = rates[j];
        if (masr_resample_rate_fill(r.ratio, r.table_dev, r.nwin, r.num_table, &want)) RS_REFUSE(-1, "bad rate: ratio must be positive, index_step > 0, a table");
        if (r.time_increment != want.time_increment || r.scale != want.scale || r.index_step != want.index_step)
            RS_REFUSE(-1, "bad rate: not what masr_resample_rate_fill derives");
    }
    int64_t count = 0;
    for (int32_t k = 0; k < n_feeds; ++k) {
        const masr_resample_feed& f = feeds[k];
        if (f.rate_slot < 0 || f.rate_slot >= n_rates) RS_REFUSE(k, "unknown rate slot");
        const masr_resample_rate& r = rates[f.rate_slot];
        if (f.format != 0 && f.format != 1) RS_REFUSE(k, "sample format 0 = int16 PCM, 1 = float32");
        const int64_t width = f.format ? 4 : 2;
        if (f.n_in <= 0) RS_REFUSE(k, "n_in must be positive");
        if (f.src_offset < 0 || f.src_offset % width != 0 || f.src_offset > src_bytes || (int64_t)f.n_in * width > src_bytes - f.src_offset)
            RS_REFUSE(k, "source range unaligned or outside the source buffer");
        if (f.n_out < 1 || (int64_t)f.n_out != (int64_t)((double)f.n_in * r.ratio)) RS_REFUSE(k, "n_out must be (int)(n_in * ratio) >= 1");
        // the source index of an output grows with the output: the last one decides (masr_resample_f32: n >= n_orig)
        if ((int64_t)((double)(f.n_out - 1) * r.time_increment) >= (int64_t)f.n_in) RS_REFUSE(k, "asks for outputs beyond its input (n >= n_orig)");
        if (f.dst_row < 0 || f.dst_row >= dst_rows || f.dst_offset < 0 || (int64_t)f.dst_offset + f.n_out > dst_stride)
            RS_REFUSE(k, "destination range outside its row");
        for (int64_t t0 = 0; t0 < f.n_out; t0 += MASR_RESAMPLE_TILE) {
            if (tiles && count < tiles_cap) {
                tiles[2 * count] = k;
                tiles[2 * count + 1] = (int32_t)t0;
            }
            ++count;
        }
    }
#undef RS_REFUSE
    *n_tiles = count;
    return 0;
}
