// Band-limited sinc interpolation of a batch of rows on the GPU: the loop of resample.cpp (resampy's published _resample_loop,
// behind the reference's AudioSegment.resample, masr/data_utils/audio.py:306-317), one thread per output sample.  Same arithmetic,
// operation for operation: time_register / frac / offset / eta in double, weight = win[k] + eta * dwin[k] as a separate multiply
// and add, every tap folded in as acc = (float)((double)acc + weight * (double)x[.]), left wing before right wing, nearest tap
// first -- so a row comes out bit for bit as masr_resample_f32 makes it.  This file is built with -ffp-contract=off (build.py
// FILE_FLAGS): a fused eta * dwin + win or weight * x + acc would round once where the host rounds twice.  Denormals are kept
// (the default kernel mode; the flag that would flush them is switched off explicitly for this file).
//
// Shape: a workgroup owns TILE consecutive outputs of one row.  The inputs they touch -- their span divided by the ratio plus one
// wing on either side -- are staged once in LDS as float32 (int16 PCM is scaled by 2^-15 there: the float32 the host makes).  The
// table is read as one 16-byte (win[k], dwin[k]) pair per tap; at tap i every output of the workgroup reads inside the window
// [i * index_step, (i + 1) * index_step] of it, so the pairs come out of the vector cache.  The chain through the float32
// accumulator is inherent in the rounding; it is hidden by the waves in flight, never by reordering the sum.
#include "../../include/masr_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace masr {

namespace {

constexpr int RS_TILE = 256;

struct RsRow {          // rows_dev [R][3]
    int n_in, n_out, dst_row;
};

__device__ __forceinline__ float rs_sample(const void* row, int fmt, long j) {
    return fmt ? reinterpret_cast<const float*>(row)[j] : (float)reinterpret_cast<const int16_t*>(row)[j] * 0x1p-15f;
}

// dst[dst_row][t] for t in [0, dst_stride): the resampled row, then zeros from n_out on
__global__ __launch_bounds__(RS_TILE) void resample_rows_kernel(const void* __restrict__ src, int fmt, long src_stride,
                                                                const RsRow* __restrict__ rows, double time_increment,
                                                                double scale, int index_step, const double2* __restrict__ table,
                                                                int nwin, int num_table, int lds_cap, float* __restrict__ dst,
                                                                long dst_stride) {
    extern __shared__ float xs[];
    const RsRow r = rows[blockIdx.y];
    const long t0 = (long)blockIdx.x * RS_TILE;
    const long t = t0 + threadIdx.x;
    float* out = dst + (long)r.dst_row * dst_stride;
    if (t0 >= r.n_out) {                                   // (uniform) a tile of padding only
        if (t < dst_stride) out[t] = 0.f;
        return;
    }
    const char* row = reinterpret_cast<const char*>(src) + (long)blockIdx.y * src_stride * (fmt ? 4 : 2);
    // inputs of the tile: [n(first output) - wing + 1, n(last output) + wing], clipped to the row
    const long wing = nwin / index_step;
    const long t_last = (t0 + RS_TILE < r.n_out ? t0 + RS_TILE : (long)r.n_out) - 1;
    long base = (long)((double)t0 * time_increment) - wing + 1;
    long end = (long)((double)t_last * time_increment) + wing + 1;
    base = base < 0 ? 0 : base;
    end = end > r.n_in ? r.n_in : end;
    const bool staged = end - base <= lds_cap;             // (uniform; the launcher sizes lds_cap so that it holds)
    if (staged) {
        for (long j = base + threadIdx.x; j < end; j += RS_TILE) xs[j - base] = rs_sample(row, fmt, j);
        __syncthreads();
    }
    if (t >= r.n_out) {
        if (t < dst_stride) out[t] = 0.f;
        return;
    }
    const double time_register = (double)t * time_increment;
    const long n = (long)time_register;
    float acc = 0.f;
    if (n < r.n_in) {                                      // (the launcher has refused rows where this fails)
        double frac = scale * (time_register - (double)n);
        double index_frac = frac * (double)num_table;
        long offset = (long)index_frac;
        double eta = index_frac - (double)offset;
        long lim = (nwin - offset) / index_step;
        const int i_max = (int)(n + 1 < lim ? n + 1 : lim);
        const double2* tp = table + offset;
        if (staged) {
            const float* xp = xs + (n - base);
            for (int i = 0; i < i_max; ++i) {
                const double2 w = tp[(long)i * index_step];
                const double weight = w.x + eta * w.y;
                acc = (float)((double)acc + weight * (double)xp[-i]);
            }
        } else {
            for (int i = 0; i < i_max; ++i) {
                const double2 w = tp[(long)i * index_step];
                const double weight = w.x + eta * w.y;
                acc = (float)((double)acc + weight * (double)rs_sample(row, fmt, n - i));
            }
        }
        frac = scale - frac;
        index_frac = frac * (double)num_table;
        offset = (long)index_frac;
        eta = index_frac - (double)offset;
        lim = (nwin - offset) / index_step;
        const int k_max = (int)(r.n_in - n - 1 < lim ? r.n_in - n - 1 : lim);
        tp = table + offset;
        if (staged) {
            const float* xp = xs + (n + 1 - base);
            for (int i = 0; i < k_max; ++i) {
                const double2 w = tp[(long)i * index_step];
                const double weight = w.x + eta * w.y;
                acc = (float)((double)acc + weight * (double)xp[i]);
            }
        } else {
            for (int i = 0; i < k_max; ++i) {
                const double2 w = tp[(long)i * index_step];
                const double weight = w.x + eta * w.y;
                acc = (float)((double)acc + weight * (double)rs_sample(row, fmt, n + 1 + i));
            }
        }
    }
    out[t] = acc;
}

// rows already at the target rate: dst[dst_row][t] = the float32 sample (int16 PCM x 2^-15), zeros from n_out on
__global__ __launch_bounds__(RS_TILE) void resample_copy_kernel(const void* __restrict__ src, int fmt, long src_stride,
                                                                const RsRow* __restrict__ rows, float* __restrict__ dst,
                                                                long dst_stride) {
    const RsRow r = rows[blockIdx.y];
    const long t = (long)blockIdx.x * RS_TILE + threadIdx.x;
    if (t >= dst_stride) return;
    const char* row = reinterpret_cast<const char*>(src) + (long)blockIdx.y * src_stride * (fmt ? 4 : 2);
    dst[(long)r.dst_row * dst_stride + t] = t < r.n_out ? rs_sample(row, fmt, t) : 0.f;
}

// ---- many short feeds of mixed rates in one launch (a streaming pool's step) ------------------------------------------------------
// The chunks of a step are 0.1 - 0.64 s each, at their own rates and formats, each landing at its own offset of a session's row.
// One flat grid over tiles: tiles[b] = (feed, first output); the workgroup reads its feed's descriptor and its rate's slot (time
// increment, scale, index step, table: what the row kernel gets as launch arguments) from device memory, then does what the row
// kernel does -- the same staging, the same per-output loop, operation for operation.  It writes its own outputs and nothing else.
static_assert(sizeof(masr_resample_feed) == 32 && sizeof(masr_resample_rate) == 48, "descriptor layout (masr_hip.h)");
static_assert(RS_TILE == MASR_RESAMPLE_TILE, "tile (masr_hip.h)");

__global__ __launch_bounds__(RS_TILE) void resample_feeds_kernel(const char* __restrict__ src, const masr_resample_feed* __restrict__ feeds,
                                                                 int n_feeds, const masr_resample_rate* __restrict__ rates,
                                                                 const int2* __restrict__ tiles, int lds_cap, float* __restrict__ dst,
                                                                 long dst_stride) {
    extern __shared__ float xs[];
    const int2 tile = tiles[blockIdx.x];
    if (tile.x < 0 || tile.x >= n_feeds) return;           // (uniform; the entry point has checked the list)
    const masr_resample_feed f = feeds[tile.x];
    const masr_resample_rate r = rates[f.rate_slot];
    const int fmt = f.format, index_step = r.index_step, nwin = r.nwin, num_table = r.num_table;
    const double time_increment = r.time_increment, scale = r.scale;
    const double2* table = reinterpret_cast<const double2*>(r.table_dev);
    const long t0 = tile.y;
    const long t = t0 + threadIdx.x;
    const char* row = src + f.src_offset;
    float* out = dst + (long)f.dst_row * dst_stride + f.dst_offset;
    // inputs of the tile: [n(first output) - wing + 1, n(last output) + wing], clipped to the feed
    const long wing = nwin / index_step;
    const long t_last = (t0 + RS_TILE < f.n_out ? t0 + RS_TILE : (long)f.n_out) - 1;
    long base = (long)((double)t0 * time_increment) - wing + 1;
    long end = (long)((double)t_last * time_increment) + wing + 1;
    base = base < 0 ? 0 : base;
    end = end > f.n_in ? f.n_in : end;
    const bool staged = end - base <= lds_cap;             // (uniform)
    if (staged) {
        for (long j = base + threadIdx.x; j < end; j += RS_TILE) xs[j - base] = rs_sample(row, fmt, j);
        __syncthreads();
    }
    if (t >= f.n_out) return;
    const double time_register = (double)t * time_increment;
    const long n = (long)time_register;
    float acc = 0.f;
    if (n < f.n_in) {                                      // (the entry point has refused feeds where this fails)
        double frac = scale * (time_register - (double)n);
        double index_frac = frac * (double)num_table;
        long offset = (long)index_frac;
        double eta = index_frac - (double)offset;
        long lim = (nwin - offset) / index_step;
        const int i_max = (int)(n + 1 < lim ? n + 1 : lim);
        const double2* tp = table + offset;
        if (staged) {
            const float* xp = xs + (n - base);
            for (int i = 0; i < i_max; ++i) {
                const double2 w = tp[(long)i * index_step];
                const double weight = w.x + eta * w.y;
                acc = (float)((double)acc + weight * (double)xp[-i]);
            }
        } else {
            for (int i = 0; i < i_max; ++i) {
                const double2 w = tp[(long)i * index_step];
                const double weight = w.x + eta * w.y;
                acc = (float)((double)acc + weight * (double)rs_sample(row, fmt, n - i));
            }
        }
        frac = scale - frac;
        index_frac = frac * (double)num_table;
        offset = (long)index_frac;
        eta = index_frac - (double)offset;
        lim = (nwin - offset) / index_step;
        const int k_max = (int)(f.n_in - n - 1 < lim ? f.n_in - n - 1 : lim);
        tp = table + offset;
        if (staged) {
            const float* xp = xs + (n + 1 - base);
            for (int i = 0; i < k_max; ++i) {
                const double2 w = tp[(long)i * index_step];
                const double weight = w.x + eta * w.y;
                acc = (float)((double)acc + weight * (double)xp[i]);
            }
        } else {
            for (int i = 0; i < k_max; ++i) {
                const double2 w = tp[(long)i * index_step];
                const double weight = w.x + eta * w.y;
                acc = (float)((double)acc + weight * (double)rs_sample(row, fmt, n + 1 + i));
            }
        }
    }
    out[t] = acc;
}

}  // namespace

// floats of LDS that hold the inputs of one tile whatever its position: the tile's own span + both wings (+ rounding slack)
static long resample_tile_span(double time_increment, int index_step, int nwin) {
    return (long)((double)(RS_TILE - 1) * time_increment) + 2 * (long)(nwin / index_step) + 4;
}

void launch_resample_rows(const void* src, int sample_format, long src_stride, const int* rows_dev, int R, double ratio,
                          const double* table, int nwin, int num_table, float* dst, long dst_stride, hipStream_t s) {
    if (R <= 0 || dst_stride <= 0) return;
    const dim3 grid((unsigned)((dst_stride + RS_TILE - 1) / RS_TILE), (unsigned)R);
    const RsRow* rows = reinterpret_cast<const RsRow*>(rows_dev);
    if (!table) {
        hipLaunchKernelGGL(resample_copy_kernel, grid, dim3(RS_TILE), 0, s, src, sample_format, src_stride, rows, dst, dst_stride);
        return;
    }
    const double scale = ratio < 1.0 ? ratio : 1.0;
    const double time_increment = 1.0 / ratio;
    const int index_step = (int)(scale * (double)num_table);
    // the staged span when it fits the 64 KB every kernel may use without opting in; beyond that (ratios below ~1/20) the
    // kernel reads its inputs from global memory
    long cap = resample_tile_span(time_increment, index_step, nwin);
    if (cap > 16000) cap = 0;
    hipLaunchKernelGGL(resample_rows_kernel, grid, dim3(RS_TILE), (size_t)cap * sizeof(float), s, src, sample_format, src_stride,
                       rows, time_increment, scale, index_step, reinterpret_cast<const double2*>(table), nwin, num_table, (int)cap,
                       dst, dst_stride);
}

// lds_floats: the largest tile span among the rates in use that fits MASR_RESAMPLE_LDS_FLOATS (the caller's, from
// masr_resample_tile_span); a rate whose tiles span more reads global memory
void launch_resample_feeds(const void* src, const masr_resample_feed* feeds_dev, int n_feeds, const masr_resample_rate* rates_dev,
                           const int* tiles_dev, long n_tiles, int lds_floats, float* dst, long dst_stride, hipStream_t s) {
    if (n_tiles <= 0 || n_feeds <= 0) return;
    hipLaunchKernelGGL(resample_feeds_kernel, dim3((unsigned)n_tiles), dim3(RS_TILE), (size_t)lds_floats * sizeof(float), s,
                       reinterpret_cast<const char*>(src), feeds_dev, n_feeds, rates_dev, reinterpret_cast<const int2*>(tiles_dev),
                       lds_floats, dst, dst_stride);
}

}  // namespace masr
