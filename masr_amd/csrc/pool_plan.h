// The framing arithmetic of the serving pool (pool.hip), as pure functions of frame and sample counts: the decoding windows of
// the reference facade (predict.py:283-306) and the frames a row of samples gives.  Host only (no HIP include): the pool's room
// check and its lock-step loop both go through pool_windows, masr_pool_window_plan (include/masr_hip.h) evaluates it without an
// engine, and tests/test_window_plan_cpu.py holds it to serving.window_plan.
#pragma once
#include <algorithm>

namespace masr {

// chunked decoding geometry (predict.py:283-290): 16 encoder frames per chunk, subsampling 4, context 7
constexpr int kDecodingChunk = 16, kSubsampling = 4, kContext = 7;
constexpr int kWindow = (kDecodingChunk - 1) * kSubsampling + kContext;      // 67 feature frames per window
constexpr int kStride = kSubsampling * kDecodingChunk;                       // 64
constexpr int kOverlap = kContext - kSubsampling;                            // 3 frames carried over

// yield(first, last) for every window of n_frames pending feature frames, a stride apart from 0: full windows only until the
// stream ends; at its end a short last window too, while it has the context's frames
template <class Yield>
inline void pool_windows(int n_frames, bool is_end, Yield&& yield) {
    if ((n_frames < kWindow && !is_end) || n_frames < kContext) return;
    const int left = is_end ? kContext : kWindow;
    for (int cur = 0; cur <= n_frames - left; cur += kStride) yield(cur, std::min(cur + kWindow, n_frames));
}

// feature frames of n samples: a 10 ms hop behind the first frame's min_samples (400: fbank and mfcc, 320: linear)
inline int pool_feature_frames(long n, int min_samples) { return n >= min_samples ? (int)((n - min_samples) / 160 + 1) : 0; }

}  // namespace masr
