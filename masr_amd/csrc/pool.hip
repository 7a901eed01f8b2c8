// libmasr_hip.so -- serving pool: any number of concurrent predict_stream sessions on ONE engine, one C call per step.
//
// What the reference keeps per stream in python (masr/predict.py:237-343: samples not yet framed, feature frames not yet
// consumed by a decoding window, the greedy decoder's history; infer_server.py:103-156 holds one such predictor per websocket)
// is kept here per session; the device work of all sessions that were fed since the last step is done together:
//   pending PCM (int16 wire format or float32) -> x / 2^15 -> [carried-over | new] samples per session in pinned memory -> ONE
//   upload -> mean squares (numpy's summation order) -> gains by the caller's evaluator (the reference's scalar numpy expressions;
//   NULL: libm) -> ONE ragged feature launch -> the new frames appended to the sessions' rows of a device-resident frame pool
//   -> the 67-frame decoding windows of all sessions gathered from it and advanced in lock-step through masr_encode_chunk ->
//   (argmax, max prob) frames appended to device-resident histories -> ONE collapse launch over the histories of the sessions
//   that advanced -> ONE copy back of the packed rows [tokens | count | score bits].
// Round 3 did this framing in python (masr_amd/serving.py: 1.4 of the 4.4 ms of a 128-stream step); the python class keeps the
// sessions' handles and builds the text.  Greedy sessions only (beam-search sessions keep their per-session python path).
// Sessions fed off the model's sample rate (masr_pool_set_rate, masr_pool_step_rates): their feeds are staged RAW, their rows are
// assembled with holes, and one masr_resample_feeds launch behind the upload fills the holes -- where the facade resamples every
// chunk on the host (predict.py:260-281 -> data_utils/audio.py:306-317).  Lengths are (int)(n * ratio): known without the device.
// Host-side only: the kernels are the engine's (masr_hip.h entry points) plus two copy / collapse launches in elementwise.hip.
#include <string.h>

#include <chrono>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/masr_hip.h"
#include "common.h"
#include "engine_state.h"      // masr::subsampled_frames and masr::engine_fail, nothing else: the engine is used through the C ABI
#include "pool_plan.h"         // the decoding windows (kWindow, kStride, kOverlap; pool_windows) and pool_feature_frames

using namespace masr;

#define PFAIL(msg) return masr::engine_fail(msg)
#define PHIP(expr)                                                                                                        \
    do {                                                                                                                  \
        hipError_t _e = (expr);                                                                                           \
        if (_e != hipSuccess) return masr::engine_fail(std::string(#expr) + ": " + hipGetErrorString(_e) + " (pool.hip)"); \
    } while (0)
#define PCHK(expr)         \
    do {                   \
        int _r = (expr);   \
        if (_r) return _r; \
    } while (0)

namespace {

constexpr int64_t kMaxFeedSamples = (int64_t)1 << 28;                        // per feed (4.6 h at 16 kHz): anything above is a caller bug

struct Dev {                     // grow-only device buffer; `keep` bytes of the old contents survive a growth
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t n, size_t keep, hipStream_t s) {
        if (n <= bytes) return 0;
        void* q = nullptr;
        const size_t want = n + n / 4 + 256;
        PHIP(hipMalloc(&q, want));
        PHIP(hipMemsetAsync(q, 0, want, s));
        if (p && keep) PHIP(hipMemcpyAsync(q, p, std::min(keep, bytes), hipMemcpyDeviceToDevice, s));
        if (p) {
            PHIP(hipStreamSynchronize(s));
            PHIP(hipFree(p));
        }
        p = q;
        bytes = want;
        return 0;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

struct Pinned {                  // pinned host area, bump-allocated per step; copies out of it are asynchronous
    char* p = nullptr;
    size_t bytes = 0, used = 0;
    std::vector<char*> retired;
    int reset() {
        for (char* r : retired) (void)hipHostFree(r);
        retired.clear();
        used = 0;
        return 0;
    }
    int take(size_t n, void** out) {
        const size_t at = (used + 63) & ~(size_t)63;
        if (at + n > bytes) {                      // copies in flight keep the old area alive until the next reset()
            if (p) retired.push_back(p);
            const size_t want = std::max(2 * bytes, 2 * n + 4096);
            void* q = nullptr;
            PHIP(hipHostMalloc(&q, want, hipHostMallocDefault));
            p = (char*)q;
            bytes = want;
            used = n;
            *out = p;
            return 0;
        }
        used = at + n;
        *out = p + at;
        return 0;
    }
    void release() {
        reset();
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

struct Session {
    int sid = -1;                 // engine stream id == pool handle
    int row = 0;                  // row of the frame pool and of the histories
    std::vector<float> remained;  // samples not yet turned into frames (already normalised: re-normalised on every call, audio.py:304)
    int f0 = 0, nf = 0;           // live feature frames: f0 .. f0 + nf of the session's row
    int frames = 0;               // encoder frames decoded so far
};

struct Tail {                    // carried-over samples of a session with off-rate feeds: on their way back through pinned memory
    int sid;
    const float* src;            // (in the pool's pinned area: valid until the next step resets it)
    size_t n;
    float gain;
    bool scaled;
};

constexpr int kMaxRates = 64;    // source rates per pool

}  // namespace

struct masr_pool {
    masr_engine* e = nullptr;
    int device = 0;
    int method = 0, n_mfcc = 40, use_db = 1, F = 80, min_samples = 400, max_frames_out = 0;
    float target_db = -20.f;
    std::map<int, Session> sessions;
    std::vector<int> free_rows;
    int n_rows = 0;
    // device-resident state
    Dev feat;                     // [rows_cap][feat_cap][F]
    int rows_cap = 0, feat_cap = 512;
    Dev hist_idx, hist_mp;        // [hist_rows][hist_cap]
    int hist_rows = 0, hist_cap = 0;
    // per-step work buffers; of off-rate feeds: the step's raw bytes + descriptors, the tails
    Dev samples, lens, ms, gains, feats, win, idx, mp, segs, meta, rows_out, raw, tails_dev;
    // every Dev above, for masr_pool_destroy
    std::vector<Dev*> buffers() {
        return {&feat, &hist_idx, &hist_mp, &samples, &lens, &ms, &gains, &feats, &win, &idx, &mp, &segs, &meta, &rows_out, &raw, &tails_dev};
    }
    // off-rate feeds: rate slots (host copy + device table, filter tables), the tails on their way back
    std::vector<masr_resample_rate> rates;
    std::map<int, int> rate_of;   // sr_orig -> slot
    std::vector<void*> rate_tables;
    masr_resample_rate* rates_dev = nullptr;
    std::vector<Tail> tails;      // not yet copied into their sessions
    Pinned pin;
    hipEvent_t ev = nullptr;      // the previous step's copies out of `pin`
    bool pending = false;
    // results of the last step (pinned; valid until the next step)
    std::vector<int32_t> handles, state;
    // host time per phase, accumulated (masr_pool_profile): assemble | upload + mean squares + wait | gains | features + frames
    // | windows | collapse + copy back + wait; and the number of steps
    double prof[6] = {0, 0, 0, 0, 0, 0};
    long prof_steps = 0;
};

namespace {

// d, [old_rows][old_row_bytes], becomes [rows][new_row_bytes] with the old rows at the front of the first old_rows new ones
int regrow_rows(Dev& d, size_t rows, size_t old_rows, size_t old_row_bytes, size_t new_row_bytes, hipStream_t s) {
    Dev nd;
    PCHK(nd.ensure(rows * new_row_bytes, 0, s));
    if (d.p && old_rows && old_row_bytes)
        PHIP(hipMemcpy2DAsync(nd.p, new_row_bytes, d.p, old_row_bytes, old_row_bytes, old_rows, hipMemcpyDeviceToDevice, s));
    PHIP(hipStreamSynchronize(s));
    d.release();
    d = nd;
    return 0;
}

// make the histories at least [rows][frames] and the frame pool at least [rows][feat_cap] (contents kept)
int grow_state(masr_pool* p, int rows, int frames, hipStream_t s) {
    if (rows > p->hist_rows || frames > p->hist_cap) {
        const int r1 = rows <= p->hist_rows ? p->hist_rows : std::max({rows, 2 * p->hist_rows, 16});
        const int f1 = frames <= p->hist_cap ? p->hist_cap : std::max({frames, 2 * p->hist_cap, 256});
        for (Dev* d : {&p->hist_idx, &p->hist_mp})
            PCHK(regrow_rows(*d, (size_t)r1, (size_t)p->hist_rows, (size_t)p->hist_cap * 4, (size_t)f1 * 4, s));
        p->hist_rows = r1;
        p->hist_cap = f1;
    }
    if (rows > p->rows_cap) {
        const int r1 = std::max({rows, 2 * p->rows_cap, 16});
        PCHK(p->feat.ensure((size_t)r1 * p->feat_cap * p->F * 4, (size_t)p->rows_cap * p->feat_cap * p->F * 4, s));
        p->rows_cap = r1;
    }
    return 0;
}

// wider rows of the frame pool (a whole utterance fed in one call)
int widen_feat(masr_pool* p, int cap, hipStream_t s) {
    PCHK(regrow_rows(p->feat, (size_t)p->rows_cap, (size_t)p->rows_cap, (size_t)p->feat_cap * p->F * 4, (size_t)cap * p->F * 4, s));
    p->feat_cap = cap;
    return 0;
}

// the carried-over samples that came back from the device (the stream has been waited for since their copy was queued)
void settle_tails(masr_pool* p) {
    for (const Tail& t : p->tails) {
        auto it = p->sessions.find(t.sid);
        if (it == p->sessions.end() || it->second.remained.size() != t.n) continue;
        std::vector<float>& r = it->second.remained;
        if (t.n) memcpy(r.data(), t.src, t.n * 4);
        if (t.scaled)
            for (float& v : r) v *= t.gain;
    }
    p->tails.clear();
}

void drop_tails(masr_pool* p, int sid) {
    p->tails.erase(std::remove_if(p->tails.begin(), p->tails.end(), [sid](const Tail& t) { return t.sid == sid; }), p->tails.end());
}

// A step that fails after it has queued tails (their sessions hold placeholders) must not leave them to be read before their copy
// has landed: on any exit but the regular one the stream is waited for and the tails are settled.
struct TailGuard {
    masr_pool* p;
    hipStream_t s;
    bool done = false;
    ~TailGuard() {
        if (done || p->tails.empty()) return;
        (void)hipStreamSynchronize(s);
        settle_tails(p);
    }
};

int upload(masr_pool* p, Dev& dst, const void* host_in_pin, size_t n, hipStream_t s) {
    PCHK(dst.ensure(n, 0, s));
    PHIP(hipMemcpyAsync(dst.p, host_in_pin, n, hipMemcpyHostToDevice, s));
    return 0;
}

// One masr_pool_step_rates call: its arguments, and what its phases (below, in the order they run) hand to each other.  The
// per-session vectors are indexed alike: session i of the step is sess[i], with end_flag[i], feeds_of[i], len[i], fresh[i], ...
struct Step {
    // the call
    int32_t n_feeds;
    const int32_t* feed_handle;
    const void* const* feed_samples;
    const int64_t* feed_n;
    const int32_t *feed_format, *feed_is_end, *feed_rate_slot;
    masr_gain_fn gain_fn;
    void* gain_user;
    int32_t* n_sessions;
    const int32_t **handles_out, **state_out, **rows_host;
    int32_t* row_width;
    int32_t** rows_dev;
    // check_feeds
    std::vector<int64_t> out_n;              // samples every feed gives at the model's rate
    int n_off = 0;                           // feeds off that rate
    // group_by_session, admit
    std::vector<Session*> sess;              // in the order they were first fed
    std::vector<int> end_flag;
    std::vector<std::vector<int>> feeds_of;
    std::vector<long> len;                   // samples of the session's row: carried-over + fed
    std::vector<int32_t> refused;            // handles of the sessions left out
    int n = 0;                               // sessions that take part
    // assemble_rows: rows of n_max floats in pinned memory; the raw bytes of off-rate feeds and their descriptors
    long n_max = 0;
    float* buf = nullptr;
    int32_t* lens_h = nullptr;
    std::vector<char> off_sess;              // the session has an off-rate feed in this step
    std::vector<masr_resample_feed> rs_feeds;
    size_t raw_bytes = 0;
    char* raw_h = nullptr;
    // upload_and_resample, gains, features
    std::vector<int> fresh;                  // feature frames the row gives
    std::vector<const float*> tail_h;        // where the carried-over samples of an off-rate session come back (pinned)
    float* gains_h = nullptr;
    int tmax = 0;                            // frames per row of the feature launch
    // append_frames, run_windows: the windows, and the step's segment tables (ONE device array; every launch gets its own slice)
    std::vector<std::vector<std::pair<int, int>>> plans;
    size_t lockstep = 0;                     // windows of the session that has most
    PoolSeg* seg_pin = nullptr;
    size_t seg_at = 0;
    // collapse_and_fetch: packed rows of the na sessions that advanced
    int na = 0, width = 0;
    int32_t* rows_h = nullptr;
    // host time since the last lap goes to slot k of masr_pool_profile
    std::chrono::steady_clock::time_point t_last;
    void lap(masr_pool* p, int k) {
        const auto t = std::chrono::steady_clock::now();
        p->prof[k] += std::chrono::duration<double, std::milli>(t - t_last).count();
        t_last = t;
    }
};

// validate EVERYTHING before any session state is touched: a bad feed fails the call with nothing committed
int check_feeds(const masr_pool* p, Step& st) {
    if (!st.feed_handle || !st.feed_samples || !st.feed_n || !st.feed_format || !st.feed_is_end) PFAIL("masr_pool_step: null feed arrays");
    for (int k = 0; k < st.n_feeds; ++k) {
        if (p->sessions.find(st.feed_handle[k]) == p->sessions.end()) PFAIL("masr_pool_step: unknown handle");
        if (st.feed_format[k] != 0 && st.feed_format[k] != 1) PFAIL("masr_pool_step: sample format 0 = int16 PCM, 1 = float32");
        if (st.feed_n[k] < 0 || st.feed_n[k] > kMaxFeedSamples) PFAIL("masr_pool_step: feed_n out of range (0 .. 2^28 samples)");
        if (st.feed_n[k] > 0 && !st.feed_samples[k]) PFAIL("masr_pool_step: null sample pointer with feed_n > 0");
    }
    // samples every feed gives at the model's rate: its own count, or (int)(n * ratio) of an off-rate feed (resample.cpp)
    st.out_n.assign(st.feed_n, st.feed_n + st.n_feeds);
    for (int k = 0; st.feed_rate_slot && k < st.n_feeds; ++k) {
        const int slot = st.feed_rate_slot[k];
        if (slot == -1) continue;
        if (slot < 0 || slot >= (int)p->rates.size()) PFAIL("masr_pool_step: unknown rate slot (masr_pool_set_rate)");
        const masr_resample_rate& r = p->rates[slot];
        const int64_t m = (int64_t)((double)st.feed_n[k] * r.ratio);
        if (m < 1 || m > kMaxFeedSamples) PFAIL("masr_pool_step: feed " + std::to_string(k) + " is too small to resample (or gives more than 2^28 samples)");
        if ((int64_t)((double)(m - 1) * r.time_increment) >= st.feed_n[k])
            PFAIL("masr_pool_step: feed " + std::to_string(k) + " asks for outputs beyond its input (n >= n_orig)");
        st.out_n[k] = m;
        ++st.n_off;
    }
    return 0;
}

// sessions of this step, in the order they were first fed
void group_by_session(masr_pool* p, Step& st) {
    std::map<int, int> pos;
    for (int k = 0; k < st.n_feeds; ++k) {
        auto it = p->sessions.find(st.feed_handle[k]);
        auto q = pos.find(st.feed_handle[k]);
        if (q == pos.end()) {
            q = pos.emplace(st.feed_handle[k], (int)st.sess.size()).first;
            st.sess.push_back(&it->second);
            st.end_flag.push_back(0);
            st.feeds_of.emplace_back();
        }
        st.end_flag[q->second] |= st.feed_is_end[k] ? 1 : 0;
        st.feeds_of[q->second].push_back(k);
    }
}

// a session whose stream cannot take the frames this step would emit (masr_encode_chunk would refuse the whole lock-step
// call: "stream exceeds its max_frames_out / max_pos") is LEFT OUT, untouched, and reported with state -1: one full
// session does not fail the step of the others
int admit(masr_pool* p, Step& st) {
    std::vector<Session*> keep_s;
    std::vector<int> keep_e;
    std::vector<std::vector<int>> keep_f;
    for (size_t i = 0; i < st.sess.size(); ++i) {
        long tot = (long)st.sess[i]->remained.size();
        for (int k : st.feeds_of[i]) tot += st.out_n[k];
        long emit = 0;                                   // (the unit of masr_stream_room: before any stride layer)
        pool_windows(st.sess[i]->nf + pool_feature_frames(tot, p->min_samples), st.end_flag[i] != 0,
                     [&](int first, int last) { emit += subsampled_frames(p->e, last - first); });
        int32_t room = 0;
        PCHK(masr_stream_room(p->e, st.sess[i]->sid, &room));
        if (emit > 0 && emit > room) {                   // (masr_stream_room already holds back the Efficient-Conformer's group padding)
            st.refused.push_back(st.sess[i]->sid);
            continue;
        }
        keep_s.push_back(st.sess[i]);
        keep_e.push_back(st.end_flag[i]);
        keep_f.push_back(std::move(st.feeds_of[i]));
        st.len.push_back(tot);
    }
    st.sess.swap(keep_s);
    st.end_flag.swap(keep_e);
    st.feeds_of.swap(keep_f);
    st.n = (int)st.sess.size();
    return 0;
}

// the first phase that touches the pool: the previous step's copies are waited for, its tails settled, the pinned area reset
int begin_step(masr_pool* p, Step& st, hipStream_t s) {
    if (p->pending) {                                // the previous step's copies out of the pinned area (long done)
        PHIP(hipEventSynchronize(p->ev));
        p->pending = false;
    }
    if (!p->ev) PHIP(hipEventCreateWithFlags(&p->ev, hipEventDisableTiming));
    settle_tails(p);                                 // (a step that ended without a wait left its tails in the pinned area)
    PCHK(p->pin.reset());
    int max_row = 0;
    for (Session* q : st.sess) max_row = std::max(max_row, q->row);
    PCHK(grow_state(p, max_row + 1, std::max(p->hist_cap, 256), s));
    return 0;
}

// [carried-over | fed] samples of every session, float32, in pinned memory (predict.py:260-281)
int assemble_rows(masr_pool* p, Step& st) {
    const int n = st.n;
    st.n_max = p->min_samples;
    for (long len : st.len) st.n_max = std::max(st.n_max, len);
    const long n_max = st.n_max;
    // off-rate feeds of the sessions that take part: their raw bytes are staged in pinned memory as fed, 4-byte aligned
    st.off_sess.assign(n, 0);
    if (st.n_off)
        for (int i = 0; i < n; ++i)
            for (int k : st.feeds_of[i])
                if (st.feed_rate_slot[k] >= 0) {
                    st.raw_bytes = ((st.raw_bytes + 3) & ~(size_t)3) + (size_t)st.feed_n[k] * (st.feed_format[k] ? 4 : 2);
                    st.off_sess[i] = 1;
                }
    if (st.raw_bytes) PCHK(p->pin.take(st.raw_bytes, (void**)&st.raw_h));
    size_t raw_at = 0;
    PCHK(p->pin.take((size_t)n * n_max * 4, (void**)&st.buf));
    PCHK(p->pin.take((size_t)n * 4, (void**)&st.lens_h));
    for (int i = 0; i < n; ++i) {
        float* row = st.buf + (size_t)i * n_max;
        size_t at = st.sess[i]->remained.size();
        if (at) memcpy(row, st.sess[i]->remained.data(), at * 4);
        for (int k : st.feeds_of[i]) {
            const long m = st.feed_n[k];
            if (st.feed_rate_slot && st.feed_rate_slot[k] >= 0) {      // staged raw; its samples are a hole the device fills
                raw_at = (raw_at + 3) & ~(size_t)3;
                const size_t bytes = (size_t)m * (st.feed_format[k] ? 4 : 2);
                memcpy(st.raw_h + raw_at, st.feed_samples[k], bytes);
                st.rs_feeds.push_back(masr_resample_feed{(int64_t)raw_at, st.feed_format[k], (int32_t)m, (int32_t)st.out_n[k], i,
                                                         (int32_t)at, st.feed_rate_slot[k]});
                raw_at += bytes;
                at += (size_t)st.out_n[k];
                continue;
            }
            if (st.feed_format[k] == 1) {
                memcpy(row + at, st.feed_samples[k], (size_t)m * 4);
            } else {                                  // int16 PCM: x / 2^15 in float32 (buf_to_float, data_utils/utils.py:382-411)
                const int16_t* src = (const int16_t*)st.feed_samples[k];
                for (long j = 0; j < m; ++j) row[at + j] = (float)src[j] * (1.0f / 32768.0f);
            }
            at += (size_t)m;
        }
        if ((long)at < n_max) memset(row + at, 0, (size_t)(n_max - (long)at) * 4);
        st.lens_h[i] = (int32_t)st.len[i];
    }
    return 0;
}

// ONE upload of the rows; off-rate feeds: ONE launch fills their holes, and the tails of their sessions come back behind it
int upload_and_resample(masr_pool* p, Step& st, hipStream_t s) {
    const int n = st.n;
    const long n_max = st.n_max;
    PCHK(upload(p, p->samples, st.buf, (size_t)n * n_max * 4, s));
    PCHK(upload(p, p->lens, st.lens_h, (size_t)n * 4, s));
    st.fresh.resize(n);
    for (int i = 0; i < n; ++i) st.fresh[i] = pool_feature_frames(st.len[i], p->min_samples);
    st.tail_h.assign(n, nullptr);
    if (st.rs_feeds.empty()) return 0;
    const int nf = (int)st.rs_feeds.size();
    int64_t n_tiles = 0;                           // (what the plan will count: one tile per 256 outputs of a feed)
    for (const masr_resample_feed& f : st.rs_feeds) n_tiles += (f.n_out + MASR_RESAMPLE_TILE - 1) / MASR_RESAMPLE_TILE;
    int32_t bad = -1;
    const char* why = nullptr;
    std::vector<PoolSeg> tsegs;
    long tail_total = 0;
    int tail_max = 0;
    for (int i = 0; i < n; ++i)
        if (st.off_sess[i]) {
            const long from = 160L * st.fresh[i], len = st.len[i] - from;
            if (len > 0) {
                tsegs.push_back(PoolSeg{(long)i * n_max + from, tail_total, (int)len, i});
                tail_max = std::max(tail_max, (int)len);
            }
            tail_total += len;
        }
    // block: feeds | tiles | tail segments (descriptors; the raw bytes are their own copy: they may be large)
    const size_t o_tiles = (size_t)nf * sizeof(masr_resample_feed), o_segs = o_tiles + (size_t)n_tiles * 8;
    const size_t block = o_segs + tsegs.size() * sizeof(PoolSeg);
    char* blk = nullptr;
    PCHK(p->pin.take(block, (void**)&blk));
    memcpy(blk, st.rs_feeds.data(), o_tiles);
    int64_t planned = 0;
    if (masr_resample_plan(st.rs_feeds.data(), nf, p->rates.data(), (int)p->rates.size(), (int64_t)st.raw_bytes, n, n_max,
                           (int32_t*)(blk + o_tiles), n_tiles, &planned, &bad, &why) || planned != n_tiles)
        PFAIL(std::string("masr_pool_step: off-rate feed: ") + (why ? why : "tile count"));
    float* tails_h = nullptr;
    if (tail_total) PCHK(p->pin.take((size_t)tail_total * 4, (void**)&tails_h));
    for (PoolSeg& g : tsegs) {
        st.tail_h[g.pad_] = tails_h + g.dst;
        g.pad_ = 0;
    }
    if (!tsegs.empty()) memcpy(blk + o_segs, tsegs.data(), tsegs.size() * sizeof(PoolSeg));
    const size_t dev_raw = (st.raw_bytes + 63) & ~(size_t)63;
    PCHK(p->raw.ensure(dev_raw + block, 0, s));
    char* raw_d = p->raw.as<char>();
    PHIP(hipMemcpyAsync(raw_d, st.raw_h, st.raw_bytes, hipMemcpyHostToDevice, s));
    PHIP(hipMemcpyAsync(raw_d + dev_raw, blk, block, hipMemcpyHostToDevice, s));
    PCHK(masr_resample_feeds(p->e, raw_d, (int64_t)st.raw_bytes, st.rs_feeds.data(), (const masr_resample_feed*)(raw_d + dev_raw), nf,
                             p->rates.data(), p->rates_dev, (int)p->rates.size(), (const int32_t*)(blk + o_tiles),
                             (const int32_t*)(raw_d + dev_raw + o_tiles), n_tiles, p->samples.as<float>(), n, n_max, s));
    if (tail_total) {
        PCHK(p->tails_dev.ensure((size_t)tail_total * 4, 0, s));
        launch_copy_segments(p->samples.as<float>(), p->tails_dev.as<float>(), nullptr, nullptr,
                             (const PoolSeg*)(raw_d + dev_raw + o_segs), (int)tsegs.size(), tail_max, 1, s);
        PHIP(hipMemcpyAsync(tails_h, p->tails_dev.p, (size_t)tail_total * 4, hipMemcpyDeviceToHost, s));
    }
    return 0;
}

// gains: mean squares from the device, the scalar expressions of AudioSegment.normalize on the host
int gains(masr_pool* p, Step& st, hipStream_t s) {
    if (!p->use_db) return 0;
    const int n = st.n;
    float* ms_h = nullptr;
    PCHK(p->pin.take((size_t)n * 4, (void**)&ms_h));
    PCHK(p->pin.take((size_t)n * 4, (void**)&st.gains_h));
    PCHK(p->ms.ensure((size_t)n * 4, 0, s));
    PCHK(masr_mean_square(p->e, p->samples.p, 1, p->lens.as<int32_t>(), n, (int32_t)st.n_max, p->ms.as<float>(), s));
    PHIP(hipMemcpyAsync(ms_h, p->ms.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    PHIP(hipStreamSynchronize(s));
    st.lap(p, 1);
    if (st.gain_fn) {
        if (st.gain_fn(ms_h, n, p->target_db, st.gains_h, st.gain_user)) PFAIL("masr_pool_step: the gain evaluator failed");
    } else {                                       // libm evaluation of audio.py:287-304,519-529 (float32 steps)
        for (int i = 0; i < n; ++i) {
            const float m = ms_h[i] == 0.f ? 1.f : ms_h[i];
            const float gain_db = p->target_db - 10.f * log10f(m);
            if (gain_db > 300.f) PFAIL("masr_pool_step: gain beyond max_gain_db (300 dB)");
            st.gains_h[i] = powf(10.f, gain_db / 20.f);
        }
    }
    PCHK(upload(p, p->gains, st.gains_h, (size_t)n * 4, s));
    st.lap(p, 2);
    return 0;
}

// ONE ragged feature launch over the pending samples, by the pool's feature method
int features(masr_pool* p, Step& st, hipStream_t s) {
    const int n = st.n, mode = p->use_db ? 2 : 0;
    const int32_t n_max = (int32_t)st.n_max;
    st.tmax = p->method == 2 ? (int)((st.n_max - 320) / 160 + 1) : (int)(1 + (st.n_max - 400) / 160);
    PCHK(p->feats.ensure((size_t)n * st.tmax * p->F * 4, 0, s));
    if (p->method == 0)
        return masr_fbank_batch(p->e, p->samples.p, 1, p->lens.as<int32_t>(), n, n_max, mode, p->target_db, p->feats.as<float>(), nullptr,
                                nullptr, p->gains.as<float>(), s);
    if (p->method == 1)
        return masr_mfcc_batch(p->e, p->samples.p, 1, p->lens.as<int32_t>(), n, n_max, mode, p->target_db, p->n_mfcc, p->feats.as<float>(),
                               nullptr, p->gains.as<float>(), s);
    return masr_linear_batch(p->e, p->samples.p, 1, p->lens.as<int32_t>(), n, n_max, mode, p->target_db, p->feats.as<float>(), nullptr,
                             p->gains.as<float>(), s);
}

// one table of the step's segments: copied into its slice of the pinned and of the device array, *dev = the device slice
int push_segments(masr_pool* p, Step& st, const std::vector<PoolSeg>& v, const PoolSeg** dev, hipStream_t s) {
    memcpy(st.seg_pin + st.seg_at, v.data(), v.size() * sizeof(PoolSeg));
    PHIP(hipMemcpyAsync(p->segs.as<PoolSeg>() + st.seg_at, st.seg_pin + st.seg_at, v.size() * sizeof(PoolSeg), hipMemcpyHostToDevice, s));
    *dev = p->segs.as<PoolSeg>() + st.seg_at;
    st.seg_at += v.size();
    return 0;
}

// bookkeeping: carried-over samples, new frames appended to the sessions' rows of the frame pool; the windows of every session
// (predict.py:283-306) are planned here, where the segment tables of the whole step are sized
int append_frames(masr_pool* p, Step& st, hipStream_t s) {
    const int n = st.n;
    int need = 0;
    for (int i = 0; i < n; ++i) need = std::max(need, st.sess[i]->nf + st.fresh[i]);
    if (need > p->feat_cap) PCHK(widen_feat(p, std::max(need, 2 * p->feat_cap), s));
    std::vector<PoolSeg> seg_h;
    int seg_rows = 0;
    for (int i = 0; i < n; ++i) {
        Session& q = *st.sess[i];
        const float* row = st.buf + (size_t)i * st.n_max;
        const long from = 160L * st.fresh[i], len = st.len[i];
        if (st.off_sess[i]) {                                         // the device has the row: its tail is on its way back
            q.remained.assign((size_t)(len - from), 0.f);
            p->tails.push_back(Tail{q.sid, st.tail_h[i], (size_t)(len - from), p->use_db ? st.gains_h[i] : 1.f, p->use_db && len > 0});
        } else {
            q.remained.assign(row + from, row + len);                // normalised in place, like AudioSegment.normalize
            if (p->use_db && len > 0)
                for (float& v : q.remained) v *= st.gains_h[i];
        }
        if (q.f0 + q.nf + st.fresh[i] > p->feat_cap) {                // make room: the live frames move to the front of the row
            float* base = p->feat.as<float>() + (size_t)q.row * p->feat_cap * p->F;
            PCHK(p->win.ensure((size_t)q.nf * p->F * 4, 0, s));
            PHIP(hipMemcpyAsync(p->win.p, base + (size_t)q.f0 * p->F, (size_t)q.nf * p->F * 4, hipMemcpyDeviceToDevice, s));
            PHIP(hipMemcpyAsync(base, p->win.p, (size_t)q.nf * p->F * 4, hipMemcpyDeviceToDevice, s));
            q.f0 = 0;
        }
        if (st.fresh[i]) {
            seg_h.push_back(PoolSeg{(long)i * st.tmax, (long)q.row * p->feat_cap + q.f0 + q.nf, st.fresh[i], 0});
            seg_rows = std::max(seg_rows, st.fresh[i]);
        }
        q.nf += st.fresh[i];
    }
    size_t seg_total = seg_h.size();
    st.plans.resize(n);
    for (int i = 0; i < n; ++i) {
        pool_windows(st.sess[i]->nf, st.end_flag[i] != 0, [&](int first, int last) { st.plans[i].push_back({first, last}); });
        st.lockstep = std::max(st.lockstep, st.plans[i].size());
        seg_total += 2 * st.plans[i].size();
    }
    PCHK(p->segs.ensure((seg_total + 8) * sizeof(PoolSeg), 0, s));
    PCHK(p->pin.take((seg_total + 8) * sizeof(PoolSeg), (void**)&st.seg_pin));
    if (!seg_h.empty()) {
        const PoolSeg* d = nullptr;
        PCHK(push_segments(p, st, seg_h, &d, s));
        launch_copy_segments(p->feats.as<float>(), p->feat.as<float>(), nullptr, nullptr, d, (int)seg_h.size(), seg_rows, p->F, s);
    }
    return 0;
}

// window k of the sessions whose window k is `len` frames long: gathered from the frame pool, advanced through masr_encode_chunk,
// (argmax, max prob) appended to the histories
int run_window_group(masr_pool* p, Step& st, size_t k, int len, std::vector<int32_t>& ids, hipStream_t s) {
    const int n = st.n;
    auto in_group = [&](int i) { return k < st.plans[i].size() && st.plans[i][k].second - st.plans[i][k].first == len; };
    std::vector<PoolSeg> gat, sca;
    ids.clear();
    int32_t tq = 0;
    PCHK(masr_encoder_frames(p->e, len, &tq));
    int hist_need = 0;
    for (int i = 0; i < n; ++i) {
        if (!in_group(i)) continue;
        Session& q = *st.sess[i];
        const long item = (long)ids.size();
        gat.push_back(PoolSeg{(long)q.row * p->feat_cap + q.f0 + st.plans[i][k].first, item * len, len, 0});
        sca.push_back(PoolSeg{item * tq, 0, tq, i});            // dst filled in once the history width is final
        hist_need = std::max(hist_need, q.frames + tq);
        ids.push_back(q.sid);
    }
    const int m = (int)ids.size();
    PCHK(grow_state(p, 0, hist_need, s));
    for (PoolSeg& g : sca) {
        Session& q = *st.sess[g.pad_];
        g.dst = (long)q.row * p->hist_cap + q.frames;
        g.pad_ = 0;
    }
    PCHK(p->win.ensure((size_t)m * len * p->F * 4, 0, s));
    PCHK(p->idx.ensure((size_t)m * std::max(tq, 1) * 4, 0, s));
    PCHK(p->mp.ensure((size_t)m * std::max(tq, 1) * 4, 0, s));
    const PoolSeg *dg = nullptr, *ds = nullptr;
    PCHK(push_segments(p, st, gat, &dg, s));
    launch_copy_segments(p->feat.as<float>(), p->win.as<float>(), nullptr, nullptr, dg, m, len, p->F, s);
    // (a last window shorter than the front-end's minimum -- 8-14 frames under conv2d8, 7-10 under conv2d6 -- gives no
    // encoder frame: nothing to run, where the reference's conv would refuse the input)
    if (tq > 0) {
        PCHK(masr_encode_chunk(p->e, ids.data(), m, p->win.as<float>(), len, nullptr, p->idx.as<int32_t>(), p->mp.as<float>(), s));
        PCHK(push_segments(p, st, sca, &ds, s));
        launch_copy_segments(reinterpret_cast<const float*>(p->idx.p), p->hist_idx.as<float>(), p->mp.as<float>(),
                             p->hist_mp.as<float>(), ds, m, tq, 1, s);
    }
    for (int i = 0; i < n; ++i)
        if (in_group(i)) st.sess[i]->frames += tq;
    return 0;
}

// the windows of all sessions, advanced in lock-step
int run_windows(masr_pool* p, Step& st, hipStream_t s) {
    std::vector<int32_t> ids;
    for (size_t k = 0; k < st.lockstep; ++k) {
        // full windows together; a short last window on its own (lengths in ascending order of first appearance)
        std::vector<int> lengths;
        for (int i = 0; i < st.n; ++i)
            if (k < st.plans[i].size()) {
                const int len = st.plans[i][k].second - st.plans[i][k].first;
                if (std::find(lengths.begin(), lengths.end(), len) == lengths.end()) lengths.push_back(len);
            }
        for (int len : lengths) PCHK(run_window_group(p, st, k, len, ids, s));
    }
    return 0;
}

// greedy: ONE collapse launch for every session that advanced (full-history best path + score, greedy_decoder_chunk semantics,
// ctc_greedy_decoder.py:52-89); ONE copy back
int collapse_and_fetch(masr_pool* p, Step& st, hipStream_t s) {
    std::vector<int> adv;
    int hmax = 0;
    for (int i = 0; i < st.n; ++i)
        if (!st.plans[i].empty()) {
            adv.push_back(i);
            hmax = std::max(hmax, st.sess[i]->frames);
        }
    const int na = st.na = (int)adv.size(), width = st.width = hmax + 2;
    // the collapse takes the longest history as its Tp: a Conformer-family session stops at its stream's max_frames_out <= max_pos
    // (5000 unless the engine was created with more), a DeepSpeech2 session has no frame limit -- the same refusal as
    // masr_ctc_collapse, by name, instead of a launch that asks for more dynamic LDS than the kernel may have
    if (hmax > CTC_COLLAPSE_MAX_FRAMES) PFAIL(std::string("masr_pool_step: ") + ctc_collapse_refusal);
    if (na) {
        int32_t* meta_h = nullptr;                 // [rows | frame counts]
        PCHK(p->pin.take((size_t)2 * na * 4, (void**)&meta_h));
        for (int j = 0; j < na; ++j) {
            meta_h[j] = st.sess[adv[j]]->row;
            meta_h[na + j] = st.sess[adv[j]]->frames;
        }
        PCHK(upload(p, p->meta, meta_h, (size_t)2 * na * 4, s));
        PCHK(p->rows_out.ensure((size_t)na * width * 4, 0, s));
        launch_ctc_collapse_hist(p->hist_idx.as<int>(), p->hist_mp.as<float>(), p->meta.as<int>() + na, p->meta.as<int>(), p->hist_cap,
                                 na, hmax, 0, p->rows_out.as<int>(), s);
        PCHK(p->pin.take((size_t)na * width * 4, (void**)&st.rows_h));
        PHIP(hipMemcpyAsync(st.rows_h, p->rows_out.p, (size_t)na * width * 4, hipMemcpyDeviceToHost, s));
    }
    PHIP(hipGetLastError());
    PHIP(hipEventRecord(p->ev, s));
    p->pending = true;
    if (na) PHIP(hipStreamSynchronize(s));
    if (na || p->use_db) settle_tails(p);            // (waited for above, or with the mean squares; else: at the next step)
    return 0;
}

// results + the windows' bookkeeping (predict.py:329: keep the overlap frames); the sessions left out follow with state -1
void publish(masr_pool* p, Step& st) {
    for (int i = 0; i < st.n; ++i) {
        Session& q = *st.sess[i];
        if (!st.plans[i].empty()) {
            const int used = st.plans[i].back().second - kOverlap;
            q.f0 += used;
            q.nf -= used;
        }
        p->handles.push_back(q.sid);
        p->state.push_back(st.plans[i].empty() ? 0 : 1);
    }
    for (int32_t h : st.refused) {
        p->handles.push_back(h);
        p->state.push_back(-1);
    }
    *st.n_sessions = st.n + (int32_t)st.refused.size();
    if (st.handles_out) *st.handles_out = p->handles.data();
    if (st.state_out) *st.state_out = p->state.data();
    if (st.rows_host) *st.rows_host = st.rows_h;
    if (st.row_width) *st.row_width = st.na ? st.width : 0;
    if (st.rows_dev) *st.rows_dev = st.na ? p->rows_out.as<int32_t>() : nullptr;
}

}  // namespace

extern "C" {

int masr_pool_create(masr_engine* e, int32_t feature_method, int32_t n_mfcc, int32_t use_db_normalization, float target_db,
                     int32_t max_frames_out, masr_pool** out) {
    if (!e || !out) PFAIL("null argument");
    if (feature_method < 0 || feature_method > 2) PFAIL("feature_method: 0 = fbank, 1 = mfcc, 2 = linear");
    masr_pool* p = new masr_pool();
    p->e = e;
    int32_t dev = 0, n_mels = 80;
    if (masr_engine_info(e, &dev, &n_mels, nullptr)) {
        delete p;
        return 1;
    }
    p->device = dev;
    p->method = feature_method;
    p->n_mfcc = n_mfcc;
    p->use_db = use_db_normalization ? 1 : 0;
    p->target_db = target_db;
    p->max_frames_out = max_frames_out;
    p->F = feature_method == 2 ? 161 : feature_method == 1 ? n_mfcc : 80;
    p->min_samples = feature_method == 2 ? 320 : 400;
    *out = p;
    return 0;
}

void masr_pool_destroy(masr_pool* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();
    for (auto& kv : p->sessions) (void)masr_stream_close(p->e, kv.second.sid);
    for (Dev* d : p->buffers()) d->release();
    for (void* t : p->rate_tables) (void)hipFree(t);
    if (p->rates_dev) (void)hipFree(p->rates_dev);
    p->pin.release();
    if (p->ev) (void)hipEventDestroy(p->ev);
    delete p;
}

int masr_pool_open(masr_pool* p, int32_t* handle) {
    if (!p || !handle) PFAIL("null argument");
    int32_t sid = -1;
    PCHK(masr_stream_open(p->e, p->max_frames_out, &sid));
    Session s;
    s.sid = sid;
    if (!p->free_rows.empty()) {
        s.row = p->free_rows.back();
        p->free_rows.pop_back();
    } else {
        s.row = p->n_rows++;
    }
    p->sessions[sid] = std::move(s);
    *handle = sid;
    return 0;
}

int masr_pool_close(masr_pool* p, int32_t handle) {
    if (!p) PFAIL("null pool");
    auto it = p->sessions.find(handle);
    if (it == p->sessions.end()) PFAIL("masr_pool_close: unknown handle");
    PCHK(masr_stream_close(p->e, handle));
    drop_tails(p, handle);
    p->free_rows.push_back(it->second.row);
    p->sessions.erase(it);
    return 0;
}

int masr_pool_reset(masr_pool* p, int32_t handle) {
    if (!p) PFAIL("null pool");
    auto it = p->sessions.find(handle);
    if (it == p->sessions.end()) PFAIL("masr_pool_reset: unknown handle");
    PCHK(masr_stream_reset(p->e, handle));
    Session& s = it->second;
    drop_tails(p, handle);
    s.remained.clear();
    s.f0 = s.nf = s.frames = 0;
    return 0;
}

int masr_pool_set_rate(masr_pool* p, int32_t sr_orig, double ratio, const double* table_host, int64_t nwin, int32_t num_table,
                       int32_t* slot) {
    if (!p || !slot || !table_host) PFAIL("masr_pool_set_rate: null argument");
    if (sr_orig <= 0) PFAIL("masr_pool_set_rate: Invalid sample rate");
    auto it = p->rate_of.find(sr_orig);
    if (it != p->rate_of.end()) {
        *slot = it->second;
        return 0;
    }
    if ((int)p->rates.size() >= kMaxRates) PFAIL("masr_pool_set_rate: at most 64 source rates per pool");
    if (!(ratio > 0.0) || nwin <= 0 || nwin > (1 << 30) || num_table <= 0) PFAIL("masr_pool_set_rate: ratio must be positive, with a filter table");
    PHIP(hipSetDevice(p->device));
    void* table = nullptr;
    PHIP(hipMalloc(&table, (size_t)nwin * 16));
    masr_resample_rate r;
    if (masr_resample_rate_fill(ratio, (const double*)table, nwin, num_table, &r)) {
        (void)hipFree(table);
        PFAIL("masr_pool_set_rate: index_step <= 0 (ratio too small for the table)");
    }
    if (!p->rates_dev) {
        const hipError_t err = hipMalloc((void**)&p->rates_dev, kMaxRates * sizeof(masr_resample_rate));
        if (err != hipSuccess) {
            (void)hipFree(table);
            PFAIL(std::string("masr_pool_set_rate: hipMalloc: ") + hipGetErrorString(err));
        }
    }
    // (synchronous copies: a registration, not a step; the slot is new, so no launch in flight reads it)
    hipError_t err = hipMemcpy(table, table_host, (size_t)nwin * 16, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(p->rates_dev + p->rates.size(), &r, sizeof(r), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        (void)hipFree(table);
        PFAIL(std::string("masr_pool_set_rate: hipMemcpy: ") + hipGetErrorString(err));
    }
    p->rate_tables.push_back(table);
    p->rates.push_back(r);
    *slot = p->rate_of[sr_orig] = (int)p->rates.size() - 1;
    return 0;
}

int masr_pool_step(masr_pool* p, int32_t n_feeds, const int32_t* feed_handle, const void* const* feed_samples,
                   const int64_t* feed_n, const int32_t* feed_format, const int32_t* feed_is_end, masr_gain_fn gain_fn,
                   void* gain_user, int32_t* n_sessions, const int32_t** handles_out, const int32_t** state_out,
                   const int32_t** rows_host, int32_t* row_width, int32_t** rows_dev, void* stream) {
    return masr_pool_step_rates(p, n_feeds, feed_handle, feed_samples, feed_n, feed_format, feed_is_end, nullptr, gain_fn, gain_user,
                                n_sessions, handles_out, state_out, rows_host, row_width, rows_dev, stream);
}

int masr_pool_step_rates(masr_pool* p, int32_t n_feeds, const int32_t* feed_handle, const void* const* feed_samples,
                         const int64_t* feed_n, const int32_t* feed_format, const int32_t* feed_is_end,
                         const int32_t* feed_rate_slot, masr_gain_fn gain_fn, void* gain_user, int32_t* n_sessions,
                         const int32_t** handles_out, const int32_t** state_out, const int32_t** rows_host, int32_t* row_width,
                         int32_t** rows_dev, void* stream) {
    if (!p || !n_sessions) PFAIL("null argument");
    PHIP(hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)stream;
    *n_sessions = 0;
    if (row_width) *row_width = 0;
    if (rows_host) *rows_host = nullptr;
    if (rows_dev) *rows_dev = nullptr;
    p->handles.clear();
    p->state.clear();
    if (n_feeds <= 0) return 0;
    Step st{n_feeds, feed_handle, feed_samples, feed_n, feed_format, feed_is_end, feed_rate_slot, gain_fn, gain_user,
            n_sessions, handles_out, state_out, rows_host, row_width, rows_dev};
    PCHK(check_feeds(p, st));                        // (these three commit nothing: a refused call leaves the pool as it was)
    group_by_session(p, st);
    PCHK(admit(p, st));
    if (st.sess.empty()) {                           // every session was left out
        publish(p, st);
        return 0;
    }
    st.t_last = std::chrono::steady_clock::now();
    PCHK(begin_step(p, st, s));
    PCHK(assemble_rows(p, st));
    st.lap(p, 0);
    PCHK(upload_and_resample(p, st, s));
    PCHK(gains(p, st, s));                           // (laps 1 and 2: behind its wait, behind its upload)
    PCHK(features(p, st, s));
    TailGuard tail_guard{p, s};                      // append_frames queues the tails; any error return from here on settles them
    PCHK(append_frames(p, st, s));
    st.lap(p, 3);
    PCHK(run_windows(p, st, s));
    st.lap(p, 4);
    PCHK(collapse_and_fetch(p, st, s));
    tail_guard.done = true;
    st.lap(p, 5);
    ++p->prof_steps;
    publish(p, st);
    return 0;
}

int masr_pool_window_plan(int32_t n_frames, int32_t is_end, int32_t* first_last, int32_t cap, int32_t* n_windows) {
    if (!n_windows || (cap > 0 && !first_last)) PFAIL("masr_pool_window_plan: null argument");
    if (n_frames > (1 << 30)) PFAIL("masr_pool_window_plan: n_frames out of range (at most 2^30)");
    int32_t n = 0;
    pool_windows(n_frames, is_end != 0, [&](int first, int last) {
        if (n < cap) {
            first_last[2 * n] = first;
            first_last[2 * n + 1] = last;
        }
        ++n;
    });
    *n_windows = n;
    return 0;
}

int masr_pool_profile(masr_pool* p, double* phase_ms, int64_t* steps, int32_t reset) {
    if (!p || !phase_ms || !steps) PFAIL("null argument");
    for (int k = 0; k < 6; ++k) phase_ms[k] = p->prof[k];
    *steps = p->prof_steps;
    if (reset) {
        for (double& v : p->prof) v = 0;
        p->prof_steps = 0;
    }
    return 0;
}

}  // extern "C"
