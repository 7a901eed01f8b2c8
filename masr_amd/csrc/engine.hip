// libmasr_hip.so -- engine: weight store, workspace, orchestration of the Conformer hot path and
// the C ABI declared in include/masr_hip.h.  Host-side only; every kernel lives in the sibling
// .hip files and is launched on the caller's stream.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "engine_state.h"

using namespace masr;

static thread_local std::string g_err;
namespace masr {
int engine_fail(const std::string& m) {      // fail() of engine_state.h; pool.hip reports through the same masr_last_error()
    g_err = m;
    return 1;
}
}

// errors noted by the kernel launchers (a refused dynamic-LDS opt-in, ...) since the last check on this thread
static thread_local std::string g_launch_err;
namespace masr {
void note_launch_error(const char* what, hipError_t e) {
    if (g_launch_err.empty()) g_launch_err = std::string(what) + ": " + hipGetErrorString(e);
}
bool launch_error_pending() { return !g_launch_err.empty(); }
std::string take_launch_error() {
    std::string m;
    m.swap(g_launch_err);
    return m;
}
void ensure_dynamic_lds(const void* fn, size_t bytes, LdsAttr& st) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) dev = 0;
    if (bytes <= st.granted[dev]) return;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        note_launch_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
        return;
    }
    st.granted[dev] = bytes;
}
}  // namespace masr

// hipMemset runs on the NULL stream, which a non-blocking stream (every torch side stream, the library's own) does not wait for:
// the host waits for the fill, so that whatever is launched next on any stream sees the cleared memory
static int clear_sync(void* p, int value, size_t n) {
    HIPCHK(hipMemset(p, value, n));
    HIPCHK(hipStreamSynchronize(nullptr));
    return 0;
}

namespace masr {
int get(masr_engine* e, const std::string& name, std::vector<int64_t> shape, const HostTensor** out) {
    auto it = e->host.find(name);
    if (it == e->host.end()) return fail("missing tensor: " + name);
    int64_t want = 1, have = 1;
    for (auto s : shape) want *= s;
    for (auto s : it->second.shape) have *= s;
    if (want != have)
        return fail("tensor " + name + ": expected " + std::to_string(want) + " elements, got " + std::to_string(have));
    *out = &it->second;
    return 0;
}

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
}  // namespace masr

namespace {

int up(masr_engine* e, const std::string& name, std::vector<int64_t> shape, float** out) {
    const HostTensor* t;
    CHK(get(e, name, shape, &t));
    return upload(e, t->v, out);
}

// The packed copy of `src` in `layout`, built on first use and kept: buffers of bytes_a (and bytes_b, 0 = none), filled by
// pack(copy, s), which issues the packing launch on the caller's stream.  nullptr = an allocation failed (masr_last_error says
// which): what was allocated is freed and nothing is cached.
template <class Pack>
const PackedW* packed_of(masr_engine* e, PackLayout layout, const float* src, size_t bytes_a, size_t bytes_b, hipStream_t s,
                         Pack&& pack) {
    const std::pair<int, const float*> key(layout, src);
    auto it = e->packed.find(key);
    if (it == e->packed.end()) {
        PackedW pk;
        if (pk.a.ensure(bytes_a) || pk.b.ensure(bytes_b)) {
            pk.release();
            return nullptr;
        }
        pack(pk, s);
        it = e->packed.emplace(key, pk).first;
    }
    return &it->second;
}

// fragment-ordered copy of a [N, 256] weight matrix (rows padded to a multiple of 256 with zeros): launch_pack_rows_pc's order,
// or launch_pack_rows16's (PACK_ROWS16)
const float* packed_rows_of(masr_engine* e, const float* W, int N, hipStream_t s, PackLayout layout = PACK_ROWS_PC) {
    const int Np = (N + 255) / 256 * 256;
    const PackedW* pk = packed_of(e, layout, W, (size_t)Np * 256 * sizeof(float), 0, s, [&](const PackedW& p, hipStream_t st) {
        (layout == PACK_ROWS16 ? launch_pack_rows16 : launch_pack_rows_pc)(W, p.a.as<float>(), Np, st, N);
    });
    return pk ? pk->a.as<float>() : nullptr;
}

// fragment-order copies of an FFN's two weight matrices, cached per W1 pointer: ffn_pc.hip's layout (PACK_FFN_PC,
// launch_pack_ffn_pc), the 16-row kernel's (PACK_FFN16, launch_pack_ffn16) or the two-chain kernel's (PACK_FFN_DUAL, launch_pack_ffn_dual)
typedef void (*PackFfnFn)(const float*, const float*, float*, float*, int, hipStream_t);
int packed_ffn_of(masr_engine* e, const float* w1, const float* w2, hipStream_t s, const float** p1, const float** p2,
                  PackLayout layout = PACK_FFN_PC, PackFfnFn pack = launch_pack_ffn_pc) {
    const size_t bytes = (size_t)e->cfg.d_ff * e->cfg.d_model * sizeof(float);
    const PackedW* pk = packed_of(e, layout, w1, bytes, bytes, s, [&](const PackedW& p, hipStream_t st) {
        pack(w1, w2, p.a.as<float>(), p.b.as<float>(), e->cfg.d_ff, st);
    });
    if (!pk) return 1;
    *p1 = pk->a.as<float>();
    *p2 = pk->b.as<float>();
    return 0;
}
// the fused Squeezeformer stages cover these sizes (launch_sqz_stage's own checks, sqz_layer.hip): anything else takes the separate launches
static bool sqz_stage_supported(const masr_engine* e) {
    const int K = e->cfg.cnn_kernel;
    return e->cfg.d_model == 256 && e->cfg.d_ff % 128 == 0 && e->cfg.d_ff >= 256 && (K == 31 || K == 15);
}

// the common prefix of a row-block launch, C[M, N] = A[M, 256] . W[N, 256]^T + bias, with the defaults every launch but the odd one
// takes (alpha 1, LayerNorm eps 1e-5, 4 feature frames per encoder frame in the pad masks); the rest is filled in by field name
RowGemmArgs rg_args(const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int M, int N) {
    RowGemmArgs a{};
    a.A = A; a.lda = lda; a.W = W; a.bias = bias; a.C = C; a.ldc = ldc; a.M = M; a.N = N;
    a.alpha = 1.f; a.eps = 1e-5f; a.mstride = 4;
    return a;
}
void rowgemm(masr_engine* e, hipStream_t s, int pro, int epi, RowGemmArgs a, int kind = PROF_GEMM) {
    // full row-block launches (the K-split kernel of few row blocks reads W itself) take the packed copy of their weights
    if (knobs().rowgemm_packed && a.M >= 112 * 32 && pro != RG_PRO_HIST && pro != RG_PRO_DWCONV && (epi == RG_EPI_CTC || a.N % 256 == 0))
        a.Wp = packed_rows_of(e, a.W, a.N, s);
    ProfScope ps(e, s, kind, 2.0 * a.M * (double)a.N * 256);
    launch_rowgemm(a, pro, epi, s);
}

}  // namespace

namespace {
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
}  // namespace

// ---- side streams (masr_side_stream) ------------------------------------------------------------------------------------------
// The library owns the streams its callers run beside the main stream: two for the prefix searches of consecutive passes, one for
// the per-pass preparation, one for copies.  ONE SET PER DEVICE, created with the FIRST engine on that device -- a fixed, early place
// in the process's history -- and shared by every engine there; non-blocking, default priority.  Rounds 3-5 borrowed
// torch.cuda.Stream()s created wherever a predictor first needed one: the HIP runtime deals streams onto a small pool of hardware
// queues (GPU_MAX_HW_QUEUES, default 4) at creation, and in a process that had already created its share a search stream landed on
// the main stream's queue and ran BEHIND the next encoder pass (BASELINE configs[2]: 63 vs 46 ms per call by process history,
// repaired then by raising GPU_MAX_HW_QUEUES from masr_amd/__init__.py).  Creating them early (the first half of round 6) only moved
// the dependence: the runtime deals queues round-robin in creation order, whatever was created BEFORE the first engine shifts the
// deal -- after torch.distributed had initialised RCCL (one stream) search stream 0 and the second lane's stream shared the
// NULL stream's queue (configs[2] sharpened 30.0 instead of 23.2 ms per call), and in a cold process the preparation stream did
// (every upload of a pass issued beside a running encoder started 4 - 6 ms late).  So the set is CHOSEN BY PROBING: candidate
// streams are created until three hardware queues other than the NULL stream's have been seen (two streams share a queue when an
// empty kernel on one waits for a spinning kernel on the other; ~0.3 ms per probe, at most 16 candidates, once per device):
//   queue B: search stream 0 and the second lane (never used together)     queue C: search stream 1
//   queue D: preparation and copies (short work only)                      the NULL stream's queue: nobody
// With fewer queues than that (GPU_MAX_HW_QUEUES < 4) the roles double up in that order.  MASR_SIDE_DEBUG=1 prints the choice.
// Measured and rejected (round 6, configs[2] sharpened head, passes of 32, ms per call): highest priority 28.9, lowest 28.8,
// default 24.0 -- a queue of another priority class has a hardware-queue pool of its own (never aliased), but every launch beside
// it pays for it (the same call WITHOUT its search kernels: 22.3 against 19.7 ms).  MASR_SIDE_PRIORITY=high|low for the A/B.
// hipExtStreamCreateWithCUMask (a dedicated queue and a CU reservation) can only create streams that synchronise with the NULL
// stream, which is torch's default stream: every search would serialise with the encoder it is meant to run beside.
struct SideStreams {
    hipStream_t s[MASR_SIDE_STREAMS] = {};
    bool made = false;
};
static std::mutex g_side_mu;
static std::map<int, SideStreams> g_side;
static int side_streams_of(int dev, SideStreams** out) {
    std::lock_guard<std::mutex> lk(g_side_mu);
    SideStreams& ss = g_side[dev];
    if (!ss.made) {
        int least = 0, greatest = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        const char* pe = getenv("MASR_SIDE_PRIORITY");          // A/B only
        const int prio = (pe && pe[0] == 'h') ? greatest : (pe && pe[0] == 'l') ? least : 0;
        if (pe) fprintf(stderr, "masr side streams: priority %d (device range: least %d .. greatest %d)\n", prio, least, greatest);
        // true when an empty kernel on `b` waits for a kernel that spins on `a`: the two streams share a hardware queue
        auto aliased = [](hipStream_t a, hipStream_t b, hipEvent_t ea, hipEvent_t eb, bool* out) -> int {
            launch_queue_spin(30000, a);                       // 300 us
            HIPCHK(hipEventRecord(ea, a));
            launch_queue_nop(b);
            HIPCHK(hipEventRecord(eb, b));
            HIPCHK(hipEventSynchronize(eb));
            *out = hipEventQuery(ea) == hipSuccess;            // the spin was over before the empty kernel got through
            (void)hipGetLastError();
            HIPCHK(hipEventSynchronize(ea));
            return 0;
        };
        hipEvent_t ea = nullptr, eb = nullptr;
        HIPCHK(hipEventCreateWithFlags(&ea, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&eb, hipEventDisableTiming));
        HIPCHK(hipDeviceSynchronize());
        std::vector<hipStream_t> cls;                          // one stream per hardware queue seen so far (not the NULL stream's)
        std::vector<hipStream_t> spare;                        // candidates on a queue already represented (kept: destroying a
        const bool dbg = getenv("MASR_SIDE_DEBUG") != nullptr; // stream would hand its slot of the deal to the next one created)
        for (int c = 0; c < 16 && cls.size() < 3; ++c) {
            hipStream_t st = nullptr;
            HIPCHK(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio));
            bool same = false;
            if (aliased(nullptr, st, ea, eb, &same)) return 1;
            for (size_t k = 0; k < cls.size() && !same; ++k)
                if (aliased(cls[k], st, ea, eb, &same)) return 1;
            (same ? spare : cls).push_back(st);
        }
        (void)hipEventDestroy(ea);
        (void)hipEventDestroy(eb);
        if (cls.empty()) {                                     // one hardware queue in all: everything shares it
            hipStream_t st = nullptr;
            if (!spare.empty()) st = spare.back();
            else HIPCHK(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio));
            cls.push_back(st);
        }
        hipStream_t qB = cls[0], qC = cls[cls.size() > 1 ? 1 : 0], qD = cls[cls.size() > 2 ? 2 : cls.size() - 1];
        // roles that share a queue still get streams of their own where a spare on that queue exists (ordering stays per role)
        ss.s[0] = qB;
        ss.s[1] = qC;
        ss.s[2] = qD;
        ss.s[3] = qD;
        ss.s[4] = qB;
        if (dbg)
            fprintf(stderr, "masr side streams (device %d): %zu hardware queues besides the NULL stream's after %zu candidates; search 0 / "
                    "lane 1 = %p, search 1 = %p, preparation / copy = %p\n", dev, cls.size(), cls.size() + spare.size(), (void*)qB,
                    (void*)qC, (void*)qD);
        ss.made = true;
    }
    *out = &ss;
    return 0;
}

namespace masr {
// frames behind the subsampling front-end (before the Efficient-Conformer's stride layer): the unit of a stream's cap and offset
int subsampled_frames(const masr_engine* e, int feature_frames) { return sub_frames(e->input_layer, feature_frames); }
}  // namespace masr

extern "C" {

const char* masr_last_error(void) { return g_err.c_str(); }
int masr_version(void) { return 1; }

int masr_create(const masr_config* cfg, masr_engine** out) {
    if (!cfg || !out) return fail("null argument");
    if (cfg->model_kind < 0 || cfg->model_kind > 3)
        return fail("model_kind must be 0 (conformer), 1 (squeezeformer, non-streaming), 2 (efficient_conformer) or 3 (deepspeech2)");
    // n_mels = input feature size of the model: 80 (fbank), n_mfcc (mfcc) or 161 (linear) -- audio_featurizer.py:141-154
    if (cfg->n_mels < 7 || cfg->n_mels > 512) return fail("input feature size (n_mels) must be in [7, 512]");
    if (cfg->model_kind == 3) {
        if (cfg->d_model < 256 || cfg->d_model > 2048 || cfg->d_model % 256)
            return fail("deepspeech2: rnn_size (masr_config.d_model) must be a multiple of 256 in [256, 2048], got " +
                        std::to_string(cfg->d_model));
        if (cfg->num_blocks <= 0) return fail("deepspeech2: num_rnn_layers must be positive");
        if (cfg->reserved[0] != 0 && cfg->reserved[0] != 1)
            return fail("deepspeech2: the recurrent cell (masr_config.reserved[0], encoder_conf.use_gru) must be 0 = LSTM or 1 = GRU");
    } else if (!(cfg->d_model == 256 && cfg->heads == 4) && !(cfg->model_kind == 0 && cfg->d_model == 512 && cfg->heads == 8)) {
        return fail("output_size / attention_heads (masr_config.d_model / heads) = " + std::to_string(cfg->d_model) + " / " +
                    std::to_string(cfg->heads) + " is not supported: 256 / 4 for every family, 512 / 8 for the Conformer "
                    "(model_kind 0) only");
    } else if (cfg->d_ff <= 0 || cfg->d_ff % 128) {
        // (0 and the negative multiples pass the remainder test; ffn() would then launch the fused kernels with no chunks)
        return fail("d_ff (linear_units) must be a positive multiple of 128, got " + std::to_string(cfg->d_ff));
    } else if (cfg->d_model != 256) {
        // the width-generic path (wide.hip) carries the shipped Conformer variant only
        if (cfg->reserved[0] == 1)
            return fail("output_size " + std::to_string(cfg->d_model) + ": cnn_module_norm: batch_norm is implemented at output_size 256 only");
        if (cfg->reserved[3] != IL_CONV2D)
            return fail("output_size " + std::to_string(cfg->d_model) + ": input_layer must be conv2d (conv2d6 / conv2d8 are implemented at "
                        "output_size 256 only)");
    }
    // pos_enc_layer_type: the Conformer's slot is reserved[2]; the Squeezeformer leaves that slot unused and runs rel_pos only (the
    // Efficient Conformer keeps its group size there and has no slot for a mode: rel_pos only as well)
    if (cfg->model_kind == 0 && (cfg->reserved[2] < POS_ENC_REL || cfg->reserved[2] > POS_ENC_NONE))
        return fail("conformer: pos_enc_layer_type (masr_config.reserved[2]) must be 0 = rel_pos, 1 = abs_pos or 2 = no_pos, got " +
                    std::to_string(cfg->reserved[2]));
    // activation_type: the Conformer's slot is reserved[4] (no other kind reads it there: the Efficient Conformer keeps its norm
    // selector in it).  Anything but swish runs the width-generic layer, which carries LayerNorm in the conv module only.
    if (cfg->model_kind == 0) {
        if (cfg->reserved[4] < ENC_ACT_SWISH || cfg->reserved[4] > ENC_ACT_SELU)
            return fail("conformer: activation_type (masr_config.reserved[4]) must be 0 = swish, 1 = relu, 2 = gelu, 3 = tanh, "
                        "4 = hardtanh or 5 = selu, got " + std::to_string(cfg->reserved[4]));
        if (cfg->reserved[4] != ENC_ACT_SWISH && cfg->reserved[0] == 1)
            return fail("conformer: activation_type (masr_config.reserved[4]) = " + std::to_string(cfg->reserved[4]) +
                        " with cnn_module_norm: batch_norm (masr_config.reserved[0] = 1) is not supported: batch_norm runs with swish "
                        "(0) only");
    }
    if (cfg->model_kind == 1 && cfg->reserved[2] != 0)
        return fail("squeezeformer: pos_enc_layer_type (masr_config.reserved[2]) = " + std::to_string(cfg->reserved[2]) +
                    " is not supported: rel_pos (0) only; abs_pos / no_pos are implemented for the conformer (model_kind 0)");
    if (cfg->model_kind == 2) {
        // (the stride layer halves the kernel: its kernels are built around 15 / 7)
        if (cfg->cnn_kernel != 15)
            return fail("efficient_conformer: cnn_module_kernel (masr_config.cnn_kernel) = " + std::to_string(cfg->cnn_kernel) +
                        " is not supported: 15 only");
    } else if (cfg->model_kind != 3) {
        // the depthwise kernels hold at most 32 taps in registers; the symmetric padding of a streaming: False build needs
        // (K - 1) / 2 rows on each side (the reference asserts it, convolution.py)
        const char* fam = cfg->model_kind == 0 ? "conformer" : "squeezeformer";
        if (cfg->cnn_kernel < 3 || cfg->cnn_kernel > 31)
            return fail(std::string(fam) + ": cnn_module_kernel (masr_config.cnn_kernel) = " + std::to_string(cfg->cnn_kernel) +
                        " is not supported: an integer in [3, 31]");
        if (!cfg->causal && cfg->cnn_kernel % 2 == 0)
            return fail(std::string(fam) + ": cnn_module_kernel (masr_config.cnn_kernel) = " + std::to_string(cfg->cnn_kernel) +
                        " is not supported with streaming: False (causal = 0): the symmetric padding needs an odd value in [3, 31]");
    }
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail("no HIP device");
    HIPCHK(hipSetDevice(cfg->device_id));
    {
        SideStreams* ss = nullptr;                   // (created with the first engine of the device: a fixed place in the process's history)
        if (side_streams_of(cfg->device_id, &ss)) return 1;
    }
    masr_engine* e = new masr_engine();
    e->cfg = *cfg;
    if (e->cfg.max_pos <= 0) e->cfg.max_pos = 5000;
    e->reduce_idx = cfg->model_kind == 1 ? cfg->reserved[0] : -1;
    // (the Efficient Conformer's reserved[0] is its stride layer: its norm selector sits in reserved[4])
    e->conv_bn = (cfg->model_kind == 0 && cfg->reserved[0] == 1) || (cfg->model_kind == 2 && cfg->reserved[4] == 1);
    e->ds2_gru = cfg->model_kind == 3 && cfg->reserved[0] == 1;
    e->recover_idx = cfg->model_kind == 1 ? cfg->reserved[1] : -1;
    e->pos_enc = cfg->model_kind == 0 ? cfg->reserved[2] : POS_ENC_REL;
    e->act = cfg->model_kind == 0 ? cfg->reserved[4] : ENC_ACT_SWISH;
    if (cfg->model_kind == 0 ||cfg->model_kind == 2) {
        if (cfg->reserved[3] < IL_CONV2D || cfg->reserved[3] > IL_CONV2D8) {
            delete e;
            return fail("input_layer (masr_config.reserved[3]) must be 0 = conv2d, 1 = conv2d6 or 2 = conv2d8");
        }
        e->input_layer = cfg->reserved[3];
    }
    if (cfg->model_kind == 2) {
        e->stride_idx = cfg->reserved[0];
        e->n_group_layers = cfg->reserved[1];
        e->group_size = cfg->reserved[2];
        if (e->group_size != 3) { delete e; return fail("efficient_conformer: group_size must be 3"); }
    }
    if (build_fbank_tables(e)) {
        masr_destroy(e);
        return 1;
    }
    *out = e;
    return 0;
}

void masr_destroy(masr_engine* e) {
    if (!e) return;
    for (void* p : e->owned) (void)hipFree(p);
    for (void* p : e->dec.owned) (void)hipFree(p);
    e->release_all();
    for (auto& w : e->parked) w.release_all();
    e->beam_pool.release();
    e->beam_state.release();
    if (e->pack_ev) (void)hipEventDestroy(e->pack_ev);
    for (auto& s : e->streams) {
        s.att.release();
        s.cnn.release();
        s.cnn2.release();
    }
    for (auto& g : e->gbeams) {
        g.pool.release();
        g.state.release();
    }
    for (auto& kv : e->beam_ws) {
        kv.second.first.release();
        kv.second.second.release();
    }
    for (auto& kv : e->ms_ws) kv.second.release();
    for (auto& kv : e->packed) kv.second.release();
    for (auto& ev : e->prof_events) {
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    delete e;
}

// The fragment-ordered weight copies (masr_engine::packed) are built on first use and keyed by the device pointer of the weights
// they were packed from.  A reload (masr_load_tensor on a finalized engine, then masr_finalize) replaces those weights: every
// reload drops the copies (after the device has drained: launches in flight may still read them), so that no key can outlive
// the values it was packed from, whichever device buffers the new upload lands in (tests/test_gpu_ffn_packed.py).
static void drop_packed_weights(masr_engine* e) {
    if (e->packed.empty()) return;
    (void)hipSetDevice(e->cfg.device_id);
    (void)hipDeviceSynchronize();
    for (auto& kv : e->packed) kv.second.release();
    e->packed.clear();
}

int masr_load_tensor(masr_engine* e, const char* name, const float* host, const int64_t* shape, int32_t ndim) {
    if (!e || !name || !host) return fail("null argument");
    std::string n(name);
    const bool dec_name = e->dec.enabled && (n.rfind("decoder.left_decoder.", 0) == 0 || n.rfind("decoder.right_decoder.", 0) == 0);
    if (n.rfind("encoder.", 0) != 0 && n.rfind("ctc.", 0) != 0 && n.rfind("decoder.ctc_lo.", 0) != 0 && n != "__pos_table__" && !dec_name)
        return 0;
    drop_packed_weights(e);
    HostTensor t;
    int64_t cnt = 1;
    for (int i = 0; i < ndim; ++i) {
        t.shape.push_back(shape[i]);
        cnt *= shape[i];
    }
    t.v.assign(host, host + cnt);
    e->host[n] = std::move(t);
    e->finalized = false;
    return 0;
}

static int finalize_squeezeformer(masr_engine* e, hipStream_t s);
static int finalize_ds2(masr_engine* e);
static int enc_dim(const masr_engine* e) {      // width of the encoder output rows
    return e->cfg.model_kind == 3 ? e->cfg.d_model * (e->cfg.causal ? 1 : 2) : e->cfg.d_model;
}
static int layer_kernel(const masr_engine* e, int i) {          // efficient conformer: kernel // stride after the stride layer
    return (e->cfg.model_kind == 2 && e->stride_idx >= 0 && i > e->stride_idx) ? e->cfg.cnn_kernel / 2 : e->cfg.cnn_kernel;
}
static bool layer_grouped(const masr_engine* e, int i) { return e->cfg.model_kind == 2 && i < e->n_group_layers; }

static int finalize_model(masr_engine* e, void* stream);

int masr_finalize(masr_engine* e, void* stream) {
    if (!e) return fail("null engine");
    // the decoder first: the model's own finalize drops the host copies of every tensor when it is done
    if (e->dec.enabled) CHK(finalize_decoder(e));
    return finalize_model(e, stream);
}

static int finalize_model(masr_engine* e, void* stream) {
    if (e->cfg.model_kind == 1) return finalize_squeezeformer(e, (hipStream_t)stream);
    if (e->cfg.model_kind == 3) return finalize_ds2(e);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(e->cfg.device_id));
    const int d = e->cfg.d_model, dff = e->cfg.d_ff, L = e->cfg.num_blocks, V = e->cfg.vocab_size, F = e->cfg.n_mels;
    const int il = e->input_layer, F2 = sub_bins(il, F), K = e->cfg.cnn_kernel, H = e->cfg.heads, dk = d / H;
    const HostTensor* t;
    CHK(up(e, "encoder.global_cmvn.mean", {F}, &e->cmvn_mean));
    CHK(up(e, "encoder.global_cmvn.istd", {F}, &e->cmvn_istd));
    {   // conv1 [d,1,3,3] -> [9][d]
        CHK(get(e, "encoder.embed.conv.0.weight", {d, 1, 3, 3}, &t));
        std::vector<float> w(9 * d);
        for (int c = 0; c < d; ++c)
            for (int k = 0; k < 9; ++k) w[k * d + c] = t->v[c * 9 + k];
        CHK(upload(e, w, &e->conv1_w));
        CHK(up(e, "encoder.embed.conv.0.bias", {d}, &e->conv1_b));
    }
    // conv2 (and conv2d8's conv3) [co,ci,KS,KS] -> [co][ci / 32][kh*KS+kw][ci % 32]: the implicit GEMM walks the KS^2 window
    // positions of one 32-channel block in consecutive K slabs, so the overlapping input columns of neighbouring positions (kw = 2
    // of one output, kw = 0 of the next) are re-read a slab or two later -- out of L1 / L2 instead of HBM
    auto conv_kxk = [&](const char* wname, const char* bname, int ks, float** wd, float** bd) -> int {
        const int kk = ks * ks;
        CHK(get(e, wname, {d, d, ks, ks}, &t));
        std::vector<float> w((size_t)d * kk * d);
        for (int co = 0; co < d; ++co)
            for (int ci = 0; ci < d; ++ci)
                for (int k = 0; k < kk; ++k)
                    w[(size_t)co * kk * d + (size_t)(ci / 32) * kk * 32 + k * 32 + ci % 32] = t->v[((size_t)co * d + ci) * kk + k];
        CHK(upload(e, w, wd));
        return up(e, bname, {d}, bd);
    };
    CHK(conv_kxk("encoder.embed.conv.2.weight", "encoder.embed.conv.2.bias", il == IL_CONV2D6 ? 5 : 3, &e->conv2_w, &e->conv2_b));
    if (il == IL_CONV2D8) CHK(conv_kxk("encoder.embed.conv.4.weight", "encoder.embed.conv.4.bias", 3, &e->conv3_w, &e->conv3_b));
    {   // embed.out.0 (conv2d) / embed.linear (conv2d6, conv2d8) [d][c*F2+f] -> [d][f*d + c]   (subsampling.py:110, 151, 206
        // flatten channel-major)
        const std::string lin = il == IL_CONV2D ? "encoder.embed.out.0" : "encoder.embed.linear";
        if (il != IL_CONV2D && e->host.count("encoder.embed.out.0.weight"))
            return fail("input_layer conv2d6 / conv2d8 but the checkpoint holds encoder.embed.out.0 (a conv2d front-end)");
        if (il == IL_CONV2D && e->host.count("encoder.embed.linear.weight"))
            return fail("input_layer conv2d but the checkpoint holds encoder.embed.linear (a conv2d6 / conv2d8 front-end)");
        if (il != IL_CONV2D8 && e->host.count("encoder.embed.conv.4.weight"))
            return fail("the checkpoint holds a third subsampling conv (encoder.embed.conv.4, conv2d8) but input_layer is not conv2d8");
        CHK(get(e, lin + ".weight", {d, (int64_t)d * F2}, &t));
        std::vector<float> w((size_t)d * d * F2);
        for (int o = 0; o < d; ++o)
            for (int c = 0; c < d; ++c)
                for (int f = 0; f < F2; ++f) w[(size_t)o * d * F2 + f * d + c] = t->v[(size_t)o * d * F2 + c * F2 + f];
        CHK(upload(e, w, &e->embed_w));
        CHK(up(e, lin + ".bias", {d}, &e->embed_b));
    }
    {   // positional table (conformer/embedding.py:31-37)
        auto it = e->host.find("__pos_table__");
        if (it != e->host.end()) {
            if ((int64_t)it->second.v.size() != (int64_t)e->cfg.max_pos * d) return fail("__pos_table__ has wrong size");
            CHK(upload(e, it->second.v, &e->pe));
        } else {
            std::vector<float> pe((size_t)e->cfg.max_pos * d);
            for (int i = 0; i < d; i += 2) {
                const float div = expf((float)i * (float)(-(log(10000.0) / d)));
                for (int p = 0; p < e->cfg.max_pos; ++p) {
                    pe[(size_t)p * d + i] = sinf((float)p * div);
                    pe[(size_t)p * d + i + 1] = cosf((float)p * div);
                }
            }
            CHK(upload(e, pe, &e->pe));
        }
    }
    e->layers.assign(L, LayerW{});
    for (int i = 0; i < L; ++i) {
        LayerW& w = e->layers[i];
        const std::string p = "encoder.encoders." + std::to_string(i) + ".";
        auto ln = [&](const std::string& n, float** ww, float** bb) -> int {
            CHK(up(e, p + n + ".weight", {d}, ww));
            return up(e, p + n + ".bias", {d}, bb);
        };
        CHK(ln("norm_ff_macaron", &w.ln_ffm_w, &w.ln_ffm_b));
        CHK(ln("norm_mha", &w.ln_mha_w, &w.ln_mha_b));
        CHK(ln("norm_conv", &w.ln_conv_w, &w.ln_conv_b));
        CHK(ln("norm_ff", &w.ln_ff_w, &w.ln_ff_b));
        CHK(ln("norm_final", &w.ln_fin_w, &w.ln_fin_b));
        if (e->conv_bn) {
            // cnn_module_norm: batch_norm (conformer/convolution.py:60-67): eval-mode BatchNorm1d folded into y = x * scale + shift
            const HostTensor *tw, *tb, *tm, *tv;
            CHK(get(e, p + "conv_module.norm.weight", {d}, &tw));
            CHK(get(e, p + "conv_module.norm.bias", {d}, &tb));
            CHK(get(e, p + "conv_module.norm.running_mean", {d}, &tm));
            CHK(get(e, p + "conv_module.norm.running_var", {d}, &tv));
            // (the reference's own float32 steps, so that y = fma(x, scale, shift) is its eval-mode batch_norm bit for bit:
            //  invstd = 1 / sqrt(var + eps), scale = weight * invstd, shift = fma(-mean, scale, bias))
            std::vector<float> sc(d), sh(d);
            for (int c = 0; c < d; ++c) {
                const float invstd = 1.0f / sqrtf(tv->v[c] + 1e-5f);
                sc[c] = tw->v[c] * invstd;
                sh[c] = fmaf(-tm->v[c], sc[c], tb->v[c]);
            }
            CHK(upload(e, sc, &w.cln_w));
            CHK(upload(e, sh, &w.cln_b));
        } else {
            CHK(ln("conv_module.norm", &w.cln_w, &w.cln_b));
        }
        CHK(up(e, p + "feed_forward_macaron.w_1.weight", {dff, d}, &w.ffm_w1));
        CHK(up(e, p + "feed_forward_macaron.w_1.bias", {dff}, &w.ffm_b1));
        CHK(up(e, p + "feed_forward_macaron.w_2.weight", {d, dff}, &w.ffm_w2));
        CHK(up(e, p + "feed_forward_macaron.w_2.bias", {d}, &w.ffm_b2));
        CHK(up(e, p + "feed_forward.w_1.weight", {dff, d}, &w.ff_w1));
        CHK(up(e, p + "feed_forward.w_1.bias", {dff}, &w.ff_b1));
        CHK(up(e, p + "feed_forward.w_2.weight", {d, dff}, &w.ff_w2));
        CHK(up(e, p + "feed_forward.w_2.bias", {d}, &w.ff_b2));
        {   // fused QKV projection [3d, d]
            std::vector<float> wq((size_t)3 * d * d), bq(3 * d);
            const char* nm[3] = {"linear_q", "linear_k", "linear_v"};
            for (int j = 0; j < 3; ++j) {
                CHK(get(e, p + "self_attn." + nm[j] + ".weight", {d, d}, &t));
                memcpy(&wq[(size_t)j * d * d], t->v.data(), sizeof(float) * d * d);
                CHK(get(e, p + "self_attn." + nm[j] + ".bias", {d}, &t));
                memcpy(&bq[j * d], t->v.data(), sizeof(float) * d);
            }
            CHK(upload(e, wq, &w.wqkv));
            CHK(upload(e, bq, &w.bqkv));
        }
        CHK(up(e, p + "self_attn.linear_out.weight", {d, d}, &w.wo));
        CHK(up(e, p + "self_attn.linear_out.bias", {d}, &w.bo));
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
        CHK(up(e, p + "conv_module.pointwise_conv1.weight", {2 * d, d, 1}, &w.pw1_w));   // rows: value c, gate d + c
        CHK(up(e, p + "conv_module.pointwise_conv1.bias", {2 * d}, &w.pw1_b));
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
        {   // glu(bias): what the zero left-padding of the causal conv turns into behind pointwise_conv1 + GLU
            std::vector<float> z(d, 0.f);
            CHK(upload(e, z, &w.gconst));
            if (d == 256) launch_glu_const(w.pw1_b, w.gconst, (hipStream_t)stream);
            else launch_glu_const_wide(w.pw1_b, w.gconst, d, (hipStream_t)stream);
        }
        {   // depthwise [d,1,K_i] -> [K_i][d]
            const int K = layer_kernel(e, i);
            CHK(get(e, p + "conv_module.depthwise_conv.weight", {d, 1, K}, &t));
            std::vector<float> wd((size_t)K * d);
            for (int c = 0; c < d; ++c)
                for (int j = 0; j < K; ++j) wd[(size_t)j * d + c] = t->v[(size_t)c * K + j];
            CHK(upload(e, wd, &w.dw_w));
            CHK(up(e, p + "conv_module.depthwise_conv.bias", {d}, &w.dw_b));
        }
        CHK(up(e, p + "conv_module.pointwise_conv2.weight", {d, d, 1}, &w.pw2_w));
        CHK(up(e, p + "conv_module.pointwise_conv2.bias", {d}, &w.pw2_b));
        if (e->pos_enc == POS_ENC_REL) {   // positional keys p_j = W_pos * PE(j) for every position, once (attention.py:229-231)
            void* pt = nullptr;
            HIPCHK(hipMalloc(&pt, (size_t)e->cfg.max_pos * d * sizeof(float)));
            e->owned.push_back(pt);
            w.ptab = (float*)pt;
            gemm(e, s, e->pe, d, w.wpos, nullptr, w.ptab, d, e->cfg.max_pos, d, d, ACT_NONE, 1.f, nullptr, 0, PROF_NONE);
        }
    }
    CHK(up(e, "encoder.after_norm.weight", {d}, &e->after_w));
    CHK(up(e, "encoder.after_norm.bias", {d}, &e->after_b));
    CHK(up(e, "ctc.ctc_lo.weight", {V, d}, &e->ctc_w));
    CHK(up(e, "ctc.ctc_lo.bias", {V}, &e->ctc_b));

    HIPCHK(hipStreamSynchronize(s));
    e->host.clear();
    e->finalized = true;
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Encoder orchestration
// ------------------------------------------------------------------------------------------------
namespace {

struct EncodeCtx {
    int nseq;        // sequences (utterances or streams)
    int Tq;          // encoder frames per sequence in this call
    const int* lens; // device feature lengths for pad masking, or nullptr (streaming)
};

// the FFNs of a layer as ffn() calls on M rows: a call site adds what it wants beside the block (post, tail, head)
FfnArgs ffn_of(int M, const float* lnw, const float* lnb, const float* w1, const float* b1, const float* w2, const float* b2) {
    FfnArgs a;
    a.M = M; a.lnw = lnw; a.lnb = lnb; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
    return a;
}
FfnArgs ffn_macaron(const LayerW& w, int M) { return ffn_of(M, w.ln_ffm_w, w.ln_ffm_b, w.ffm_w1, w.ffm_b1, w.ffm_w2, w.ffm_b2); }
// (y: where the layer's norm_final goes when it rides on this call -- a.post; nullptr: the caller runs or defers it)
FfnArgs ffn_final(const LayerW& w, int M, float* y = nullptr) {
    FfnArgs a = ffn_of(M, w.ln_ff_w, w.ln_ff_b, w.ff_w1, w.ff_b1, w.ff_w2, w.ff_b2);
    a.post = {w.ln_fin_w, w.ln_fin_b, y};
    return a;
}
// Squeezeformer (post-LN): adaptive scale / bias in front of the block, the whole block added, `post` = the LayerNorm behind it
FfnArgs ffn_sqz(int M, const float* s, const float* b, const float* w1, const float* b1, const float* w2, const float* b2,
                const float* post_w, const float* post_b, float* post_y) {
    FfnArgs a = ffn_of(M, s, b, w1, b1, w2, b2);
    a.scale = 1.0f; a.affine = 1; a.post = {post_w, post_b, post_y};
    return a;
}
FfnArgs ffn_sqz1(const SqLayerW& w, int M, float* y) { return ffn_sqz(M, w.f1_s, w.f1_b, w.f1_w1, w.f1_b1, w.f1_w2, w.f1_b2, w.ln2_w, w.ln2_b, y); }
FfnArgs ffn_sqz2(const SqLayerW& w, int M, float* y) { return ffn_sqz(M, w.f2_s, w.f2_b, w.f2_w1, w.f2_b1, w.f2_w2, w.f2_b2, w.ln4_w, w.ln4_b, y); }
// tail stage of a layer's first FFN: the attention block's LayerNorm + fused QKV projection into out [M, ldo]
FfnTail qkv_tail(const masr_engine* e, const LayerW& w, float* out, int ldo) {
    FfnTail t{};
    t.lnw = w.ln_mha_w; t.lnb = w.ln_mha_b; t.W = w.wqkv; t.bias = w.bqkv; t.out = out; t.N = 3 * e->cfg.d_model; t.ldo = ldo;
    return t;
}
// a depthwise launch of elementwise.hip; a tap count it has no kernel for is an error, never a launch that did not happen
#define DWCHK(launched, ktaps)                                                                                        \
    do {                                                                                                              \
        if (!(launched)) return fail("no depthwise kernel for cnn_module_kernel " + std::to_string(ktaps) + ": " #launched); \
    } while (0)

// head stage of a layer's second FFN: the conv module behind pointwise_conv1 + GLU, on the offline GLU buffer (whose causal
// history rows are the constant glu(bias), not materialised)
FfnHead conv_head(const masr_engine* e, const LayerW& w, const int* lens, int Tq, int ktaps, int mstride) {
    FfnHead h{};
    h.glu = e->glu.as<float>(); h.dw_w = w.dw_w; h.dw_b = w.dw_b; h.lnw = w.cln_w; h.lnb = w.cln_b;
    h.gconst = e->cfg.causal ? w.gconst : nullptr; h.W = w.pw2_w; h.bias = w.pw2_b;
    h.lens = lens; h.seq_t = Tq; h.ktaps = ktaps; h.mstride = mstride; h.norm = e->conv_bn ? 1 : 0;
    return h;
}

// what ffn() did with the stages asked for; as an int: the error code (0 = launched)
struct FfnDone {
    int err;
    bool tail_done = false;   // the kernel ran the tail stage; otherwise the caller launches it
    bool head_done = false;   // the kernel ran the head stage; otherwise ffn() has launched it in front of the block
    FfnDone(int err_ = 0) : err(err_) {}
    operator int() const { return err; }
};

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
        RowGemmArgs g = rg_args(e->dwo.as<float>(), d, head.W, head.bias, x, d, M, d);
        g.R = x; g.ldr = d; g.lens = head.lens; g.mask_tp = head.lens ? head.seq_t : 0; g.mstride = head.mstride;
        rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_RESID, g);
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

// device lengths in conv2d units for the conv2d6 / conv2d8 front-ends (nullptr in, or conv2d: lens itself).  The encoder's kernels
// treat frame t of a sequence as padding when mstride * t >= lens (mstride 4 at the conv2d rate); with rate r the reference keeps
// frame t iff r * t < len, i.e. iff t < ceil(len / r) -- the same test on 4 * ceil(len / r)
static const int* sub_lens(masr_engine* e, hipStream_t s, const int* lens, int B) {
    if (!lens || e->input_layer == IL_CONV2D || B <= 0) return lens;
    if (e->sublens.ensure(sizeof(int) * B)) return nullptr;
    launch_sub_lens(lens, B, sub_rate(e->input_layer), e->sublens.as<int>(), s);
    return e->sublens.as<int>();
}

// feats [nseq, T, 80] -> x [nseq*Tq, d] (embed incl. x*sqrt(d)).  skip_lens: lengths in conv2d units (sub_lens)
int embed(masr_engine* e, hipStream_t s, const float* feats, int nseq, int T, int* Tq_out, const int* skip_lens = nullptr) {
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

// abs_pos (PositionalEncoding.forward, embedding.py:39-56): x * sqrt(d) + pe[offset : offset + Tq] -- embed() has multiplied, this
// adds the sinusoid rows in a launch of its own (multiply, round, add, round: the reference's two operations).  offs: the device
// offsets of the sequences (chunk steps: each stream's own), nullptr = 0 for all (full context).  The callers have checked
// offset + Tq against max_pos.  rel_pos hands the same rows to the layers instead; no_pos adds nothing.
void add_abs_pos(masr_engine* e, hipStream_t s, int nseq, int Tq, const int* offs) {
    if (e->pos_enc != POS_ENC_ABS) return;
    launch_add_pos_rows(e->x.as<float>(), e->pe, offs, nseq, Tq, e->cfg.d_model, e->cfg.max_pos, s);
}
// which attention instantiation a Conformer layer runs (common.h AttPos)
int att_pos(const masr_engine* e) { return e->pos_enc == POS_ENC_REL ? ATT_REL_POS : ATT_NO_POS; }

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
int conv_module(masr_engine* e, hipStream_t s, const LayerW& w, const EncodeCtx& c, bool hist, int K = 0, int mstride = 4,
                bool pw1_done = false, bool pw2_later = false) {
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
    {
        RowGemmArgs g = rg_args(e->dwo.as<float>(), d, w.pw2_w, w.pw2_b, x, d, M, d);
        g.R = x; g.ldr = d; g.lens = c.lens; g.mask_tp = c.lens ? c.Tq : 0; g.mstride = mstride;
        rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_RESID, g);
    }
    return 0;
}

// Streaming conv module of the Conformer family (LayerNorm conv norm), two launches on the small-M kernel:
//   [cnn cache | LayerNorm(new rows)] -> pointwise_conv1 + GLU        (+ the new cache)          (rowgemm_small PRO_HIST)
//   causal depthwise conv + LayerNorm + SiLU -> pointwise_conv2 + residual                       (rowgemm_small PRO_DWCONV)
// (convolution.py:98-131).  Where the small-M kernel does not apply (>= 2048 rows, frames per chunk not a multiple of 4) the
// same steps run as separate launches: conv_hist, pointwise_conv1, dwconv_ln_silu, pointwise_conv2.
int conv_module_stream(masr_engine* e, hipStream_t s, const LayerW& w, int n, int Tq, float* const* cache_rd,
                       float* const* cache_wr, int K, bool pw2_later = false) {
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
void mhsa(masr_engine* e, hipStream_t s, const LayerW& w, int M, const AttSeq* kv_seqs = nullptr, int kv_tq = 0) {
    const int d = e->cfg.d_model;
    RowGemmArgs g = rg_args(e->x.as<float>(), d, w.wqkv, w.bqkv, e->qkv.as<float>(), 3 * d, M, 3 * d);
    g.lnw = w.ln_mha_w; g.lnb = w.ln_mha_b; g.kv_seqs = kv_seqs; g.kv_tq = kv_tq;
    rowgemm(e, s, RG_PRO_LN, RG_EPI_STORE, g);
}
void mhsa_out(masr_engine* e, hipStream_t s, const LayerW& w, int M) {
    const int d = e->cfg.d_model;
    float* x = e->x.as<float>();
    RowGemmArgs g = rg_args(e->att.as<float>(), d, w.wo, w.bo, x, d, M, d);
    g.R = x; g.ldr = d;
    rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_RESID, g);
}

// offline conformer layer: attention out-projection + residual and the conv module's LayerNorm + pointwise_conv1 + GLU in ONE
// kernel (rowgemm EPI_CHAIN): the updated rows go to x (global) and, without leaving the CU, through the second GEMM
// K: the layer's depthwise kernel size (Efficient Conformer: 15 before, 7 behind the stride layer); att / a_seq_t / a_seq_stride: the
// attention output when it lives in a per-sequence padded buffer (grouped attention's planes)
void mhsa_out_pw1(masr_engine* e, hipStream_t s, const LayerW& w, const EncodeCtx& c, int mstride = 4, int K = 0,
                  const float* att = nullptr, int a_seq_t = 0, int a_seq_stride = 0) {
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

// ------------------------------------------------------------------------------------------------
// Width-generic Conformer path (masr_create admits it for model_kind 0 only): output_size 512 / attention_heads 8, and output_size
// 256 / 4 with an activation_type other than swish.  The layer of conformer/encoder.py:88-167 with every step as its own launch --
// the row kernels of wide.hip, the tiled GEMM of gemm_f32.hip for every product and the attention kernels with heads of 64.  No
// packed weight copies for the layers, none of the fused row-block kernels (they are built for K = 256 and for Swish), so none of
// their masr_debug_set switches applies here; the subsampling front end has no activation_type and runs as on the fused path.
// The activation (e->act) sits in two places: the epilogue of the first GEMM of wide_ffn and the tail of the depthwise kernel.
// ------------------------------------------------------------------------------------------------
bool is_wide(const masr_engine* e) { return e->cfg.model_kind == 0 && (e->cfg.d_model != 256 || e->act != ENC_ACT_SWISH); }

int ensure_wide_ws(masr_engine* e, int nseq, int Tq) {
    CHK(ensure_layer_ws(e, nseq, Tq));
    // hidden rows of an FFN [M, d_ff] or the value | gate rows of pointwise_conv1 over the padded layout [Mp, 2 d]
    const size_t Mp = (size_t)nseq * (Tq + e->cfg.cnn_kernel - 1);
    return e->hid.ensure(Mp * std::max(e->cfg.d_ff, 2 * e->cfg.d_model) * sizeof(float));
}

// x <- x + 0.5 * (W2 . act(W1 . LayerNorm(x) + b1) + b2), act = the engine's activation_type
int wide_ffn(masr_engine* e, hipStream_t s, int M, const float* lnw, const float* lnb, const float* w1, const float* b1,
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
int wide_layer(masr_engine* e, hipStream_t s, const LayerW& w, int nseq, int Tq, const int* lens, const AttSeq* seqs, int chunk,
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

}  // namespace

// ------------------------------------------------------------------------------------------------
// Squeezeformer (non-streaming build): weights + full-context forward
// reference: masr/model_utils/squeezeformer/{encoder,attention,convolution,positionwise,subsampling,time_reduction}.py
// ------------------------------------------------------------------------------------------------
static int upload_conv_frontend(masr_engine* e, const std::string& c1, const std::string& c2, const std::string& proj) {
    const int d = e->cfg.d_model, F = e->cfg.n_mels, F1 = (F - 1) / 2, F2 = (F1 - 1) / 2;
    const HostTensor* t;
    CHK(up(e, "encoder.global_cmvn.mean", {F}, &e->cmvn_mean));
    CHK(up(e, "encoder.global_cmvn.istd", {F}, &e->cmvn_istd));
    CHK(get(e, c1 + ".weight", {d, 1, 3, 3}, &t));
    {
        std::vector<float> w(9 * d);
        for (int c = 0; c < d; ++c)
            for (int k = 0; k < 9; ++k) w[k * d + c] = t->v[c * 9 + k];
        CHK(upload(e, w, &e->conv1_w));
    }
    CHK(up(e, c1 + ".bias", {d}, &e->conv1_b));
    CHK(get(e, c2 + ".weight", {d, d, 3, 3}, &t));
    {
        std::vector<float> w((size_t)d * 9 * d);
        for (int co = 0; co < d; ++co)
            for (int ci = 0; ci < d; ++ci)
                for (int k = 0; k < 9; ++k)          // [co][ci / 32][kh*3+kw][ci % 32], see masr_finalize
                    w[(size_t)co * 9 * d + (size_t)(ci / 32) * 9 * 32 + k * 32 + ci % 32] = t->v[((size_t)co * d + ci) * 9 + k];
        CHK(upload(e, w, &e->conv2_w));
    }
    CHK(up(e, c2 + ".bias", {d}, &e->conv2_b));
    CHK(get(e, proj + ".weight", {d, (int64_t)d * F2}, &t));
    {
        std::vector<float> w((size_t)d * d * F2);
        for (int o = 0; o < d; ++o)
            for (int c = 0; c < d; ++c)
                for (int f = 0; f < F2; ++f) w[(size_t)o * d * F2 + f * d + c] = t->v[(size_t)o * d * F2 + c * F2 + f];
        CHK(upload(e, w, &e->embed_w));
    }
    CHK(up(e, proj + ".bias", {d}, &e->embed_b));
    return 0;
}

static int upload_pos_table(masr_engine* e) {
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

static int finalize_squeezeformer(masr_engine* e, hipStream_t s) {
    HIPCHK(hipSetDevice(e->cfg.device_id));
    const int d = e->cfg.d_model, dff = e->cfg.d_ff, L = e->cfg.num_blocks, V = e->cfg.vocab_size, K = e->cfg.cnn_kernel,
              H = e->cfg.heads, dk = d / H;
    const HostTensor* t;
    CHK(upload_conv_frontend(e, "encoder.embed.pw_conv", "encoder.embed.dw_conv", "encoder.embed.input_proj.0"));
    CHK(upload_pos_table(e));
    CHK(up(e, "encoder.preln.weight", {d}, &e->preln_w));
    CHK(up(e, "encoder.preln.bias", {d}, &e->preln_b));
    e->sq_layers.assign(L, SqLayerW{});
    for (int i = 0; i < L; ++i) {
        SqLayerW& w = e->sq_layers[i];
        const std::string p = "encoder.encoders." + std::to_string(i) + ".";
        auto vec = [&](const std::string& n, float** out) -> int { return up(e, p + n, {d}, out); };
        CHK(vec("self_attn.ada_scale", &w.att_s));
        CHK(vec("self_attn.ada_bias", &w.att_b));
        {
            std::vector<float> wq((size_t)3 * d * d), bq(3 * d);
            const char* nm[3] = {"linear_q", "linear_k", "linear_v"};
            for (int j = 0; j < 3; ++j) {
                CHK(get(e, p + "self_attn." + nm[j] + ".weight", {d, d}, &t));
                memcpy(&wq[(size_t)j * d * d], t->v.data(), sizeof(float) * d * d);
                CHK(get(e, p + "self_attn." + nm[j] + ".bias", {d}, &t));
                memcpy(&bq[j * d], t->v.data(), sizeof(float) * d);
            }
            CHK(upload(e, wq, &w.wqkv));
            CHK(upload(e, bq, &w.bqkv));
        }
        CHK(up(e, p + "self_attn.linear_out.weight", {d, d}, &w.wo));
        CHK(up(e, p + "self_attn.linear_out.bias", {d}, &w.bo));
        CHK(up(e, p + "self_attn.linear_pos.weight", {d, d}, &w.wpos));
        CHK(up(e, p + "self_attn.pos_bias_u", {H, dk}, &w.pos_u));
        CHK(up(e, p + "self_attn.pos_bias_v", {H, dk}, &w.pos_v));
        {
            void* pt = nullptr;
            HIPCHK(hipMalloc(&pt, (size_t)e->cfg.max_pos * d * sizeof(float)));
            e->owned.push_back(pt);
            w.ptab = (float*)pt;
            gemm(e, s, e->pe, d, w.wpos, nullptr, w.ptab, d, e->cfg.max_pos, d, d, ACT_NONE, 1.f, nullptr, 0, PROF_NONE);
        }
        CHK(vec("layer_norm1.weight", &w.ln1_w)); CHK(vec("layer_norm1.bias", &w.ln1_b));
        CHK(vec("layer_norm2.weight", &w.ln2_w)); CHK(vec("layer_norm2.bias", &w.ln2_b));
        CHK(vec("layer_norm3.weight", &w.ln3_w)); CHK(vec("layer_norm3.bias", &w.ln3_b));
        CHK(vec("layer_norm4.weight", &w.ln4_w)); CHK(vec("layer_norm4.bias", &w.ln4_b));
        CHK(vec("ffn1.ada_scale", &w.f1_s)); CHK(vec("ffn1.ada_bias", &w.f1_b));
        CHK(up(e, p + "ffn1.w_1.weight", {dff, d}, &w.f1_w1)); CHK(up(e, p + "ffn1.w_1.bias", {dff}, &w.f1_b1));
        CHK(up(e, p + "ffn1.w_2.weight", {d, dff}, &w.f1_w2)); CHK(up(e, p + "ffn1.w_2.bias", {d}, &w.f1_b2));
        CHK(vec("ffn2.ada_scale", &w.f2_s)); CHK(vec("ffn2.ada_bias", &w.f2_b));
        CHK(up(e, p + "ffn2.w_1.weight", {dff, d}, &w.f2_w1)); CHK(up(e, p + "ffn2.w_1.bias", {dff}, &w.f2_b1));
        CHK(up(e, p + "ffn2.w_2.weight", {d, dff}, &w.f2_w2)); CHK(up(e, p + "ffn2.w_2.bias", {d}, &w.f2_b2));
        CHK(vec("conv_module.ada_scale", &w.cv_s)); CHK(vec("conv_module.ada_bias", &w.cv_b));
        CHK(up(e, p + "conv_module.pointwise_conv1.weight", {2 * d, d, 1}, &w.pw1_w));
        CHK(up(e, p + "conv_module.pointwise_conv1.bias", {2 * d}, &w.pw1_b));
        {   // streaming-trained build (causal conv): the K-1 zero frames padded in front of pointwise_conv1 become glu(bias)
            std::vector<float> z(d, 0.f);
            CHK(upload(e, z, &w.gconst));
            launch_glu_const(w.pw1_b, w.gconst, s);
        }
        {
            CHK(get(e, p + "conv_module.depthwise_conv.weight", {d, 1, K}, &t));
            std::vector<float> wd((size_t)K * d);
            for (int c = 0; c < d; ++c)
                for (int j = 0; j < K; ++j) wd[(size_t)j * d + c] = t->v[(size_t)c * K + j];
            CHK(upload(e, wd, &w.dw_w));
            CHK(up(e, p + "conv_module.depthwise_conv.bias", {d}, &w.dw_b));
        }
        {   // eval-mode BatchNorm1d folded: y = x * scale + shift, scale = w / sqrt(var + eps), shift = b - mean * scale
            const HostTensor *tw, *tb, *tm, *tv;
            CHK(get(e, p + "conv_module.norm.weight", {d}, &tw));
            CHK(get(e, p + "conv_module.norm.bias", {d}, &tb));
            CHK(get(e, p + "conv_module.norm.running_mean", {d}, &tm));
            CHK(get(e, p + "conv_module.norm.running_var", {d}, &tv));
            std::vector<float> sc(d), sh(d);
            for (int c = 0; c < d; ++c) {
                sc[c] = tw->v[c] / sqrtf(tv->v[c] + 1e-5f);
                sh[c] = tb->v[c] - tm->v[c] * sc[c];
            }
            CHK(upload(e, sc, &w.bn_scale));
            CHK(upload(e, sh, &w.bn_shift));
        }
        CHK(up(e, p + "conv_module.pointwise_conv2.weight", {d, d, 1}, &w.pw2_w));
        CHK(up(e, p + "conv_module.pointwise_conv2.bias", {d}, &w.pw2_b));
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
        CHK(up(e, "encoder.time_reduction_layer.pw_conv.weight", {d, d, 1}, &e->tr_pw_w));
        CHK(up(e, "encoder.time_reduction_layer.pw_conv.bias", {d}, &e->tr_pw_b));
        CHK(up(e, "encoder.time_recover_layer.weight", {d, d}, &e->rec_w));
        CHK(up(e, "encoder.time_recover_layer.bias", {d}, &e->rec_b));
    }
    CHK(up(e, "ctc.ctc_lo.weight", {V, d}, &e->ctc_w));
    CHK(up(e, "ctc.ctc_lo.bias", {V}, &e->ctc_b));
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
    HIPCHK(hipStreamSynchronize(s));
    e->host.clear();
    e->finalized = true;
    return 0;
}

// SqueezeformerEncoder.forward, streaming = False (squeezeformer/encoder.py:168-216)
static int encode_full_squeezeformer(masr_engine* e, hipStream_t s, const float* feats, const int* lens, int B, int T,
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
        if (!qkv_ready)
            {
                RowGemmArgs g = rg_args(x, d, w.wqkv, w.bqkv, e->qkv.as<float>(), 3 * d, M, 3 * d);
                g.lnw = w.att_s; g.lnb = w.att_b;
                rowgemm(e, s, RG_PRO_AFFINE, RG_EPI_STORE, g);
            }
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
        {
            RowGemmArgs g = rg_args(e->att.as<float>(), d, w.wo, w.bo, x, d, M, d);
            g.R = x; g.ldr = d;
            rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_RESID, g);
        }
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
        {
            RowGemmArgs g = rg_args(e->dwo.as<float>(), d, w.pw2_w, w.pw2_b, x, d, M, d);
            g.R = x; g.ldr = d; g.lens = lens; g.mask_tp = Tq; g.mstride = mstride;
            rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_RESID, g);
        }
        launch_layernorm(x, w.ln3_w, w.ln3_b, x, M, 1e-5f, 0, 0, nullptr, s);
        // x = LN4(x + FFN2(ada(x)))
        CHK(ffn(e, s, ffn_sqz2(w, M, i == L - 1 ? enc_out : x)));
    }
    LAUNCHCHK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Efficient Conformer, full-context forward (efficient_conformer/encoder.py:213-265): Conformer layers with
// grouped attention in the first n_group_layers blocks, a stride-2 conv block at stride_idx (AvgPool residual),
// half frame rate + kernel 7 afterwards.  Weights share the Conformer key names (masr_finalize).
// ------------------------------------------------------------------------------------------------
static int encode_full_efficient(masr_engine* e, hipStream_t s, const float* feats, const int* lens, int B, int T,
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
            else
                {
                    RowGemmArgs g = rg_args(e->attp.as<float>(), d, w.wo, w.bo, x, d, M, d);
                    g.R = x; g.ldr = d; g.mstride = mstride; g.a_seq_t = Tq; g.a_seq_stride = Tpad;
                    rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_RESID, g);
                }
        } else {
            if (!r1.tail_done) mhsa(e, s, w, M);
            {
                ProfScope ps(e, s, PROF_ATT, 6.0 * d * (double)Tq * Tq * B);
                launch_attention(seq_r, B, Tq, H, 3 * d, 3 * d, w.ptab, w.pos_u, w.pos_v, chunk, pstride, s, 256, ATT_REL_POS);
            }
            if (fused) mhsa_out_pw1(e, s, w, ctx0, mstride, Ki);
            else mhsa_out(e, s, w, M);
        }
        EncodeCtx ctx{B, Tq, lens};
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
            if (!causal)     // half rate, kernel 7 from here on: a new padded layout
                HIPCHK(hipMemsetAsync(e->glu.p, 0, (size_t)B * (Tq + layer_kernel(e, i + 1) - 1) * d * sizeof(float), s));
            {
                RowGemmArgs g = rg_args(e->dwo.as<float>(), d, w.pw2_w, w.pw2_b, x, d, M, d);
                g.R = e->xsave.as<float>(); g.ldr = d; g.lens = lens; g.mask_tp = Tq; g.mstride = mstride;
                rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_RESID, g);
            }
            launch_attseq_full(seq_r, e->qkv.as<float>(), e->att.as<float>(), lens, B, Tq, mstride, s);
        } else {
            CHK(conv_module(e, s, w, ctx, false, layer_kernel(e, i), mstride));
        }
        CHK(ffn(e, s, ffn_final(w, M)));
        launch_layernorm(x, w.ln_fin_w, w.ln_fin_b, x, M, 1e-5f, 0, 0, nullptr, s);
    }
    launch_layernorm(x, e->after_w, e->after_b, enc_out, B * Tq, 1e-5f, 0, 0, nullptr, s);
    LAUNCHCHK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// DeepSpeech2 (model_kind 3): weights + forward (full utterances and stateful chunks)
// reference: masr/model_utils/deepspeech2/{model.py:64-108, encoder.py:36-129, conv.py:5-22}
// ------------------------------------------------------------------------------------------------
static int finalize_ds2(masr_engine* e) {
    HIPCHK(hipSetDevice(e->cfg.device_id));
    const int H = e->cfg.d_model, L = e->cfg.num_blocks, ndir = e->cfg.causal ? 1 : 2, V = e->cfg.vocab_size;
    const int F = e->cfg.n_mels, F1 = (F - 1) / 2, F2 = (F1 - 1) / 2, C = 32, D = H * ndir;
    const HostTensor* t;
    CHK(up(e, "encoder.global_cmvn.mean", {F}, &e->cmvn_mean));
    CHK(up(e, "encoder.global_cmvn.istd", {F}, &e->cmvn_istd));
    CHK(get(e, "encoder.conv.conv.0.weight", {C, 1, 3, 3}, &t));
    {
        std::vector<float> w(9 * C);
        for (int c = 0; c < C; ++c)
            for (int k = 0; k < 9; ++k) w[k * C + c] = t->v[c * 9 + k];
        CHK(upload(e, w, &e->conv1_w));
    }
    CHK(up(e, "encoder.conv.conv.0.bias", {C}, &e->conv1_b));
    CHK(get(e, "encoder.conv.conv.2.weight", {C, C, 3, 3}, &t));
    {
        std::vector<float> w((size_t)C * 9 * C);
        for (int co = 0; co < C; ++co)
            for (int ci = 0; ci < C; ++ci)
                for (int k = 0; k < 9; ++k) w[(size_t)co * 9 * C + k * C + ci] = t->v[((size_t)co * C + ci) * 9 + k];
        CHK(upload(e, w, &e->conv2_w));
    }
    CHK(up(e, "encoder.conv.conv.2.bias", {C}, &e->conv2_b));
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
        CHK(up(e, p + "layer_norm.weight", {D}, &w.ln_w));
        CHK(up(e, p + "layer_norm.bias", {D}, &w.ln_b));
    }
    CHK(up(e, "decoder.ctc_lo.weight", {V, D}, &e->ctc_w));
    CHK(up(e, "decoder.ctc_lo.bias", {V}, &e->ctc_b));
    e->host.clear();
    e->finalized = true;
    return 0;
}

// feats [nseq, T, 80] -> enc_out [nseq*Tq, D].  lens: device feature lengths (full utterances) or nullptr (chunks:
// every row is valid, inference_predictor.py:70).  st: per-sequence streams carrying (h, c) of every layer, or nullptr.
static int ds2_forward(masr_engine* e, hipStream_t s, const float* feats, const int* lens, int nseq, int T, float* enc_out,
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

// ConformerEncoder.forward on the fused kernels (masr_encode_full: output_size 256, swish).  chunk: decoding_chunk_size in the
// streaming-trained build, 0 otherwise
static int encode_full_conformer(masr_engine* e, hipStream_t s, const float* feats_dev, const int* feat_lens_dev, int B, int T,
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

// the one refusal of a vocabulary the softmax / pruning kernels cannot hold (masr_ctc_probs and the chunk steps)
static const char kVocabRefusal[] = "vocab_size > 16384 is not supported by the softmax / pruning kernels (one 256-thread workgroup holds a row in registers)";

extern "C" {

int masr_encode_full(masr_engine* e, const float* feats_dev, const int32_t* feat_lens_dev, int32_t B, int32_t T,
                     int32_t decoding_chunk_size, float* enc_out_dev, void* stream) {
    if (!e || !e->finalized) return fail("engine not finalized");
    ENTER(e);
    CallGuard call_guard(e, (hipStream_t)stream);
    if (B <= 0) return fail("empty batch");
    hipStream_t s = (hipStream_t)stream;
    if (e->cfg.model_kind == 3) return ds2_forward(e, s, feats_dev, feat_lens_dev, B, T, enc_out_dev, nullptr, nullptr);
    // decoding_chunk_size > 0 limits the attention to chunks in the streaming-trained builds only (use_dynamic_chunk follows
    // `streaming`, model.py of every family; utils/mask.py:117-143 ignores it otherwise)
    const int chunk = (decoding_chunk_size > 0 && e->cfg.causal) ? decoding_chunk_size : 0;
    // conv2d6 / conv2d8: every mask below tests 4 * t against the lengths in conv2d units
    if (feat_lens_dev && e->input_layer != IL_CONV2D && !(feat_lens_dev = sub_lens(e, s, feat_lens_dev, B)))
        return fail("out of device memory (subsampled lengths)");
    if (e->cfg.model_kind == 1) return encode_full_squeezeformer(e, s, feats_dev, feat_lens_dev, B, T, enc_out_dev, chunk);
    if (e->cfg.model_kind == 2) return encode_full_efficient(e, s, feats_dev, feat_lens_dev, B, T, enc_out_dev, chunk);
    if (is_wide(e)) return encode_full_wide(e, s, feats_dev, feat_lens_dev, B, T, enc_out_dev, chunk);
    return encode_full_conformer(e, s, feats_dev, feat_lens_dev, B, T, enc_out_dev, chunk);
}

static int ctc_head(masr_engine* e, const float* enc_dev, int M, float* probs_dev, int write_probs, int32_t* argmax_dev,
                    float* maxprob_dev, hipStream_t s) {
    const int d = enc_dim(e), V = e->cfg.vocab_size;
    float* logits = probs_dev;
    if (!logits) {
        CHK(e->logits.ensure((size_t)M * V * sizeof(float)));
        logits = e->logits.as<float>();
    }
    gemm(e, s, enc_dev, d, e->ctc_w, e->ctc_b, logits, V, M, V, d, ACT_NONE, 1.f, nullptr, 0);
    launch_softmax_argmax(logits, M, V, V, write_probs, argmax_dev, maxprob_dev, s);
    LAUNCHCHK();
    return 0;
}

int masr_ctc_probs(masr_engine* e, const float* enc_dev, int32_t M, float* probs_dev, int32_t* argmax_dev,
                   float* maxprob_dev, void* stream) {
    if (!e || !e->finalized) return fail("engine not finalized");
    ENTER(e);
    CallGuard call_guard(e, (hipStream_t)stream);
    if (!probs_dev) return fail("probs_dev is null");
    if (e->cfg.vocab_size > 16384) return fail(kVocabRefusal);
    return ctc_head(e, enc_dev, M, probs_dev, 1, argmax_dev, maxprob_dev, (hipStream_t)stream);
}

int masr_ctc_greedy_frames(masr_engine* e, const float* enc_dev, int32_t M, int32_t* argmax_dev, float* maxprob_dev,
                           void* stream) {
    if (!e || !e->finalized) return fail("engine not finalized");
    ENTER(e);
    CallGuard call_guard(e, (hipStream_t)stream);
    if (e->cfg.model_kind == 3 || is_wide(e))      // K = 512 / 1024 / 2048 rows, or the width-generic path at 256 (no packed copies): generic GEMM + softmax statistics (logits stay in a workspace)
        return ctc_head(e, enc_dev, M, nullptr, 0, argmax_dev, maxprob_dev, (hipStream_t)stream);
    // few row blocks (one utterance: 7; the Efficient Conformer's half-rate output at 32 x 10 s: 124): the fused head gives a
    // workgroup 32 rows x the WHOLE vocabulary (165 us whether 7 or 248 row blocks run); below knobs().ctc_fused_blocks the logits go
    // through the tiled GEMM (vocabulary spread over the CUs) into a workspace and the softmax statistics are a second launch
    if ((M + 31) / 32 < knobs().ctc_fused_blocks) return ctc_head(e, enc_dev, M, nullptr, 0, argmax_dev, maxprob_dev, (hipStream_t)stream);
    // fused: logits GEMM + online softmax statistics + argmax, nothing but (idx, prob) leaves the chip
    {
        RowGemmArgs g = rg_args(enc_dev, e->cfg.d_model, e->ctc_w, e->ctc_b, nullptr, 0, M, e->cfg.vocab_size);
        g.out_idx = argmax_dev; g.out_maxp = maxprob_dev;
        rowgemm(e, (hipStream_t)stream, RG_PRO_PLAIN, RG_EPI_CTC, g);
    }
    LAUNCHCHK();
    return 0;
}

int masr_ctc_collapse(masr_engine* e, const int32_t* argmax_dev, const float* maxprob_dev, const int32_t* n_frames_dev,
                      int32_t B, int32_t Tp, int32_t blank, int32_t* tokens_dev, int32_t* n_tokens_dev,
                      float* score_dev, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    launch_ctc_collapse(argmax_dev, maxprob_dev, n_frames_dev, B, Tp, blank, tokens_dev, n_tokens_dev, score_dev,
                        (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

int masr_argmax_rows(masr_engine* e, const float* probs_dev, int32_t M, int32_t V, int32_t* argmax_dev,
                     float* maxprob_dev, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    if (V > 16384) return fail("V > 16384 not supported (one 256-thread workgroup holds a row in registers)");
    launch_argmax_rows(probs_dev, M, V, argmax_dev, maxprob_dev, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

int masr_ctc_topk(masr_engine* e, const float* probs_dev, int32_t M, int32_t V, int32_t top_n, float cutoff_prob,
                  int32_t* idx_dev, float* logp_dev, int32_t* count_dev, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    if (V > 16384) return fail("V > 16384 not supported (one 256-thread workgroup holds a row in registers)");
    if (top_n <= 0) return fail("top_n must be positive");
    launch_topk_prune(probs_dev, M, V, top_n, cutoff_prob, idx_dev, logp_dev, count_dev, -1, nullptr, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

int masr_ctc_topk_blank(masr_engine* e, const float* probs_dev, int32_t M, int32_t V, int32_t top_n, float cutoff_prob,
                        int32_t blank, int32_t* idx_dev, float* logp_dev, int32_t* count_dev, float* blank_logp_dev,
                        void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    if (V > 16384) return fail("V > 16384 not supported (one 256-thread workgroup holds a row in registers)");
    if (top_n <= 0) return fail("top_n must be positive");
    if (blank < 0 || blank >= V || !blank_logp_dev) return fail("masr_ctc_topk_blank: blank id out of range or null output");
    launch_topk_prune(probs_dev, M, V, top_n, cutoff_prob, idx_dev, logp_dev, count_dev, blank, blank_logp_dev,
                      (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

static int bind_lm(BeamGpuArgs& a, masr_lm* lm, float alpha, float beta) {
    a.use_lm = 0;
    a.lm_cache = knobs().beam_lm_cache;
    a.narrow = knobs().beam_narrow;
    a.alpha = alpha;
    a.beta = beta;
    if (!lm) return 0;
    if (lm_device_view(lm, &a.lm)) return fail(masr_lm_last_error());
    a.use_lm = 1;
    return 0;
}

int masr_beam_search_gpu(masr_engine* e, const int32_t* idx_dev, const float* logp_dev, const int32_t* count_dev,
                         const int32_t* frames_dev, int32_t B, int32_t T_stride, int32_t K, int32_t beam_size, int32_t blank,
                         int32_t* tokens_dev, int32_t max_len, int32_t* len_dev, float* score_dev, void* stream) {
    return masr_beam_search_gpu_lm(e, idx_dev, logp_dev, count_dev, frames_dev, B, T_stride, K, beam_size, blank, nullptr, 0.f,
                                   0.f, nullptr, tokens_dev, max_len, len_dev, score_dev, stream);
}

int masr_beam_search_gpu_lm(masr_engine* e, const int32_t* idx_dev, const float* logp_dev, const int32_t* count_dev,
                            const int32_t* frames_dev, int32_t B, int32_t T_stride, int32_t K, int32_t beam_size, int32_t blank,
                            masr_lm* lm, float alpha, float beta, const float* blank_logp_dev, int32_t* tokens_dev,
                            int32_t max_len, int32_t* len_dev, float* score_dev, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    if (B <= 0 || T_stride <= 0) return fail("empty batch");
    if (e->cfg.vocab_size > 16384 && e->finalized) return fail("vocab_size > 16384 not supported");
    BeamGpuArgs a{};
    a.cidx = idx_dev; a.clp = logp_dev; a.ccount = count_dev; a.frames = frames_dev;
    a.blank_lp = lm ? blank_logp_dev : nullptr;
    a.T_stride = T_stride; a.K = K; a.beam = beam_size; a.blank = blank; a.max_len = max_len;
    a.pool_cap = T_stride * beam_size + 1;
    if (lm && lm_word_based(lm))
        return fail("word-based language models are searched on host threads (masr_beam_search_batch_lm): the spelling "
                    "dictionary is not in the GPU kernel");
    if (K > 64 || beam_size > 512 || beam_size < 1 || beam_gpu_lds_bytes(beam_size, K, lm != nullptr) > 160 * 1024)
        return fail("beam search on the GPU needs cutoff_top_n <= 64, beam_size <= 512 and beam_size*cutoff_top_n*4 B + tables "
                    "within 160 KB of LDS; use masr_beam_search_batch (host threads) beyond that");
    DevBuf *pool = &e->beam_pool, *state = &e->beam_state;
    if (!e->beam_first_set) {
        e->beam_first_set = true;
        e->beam_first_stream = stream;
    } else if (stream != e->beam_first_stream) {
        auto& ws = e->beam_ws[stream];
        pool = &ws.first;
        state = &ws.second;
    }
    CHK(pool->ensure((size_t)B * a.pool_cap * 2 * sizeof(int)));
    CHK(state->ensure((size_t)B * beam_state_bytes(beam_size)));
    a.pool_parent = pool->as<int>();
    a.pool_ch = a.pool_parent + (size_t)B * a.pool_cap;
    beam_state_carve(state->p, B, beam_size, &a.state_h, &a.state_i, &a.state_f);
    CHK(bind_lm(a, lm, alpha, beta));
    a.init = 1;
    a.prof = e->beam_prof;
    a.tokens = tokens_dev; a.len = len_dev; a.score = score_dev;
    if (launch_beam_search(a, B, (hipStream_t)stream)) return fail("beam search launch rejected the sizes");
    LAUNCHCHK();
    return 0;
}

// ---- streaming beam search on the device (BeamSearchDecoder.decode_chunk / reset_decoder) -----------------------------
static void gbeam_args(GBeam& g, BeamGpuArgs& a) {
    a.pool_cap = g.cap;
    a.pool_parent = g.pool.as<int>();
    a.pool_ch = a.pool_parent + g.cap;
    beam_state_carve(g.state.p, 1, g.beam, &a.state_h, &a.state_i, &a.state_f);
}

int masr_gbeam_open(masr_engine* e, int32_t beam_size, int32_t blank, int32_t max_frames, int32_t* handle) {
    if (!e || !handle) return fail("null argument");
    ENTER(e);
    if (beam_size < 1 || beam_size > 512) return fail("beam_size must be in [1, 512]");
    if (max_frames <= 0) max_frames = 5000;
    int id = -1;
    for (size_t i = 0; i < e->gbeams.size(); ++i)
        if (!e->gbeams[i].open) { id = (int)i; break; }
    if (id < 0) {
        e->gbeams.emplace_back();
        id = (int)e->gbeams.size() - 1;
    }
    GBeam& g = e->gbeams[id];
    g.beam = beam_size;
    g.blank = blank;
    g.cap = max_frames * beam_size + 1;
    CHK(g.pool.ensure((size_t)g.cap * 2 * sizeof(int)));
    CHK(g.state.ensure(beam_state_bytes(beam_size)));
    g.lm = nullptr;
    g.alpha = g.beta = 0.f;
    g.open = true;
    g.started = false;
    *handle = id;
    return 0;
}

static int gbeam_of(masr_engine* e, int id, GBeam** out) {
    if (!e) return fail("null engine");
    if (id < 0 || id >= (int)e->gbeams.size() || !e->gbeams[id].open) return fail("bad beam handle");
    *out = &e->gbeams[id];
    return 0;
}

int masr_gbeam_set_lm(masr_engine* e, int32_t handle, masr_lm* lm, float alpha, float beta) {
    GBeam* g;
    CHK(gbeam_of(e, handle, &g));
    if (g->started) return fail("the language model of a stream can only change between utterances (after masr_gbeam_reset)");
    if (lm && lm_word_based(lm)) return fail("word-based language models are searched on host threads (masr_beam_*)");
    g->lm = lm;
    g->alpha = alpha;
    g->beta = beta;
    return 0;
}

int masr_gbeam_reset(masr_engine* e, int32_t handle) {
    GBeam* g;
    CHK(gbeam_of(e, handle, &g));
    g->started = false;
    return 0;
}

int masr_gbeam_close(masr_engine* e, int32_t handle) {
    GBeam* g;
    CHK(gbeam_of(e, handle, &g));
    ENTER(e);
    HIPCHK(hipDeviceSynchronize());
    g->pool.release();
    g->state.release();
    g->open = false;
    return 0;
}

int masr_gbeam_advance(masr_engine* e, int32_t handle, const int32_t* idx_dev, const float* logp_dev,
                       const int32_t* count_dev, int32_t T, int32_t K, int32_t* tokens_dev, int32_t max_len,
                       int32_t* len_dev, float* score_dev, void* stream) {
    return masr_gbeam_advance_lm(e, handle, idx_dev, logp_dev, count_dev, nullptr, T, K, tokens_dev, max_len, len_dev, score_dev,
                                 stream);
}

int masr_gbeam_advance_lm(masr_engine* e, int32_t handle, const int32_t* idx_dev, const float* logp_dev,
                          const int32_t* count_dev, const float* blank_logp_dev, int32_t T, int32_t K, int32_t* tokens_dev,
                          int32_t max_len, int32_t* len_dev, float* score_dev, void* stream) {
    GBeam* g;
    CHK(gbeam_of(e, handle, &g));
    ENTER(e);
    if (T < 0 || K > 64 || beam_gpu_lds_bytes(g->beam, K, g->lm != nullptr) > 160 * 1024)
        return fail("unsupported chunk / cutoff_top_n");
    BeamGpuArgs a{};
    a.cidx = idx_dev; a.clp = logp_dev; a.ccount = count_dev; a.frames = nullptr;
    a.blank_lp = g->lm ? blank_logp_dev : nullptr;
    a.T_stride = T; a.K = K; a.beam = g->beam; a.blank = g->blank; a.max_len = max_len;
    gbeam_args(*g, a);
    CHK(bind_lm(a, g->lm, g->alpha, g->beta));
    a.init = g->started ? 0 : 1;
    a.prof = nullptr;
    a.tokens = tokens_dev; a.len = len_dev; a.score = score_dev;
    // (the kernel stops allocating trie nodes at the pool capacity; max_frames bounds the utterance length)
    if (launch_beam_search(a, 1, (hipStream_t)stream)) return fail("beam search launch rejected the sizes");
    LAUNCHCHK();
    g->started = true;
    return 0;
}

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

// ---- streaming -----------------------------------------------------------------------------------------

int masr_stream_open(masr_engine* e, int32_t max_frames_out, int32_t* stream_id) {
    if (!e || !e->finalized) return fail("engine not finalized");
    ENTER(e);
    if (e->cfg.model_kind == 3) {
        if (!e->cfg.causal) return fail("deepspeech2: streaming needs the uni-directional model");
    } else if (!e->cfg.causal) {
        return fail("chunked streaming needs the streaming-trained (causal conv) build");
    }
    if (e->conv_bn && e->cfg.model_kind == 0) return fail("cnn_module_norm=batch_norm: only the full-context forward is implemented (the chunk-step kernels carry the LayerNorm variant)");
    if (max_frames_out <= 0 || max_frames_out > e->cfg.max_pos) max_frames_out = e->cfg.max_pos;
    int id = -1;
    for (size_t i = 0; i < e->streams.size(); ++i)
        if (!e->streams[i].open) { id = (int)i; break; }
    if (id < 0) {
        e->streams.emplace_back();
        id = (int)e->streams.size() - 1;
    }
    Stream& st = e->streams[id];
    const int d = e->cfg.d_model, L = e->cfg.num_blocks, pad = e->cfg.cnn_kernel - 1;
    st.cap = max_frames_out;
    if (e->cfg.model_kind == 3) {      // recurrent state (h, c) per layer; no attention cache, no frame limit
        st.cap = 1 << 30;
        CHK(st.cnn.ensure((size_t)L * 2 * d * sizeof(float)));
        CHK(clear_sync(st.cnn.p, 0, (size_t)L * 2 * d * sizeof(float)));
        st.offset = 0;
        st.open = true;
        *stream_id = id;
        return 0;
    }
    CHK(st.att.ensure((size_t)L * st.cap * 2 * d * sizeof(float)));
    CHK(st.cnn.ensure((size_t)L * pad * d * sizeof(float)));
    CHK(clear_sync(st.cnn.p, 0, (size_t)L * pad * d * sizeof(float)));
    CHK(st.cnn2.ensure((size_t)L * pad * d * sizeof(float)));
    CHK(clear_sync(st.cnn2.p, 0, (size_t)L * pad * d * sizeof(float)));
    if (e->cfg.model_kind == 2)     // planar caches of the grouped layers: rows behind the last key must read as zero
        CHK(clear_sync(st.att.p, 0, (size_t)L * st.cap * 2 * d * sizeof(float)));
    st.offset = 0;
    st.offset_r = 0;
    st.history = -1;
    st.cache_t1 = 0;
    st.first_half = 0;
    st.open = true;
    *stream_id = id;
    return 0;
}

static int stream_of(masr_engine* e, int id, Stream** out) {
    if (!e) return fail("null engine");
    if (id < 0 || id >= (int)e->streams.size() || !e->streams[id].open) return fail("bad stream id");
    *out = &e->streams[id];
    return 0;
}

int masr_stream_reset(masr_engine* e, int32_t stream_id) {
    Stream* st;
    CHK(stream_of(e, stream_id, &st));
    ENTER(e);
    const int d = e->cfg.d_model, L = e->cfg.num_blocks, pad = e->cfg.cnn_kernel - 1;
    HIPCHK(hipDeviceSynchronize());
    CHK(clear_sync(st->cnn.p, 0, (e->cfg.model_kind == 3 ? (size_t)L * 2 * d : (size_t)L * pad * d) * sizeof(float)));
    if (e->cfg.model_kind == 2) CHK(clear_sync(st->att.p, 0, (size_t)L * st->cap * 2 * d * sizeof(float)));
    st->offset = 0;
    st->offset_r = 0;
    st->cache_t1 = 0;
    st->first_half = 0;
    return 0;
}

int masr_stream_close(masr_engine* e, int32_t stream_id) {
    Stream* st;
    CHK(stream_of(e, stream_id, &st));
    ENTER(e);
    HIPCHK(hipDeviceSynchronize());
    st->att.release();
    st->cnn.release();
    st->cnn2.release();
    st->open = false;
    return 0;
}

int masr_stream_set_history(masr_engine* e, int32_t stream_id, int32_t required_cache_size) {
    Stream* st;
    CHK(stream_of(e, stream_id, &st));
    if (required_cache_size >= 0 && e->cfg.model_kind == 3)
        return fail("required_cache_size: DeepSpeech2 streams carry an LSTM state, not an attention cache");
    st->history = required_cache_size;
    return 0;
}

int masr_encoder_frames(masr_engine* e, int32_t feature_frames, int32_t* encoder_frames) {
    if (!e || !encoder_frames) return fail("null argument");
    const int Tsub = sub_frames(e->input_layer, feature_frames);
    const bool halved = e->cfg.model_kind == 2 && e->stride_idx >= 0;
    *encoder_frames = halved ? (Tsub + 1) / 2 : Tsub;
    return 0;
}

int masr_frame_reduction(masr_engine* e, int32_t* feature_frames_per_encoder_frame) {
    if (!e || !feature_frames_per_encoder_frame) return fail("null argument");
    // the subsampling front end (4 / 6 / 8; DeepSpeech2's two stride-2 convs: 4), once more halved by the Efficient Conformer's
    // stride layer; the Squeezeformer's time reduction is undone by its recovery layer
    const int r = sub_rate(e->input_layer);
    *feature_frames_per_encoder_frame = e->cfg.model_kind == 2 && e->stride_idx >= 0 ? 2 * r : r;
    return 0;
}

int masr_engine_info(masr_engine* e, int32_t* device_id, int32_t* n_mels, int32_t* vocab_size) {
    if (!e) return fail("null engine");
    if (device_id) *device_id = e->cfg.device_id;
    if (n_mels) *n_mels = e->cfg.n_mels;
    if (vocab_size) *vocab_size = e->cfg.vocab_size;
    return 0;
}

int masr_stream_offset(masr_engine* e, int32_t stream_id, int32_t* offset) {
    Stream* st;
    CHK(stream_of(e, stream_id, &st));
    *offset = st->offset;
    return 0;
}

int masr_stream_room(masr_engine* e, int32_t stream_id, int32_t* frames_left) {
    if (!frames_left) return fail("null argument");
    Stream* st;
    CHK(stream_of(e, stream_id, &st));
    // (the Efficient-Conformer's grouped layers pad a chunk to a multiple of the group size before the room check of
    //  masr_encode_chunk: that slack is taken off HERE, for that family only, so that a caller compares plain frame counts)
    const int slack = e->cfg.model_kind == 2 ? std::max(0, e->group_size) : 0;
    *frames_left = std::max(0, st->cap - st->offset - slack);
    return 0;
}

int masr_stream_cache_len(masr_engine* e, int32_t stream_id, int32_t* cache_len) {
    Stream* st;
    CHK(stream_of(e, stream_id, &st));
    *cache_len = st->cache_t1;
    return 0;
}

}  // extern "C"

// forward_chunk's cache bookkeeping (conformer/encoder.py:390-410, squeezeformer/encoder.py:288-297,338-347,
// efficient_conformer/encoder.py:316-336,365-381), as a window into append-only caches: a chunk of T0 input-rate frames attends
// over the last cache_t1 cached frames + itself; afterwards the cache is cut at next_cache_start.
struct ChunkWindow {
    int cache_t1, first_full;    // cached frames attended over; absolute index of the first of them (= positional index of key 0)
    int next_cache_t1, ncs;      // after the step
};
static ChunkWindow chunk_window(const Stream& st, int T0) {
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
static int half_rate_window(const Stream& st, int want, int* first, int* count) {
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
static AttSeq interleaved_seq(const float* q, float* cache, int d, int first, int ncached, int Tl, float* out, int pos0, int q_abs0) {
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
static std::vector<float*> cnn_cache_table(const std::vector<Stream*>& st, int L, size_t layer_floats) {
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
static int upload_chunk_tables(masr_engine* e, hipStream_t s, const std::vector<AttSeq>& hs, const std::vector<float*>& hp,
                               void* third_dev = nullptr, const void* third = nullptr, size_t third_bytes = 0) {
    CHK(e->stage.begin(sizeof(AttSeq) * hs.size() + sizeof(float*) * hp.size() + third_bytes + 64));
    CHK(e->stage.push(e->attseq.p, hs.data(), sizeof(AttSeq) * hs.size(), s));
    CHK(e->stage.push(e->cnnptrs.p, hp.data(), sizeof(float*) * hp.size(), s));
    if (third_bytes) CHK(e->stage.push(third_dev, third, third_bytes, s));
    CHK(e->stage.end(s));
    return 0;
}

// the CTC head on the step's encoder rows: probabilities where the caller asks for them, argmax and its probability always
static int chunk_ctc(masr_engine* e, hipStream_t s, const float* enc, int rows, float* probs, int32_t* argmax, float* maxprob) {
    if (e->cfg.vocab_size > 16384) return fail(kVocabRefusal);
    return ctc_head(e, enc, rows, probs, probs ? 1 : 0, argmax, maxprob, s);
}

// behind a step of T0 input-rate frames (Tr at the half rate) of the Squeezeformer or the Efficient Conformer
static void advance_half_rate(std::vector<Stream*>& st, const std::vector<ChunkWindow>& win, int T0, int Tr) {
    for (size_t i = 0; i < st.size(); ++i) {
        st[i]->offset += T0;
        st[i]->offset_r += Tr;
        st[i]->cache_t1 = win[i].next_cache_t1;
        st[i]->first_half += win[i].ncs / 2;
        std::swap(st[i]->cnn, st[i]->cnn2);
    }
}

// a stream given twice in one call would be advanced twice from one state
static int distinct_streams(const std::vector<Stream*>& st) {
    for (size_t i = 0; i < st.size(); ++i)
        for (size_t j = 0; j < i; ++j)
            if (st[i] == st[j]) return fail("duplicate stream id in one call");
    return 0;
}

// Squeezeformer chunk step (streaming-trained build), n streams in lock-step: SqueezeformerEncoder.forward_chunk
// (squeezeformer/encoder.py:240-362) with required_cache_size < 0.  Every layer keeps its key/value cache at its OWN frame
// rate (the reference stores the half-rate layers repeat-interleaved and reads every second entry back, :338-347), the cnn
// cache holds the last K-1 adaptive-scaled input rows of the conv module.  TimeReductionLayerStream (k = 1, stride 2) and the
// recovery are chunk-local.
static int encode_chunk_squeezeformer(masr_engine* e, hipStream_t s, std::vector<Stream*>& st, const float* feats, int Tc,
                                      float* probs_dev, int32_t* argmax_dev, float* maxprob_dev) {
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
        {
            RowGemmArgs g = rg_args(x, d, w.wqkv, w.bqkv, e->qkv.as<float>(), 3 * d, M, 3 * d);
            g.lnw = w.att_s; g.lnb = w.att_b; g.kv_seqs = seqs; g.kv_tq = Tq;
            rowgemm(e, s, RG_PRO_AFFINE, RG_EPI_STORE, g);
        }
        launch_attention(seqs, n, Tq, H, 3 * d, 2 * d, w.ptab, w.pos_u, w.pos_v, 0, reduced(l) ? 2 : 1, s, 256, ATT_REL_POS);
        {
            RowGemmArgs g = rg_args(e->att.as<float>(), d, w.wo, w.bo, x, d, M, d);
            g.R = x; g.ldr = d;
            rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_RESID, g);
        }
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
        {
            RowGemmArgs g = rg_args(e->dwo.as<float>(), d, w.pw2_w, w.pw2_b, x, d, M, d);
            g.R = x; g.ldr = d;
            rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_RESID, g);
        }
        launch_layernorm(x, w.ln3_w, w.ln3_b, x, M, 1e-5f, 0, 0, nullptr, s);
        CHK(ffn(e, s, ffn_sqz2(w, M, l == L - 1 ? e->enc.as<float>() : x)));
    }
    CHK(chunk_ctc(e, s, e->enc.as<float>(), n * T0, probs_dev, argmax_dev, maxprob_dev));
    advance_half_rate(st, win, T0, Tr);
    return 0;
}

// Efficient-Conformer chunk step, n streams in lock-step: EfficientConformerEncoder.forward_chunk
// (efficient_conformer/encoder.py:267-392) with required_cache_size < 0.  Grouped layers keep PLANAR key / value caches at the
// input frame rate (the flat regrouping runs over cache + chunk), layers behind the stride layer keep interleaved k|v rows
// at half the rate (the reference stores them repeat-interleaved, :370); cnn caches hold each layer's own K-1 rows.
static int encode_chunk_efficient(masr_engine* e, hipStream_t s, std::vector<Stream*>& st, const float* feats, int Tc,
                                  float* probs_dev, int32_t* argmax_dev, float* maxprob_dev) {
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
            {
                RowGemmArgs g = rg_args(e->attp.as<float>(), d, w.wo, w.bo, x, d, M, d);
                g.R = x; g.ldr = d; g.a_seq_t = Tq; g.a_seq_stride = Tpad;
                rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_RESID, g);
            }
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
            {
                RowGemmArgs g = rg_args(e->dwo.as<float>(), d, w.pw2_w, w.pw2_b, x, d, M, d);
                g.R = e->xsave.as<float>(); g.ldr = d;
                rowgemm(e, s, RG_PRO_PLAIN, RG_EPI_RESID, g);
            }
        } else {
            CHK(conv_module_stream(e, s, w, n, Tq, cptr, cptr + (size_t)L * n, K));
        }
        CHK(ffn(e, s, ffn_final(w, M, x)));
    }
    CHK(e->enc.ensure((size_t)n * T2 * d * sizeof(float)));
    launch_layernorm(x, e->after_w, e->after_b, e->enc.as<float>(), n * T2, 1e-5f, 0, 0, nullptr, s);
    CHK(chunk_ctc(e, s, e->enc.as<float>(), n * T2, probs_dev, argmax_dev, maxprob_dev));
    advance_half_rate(st, win, T0, T2);
    return 0;
}

// DeepSpeech2 chunk step, n streams in lock-step (deepspeech2/model.py:79-108): chunk conv + LSTM stack with carried (h, c)
static int encode_chunk_ds2(masr_engine* e, hipStream_t s, std::vector<Stream*>& st, const float* feats_dev, int Tc,
                            float* probs_dev, int32_t* argmax_dev, float* maxprob_dev) {
    const int n = (int)st.size();
    int Tq = 0;
    const int Tq3 = ((Tc - 1) / 2 - 1) / 2;
    if (Tq3 <= 0) return fail("chunk too short");
    CHK(e->enc.ensure((size_t)n * Tq3 * enc_dim(e) * sizeof(float)));
    CHK(ds2_forward(e, s, feats_dev, nullptr, n, Tc, e->enc.as<float>(), st.data(), &Tq));
    CHK(chunk_ctc(e, s, e->enc.as<float>(), n * Tq, probs_dev, argmax_dev, maxprob_dev));
    for (int i = 0; i < n; ++i) st[i]->offset += Tq;
    return 0;
}

// Conformer chunk step, n streams in lock-step: ConformerEncoder.forward_chunk (conformer/encoder.py:355-420), on the fused
// kernels or (is_wide) on the width-generic layer.  Unlike the other families' steps this one has never refused a stream id given
// twice in one call (distinct_streams): whether it should is a behaviour decision of its own.
static int encode_chunk_conformer(masr_engine* e, hipStream_t s, std::vector<Stream*>& st, const float* feats_dev, int Tc,
                                  float* probs_dev, int32_t* argmax_dev, float* maxprob_dev) {
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
    CHK(chunk_ctc(e, s, e->enc.as<float>(), M, probs_dev, argmax_dev, maxprob_dev));
    for (int i = 0; i < n; ++i) {
        st[i]->cache_t1 = chunk_window(*st[i], Tq).next_cache_t1;
        st[i]->offset += Tq;
        std::swap(st[i]->cnn, st[i]->cnn2);
    }
    return 0;
}

extern "C" {

int masr_encode_chunk(masr_engine* e, const int32_t* stream_ids, int32_t n, const float* feats_dev, int32_t Tc,
                      float* probs_dev, int32_t* argmax_dev, float* maxprob_dev, void* stream) {
    if (!e || !e->finalized) return fail("engine not finalized");
    ENTER(e);
    CallGuard call_guard(e, (hipStream_t)stream);
    if (n <= 0) return fail("no streams");
    hipStream_t s = (hipStream_t)stream;
    std::vector<Stream*> st(n);
    for (int i = 0; i < n; ++i) CHK(stream_of(e, stream_ids[i], &st[i]));
    // (the Conformer step, model_kind 0, has never had this check and gets none here: whether it should is a behaviour decision)
    if (e->cfg.model_kind != 0) CHK(distinct_streams(st));
    switch (e->cfg.model_kind) {
    case 1: return encode_chunk_squeezeformer(e, s, st, feats_dev, Tc, probs_dev, argmax_dev, maxprob_dev);
    case 2: return encode_chunk_efficient(e, s, st, feats_dev, Tc, probs_dev, argmax_dev, maxprob_dev);
    case 3: return encode_chunk_ds2(e, s, st, feats_dev, Tc, probs_dev, argmax_dev, maxprob_dev);
    default: return encode_chunk_conformer(e, s, st, feats_dev, Tc, probs_dev, argmax_dev, maxprob_dev);
    }
}

int masr_stream_export_cache(masr_engine* e, int32_t stream_id, float* att_dev, float* cnn_dev, void* stream) {
    Stream* st;
    CHK(stream_of(e, stream_id, &st));
    ENTER(e);
    hipStream_t s = (hipStream_t)stream;
    const int d = e->cfg.d_model, L = e->cfg.num_blocks, pad = e->cfg.cnn_kernel - 1, H = e->cfg.heads;
    if (e->cfg.model_kind == 3) {       // att_dev <- h [L][rnn_size], cnn_dev <- c [L][rnn_size] (GRU: h again)
        for (int l = 0; l < L; ++l) {
            const float* hc = st->cnn.as<float>() + (size_t)l * 2 * d;
            if (att_dev) HIPCHK(hipMemcpyAsync(att_dev + (size_t)l * d, hc, sizeof(float) * d, hipMemcpyDeviceToDevice, s));
            if (cnn_dev) HIPCHK(hipMemcpyAsync(cnn_dev + (size_t)l * d, hc + d, sizeof(float) * d, hipMemcpyDeviceToDevice, s));
        }
        return 0;
    }
    // what the reference's (trimmed) cache tensor holds: the last t = cache_t1 input-rate frames [L, H, t, 2 dk]
    const int t = st->cache_t1;
    if (att_dev && t > 0) {
        const int first = st->offset - t;
        if (e->cfg.model_kind == 2) {     // planar grouped layers; half-rate layers repeat-interleaved, the LAST t entries (:370,380)
            for (int l = 0; l < L; ++l) {
                const float* base = st->att.as<float>() + (size_t)l * st->cap * 2 * d;
                float* o = att_dev + (size_t)l * t * 2 * d;
                if (layer_grouped(e, l))
                    launch_export_att_planar(base + (size_t)first * d, base + (size_t)st->cap * d + (size_t)first * d, o, H, t, d / H, s);
                else if (l > e->stride_idx)
                    launch_export_att(base, o, 1, H, st->cap, t, d / H, s, 2, 2 * st->offset_r - t);
                else
                    launch_export_att(base + (size_t)first * 2 * d, o, 1, H, st->cap, t, d / H, s);
            }
        } else if (e->cfg.model_kind == 1) {     // half-rate layers: every kept entry twice, the FIRST t of them (encoder.py:345-351)
            for (int l = 0; l < L; ++l) {
                const float* base = st->att.as<float>() + (size_t)l * st->cap * 2 * d;
                if (l >= e->reduce_idx && l < e->recover_idx)
                    launch_export_att(base, att_dev + (size_t)l * t * 2 * d, 1, H, st->cap, t, d / H, s, 2, 2 * st->first_half);
                else
                    launch_export_att(base + (size_t)first * 2 * d, att_dev + (size_t)l * t * 2 * d, 1, H, st->cap, t, d / H, s);
            }
        } else {
            launch_export_att(st->att.as<float>() + (size_t)first * 2 * d, att_dev, L, H, st->cap, t, d / H, s);
        }
    }
    if (cnn_dev && e->cfg.model_kind == 2) {       // each layer's own K-1 rows, left-padded with zeros to cnn_module_kernel - 1
        HIPCHK(hipMemsetAsync(cnn_dev, 0, (size_t)L * pad * d * sizeof(float), s));
        for (int l = 0; l < L; ++l)
            launch_export_cnn_layer(st->cnn.as<float>() + (size_t)l * pad * d, cnn_dev + (size_t)l * pad * d, layer_kernel(e, l) - 1,
                                    pad, d, s);
    } else if (cnn_dev) {
        launch_export_cnn(st->cnn.as<float>(), cnn_dev, L, pad, d, s);
    }
    LAUNCHCHK();
    return 0;
}

// ---- single ops -------------------------------------------------------------------------------------------

int masr_op_layernorm(masr_engine* e, const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev,
                      int32_t M, float eps, void* stream) {
    if (!e) return fail("null engine");
    ENTER(e);
    launch_layernorm(x_dev, w_dev, b_dev, y_dev, M, eps, 0, 0, nullptr, (hipStream_t)stream);
    LAUNCHCHK();
    return 0;
}

int masr_op_gemm(masr_engine* e, const float* a_dev, const float* w_dev, const float* bias_dev, const float* res_dev,
                 float* c_dev, int32_t M, int32_t N, int32_t K, int32_t act, float alpha, void* stream) {
    // (refused before the engine is touched: an unknown value used to run as "none")
    if (!gemm_act_valid(act))
        return fail("masr_op_gemm: act = " + std::to_string(act) + " is not an activation: 0 = none, 1 = relu, 2 = silu, 3 = gelu, "
                    "4 = tanh, 5 = hardtanh, 6 = selu");
    if (!e) return fail("null engine");
    ENTER(e);
    CallGuard call_guard(e, (hipStream_t)stream);
    if (K % 32) return fail("K must be a multiple of 32");
    gemm(e, (hipStream_t)stream, a_dev, K, w_dev, bias_dev, c_dev, N, M, N, K, act, alpha, res_dev, N);
    LAUNCHCHK();
    return 0;
}

}  // extern "C"

// masr_op_attention (pos_mode ATT_REL_POS) and masr_op_attention_plain (ATT_NO_POS: no table, no biases, group 1)
static int op_attention(masr_engine* e, int pos_mode, const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev,
                      const float* ptab_dev, int32_t n_pos, const float* bias_u_dev, const float* bias_v_dev, int32_t nseq,
                      const int64_t* q_off, const int64_t* k_off, const int64_t* v_off, const int64_t* out_off, const int32_t* nq,
                      const int32_t* nk, const int32_t* klen, const int32_t* pos0, const int32_t* q_abs0, int32_t heads,
                      int32_t q_stride, int32_t kv_stride, int32_t chunk_size, int32_t pos_stride, int32_t group, int32_t t_true,
                      void* stream) {
    // every refusal comes before the engine is touched: none of them needs a device
    const bool pos = pos_mode == ATT_REL_POS;
    if (!q_dev || !k_dev || !v_dev || !out_dev || (pos && (!ptab_dev || !bias_u_dev || !bias_v_dev)) || !q_off || !k_off || !v_off ||
        !out_off || !nq || !nk || !klen || !pos0 || !q_abs0)
        return fail("masr_op_attention: null argument");
    if (nseq <= 0) return fail("masr_op_attention: nseq must be positive");
    if (heads != 4 && heads != 8) return fail("masr_op_attention: heads must be 4 or 8");
    if (group != 1 && group != 3) return fail("masr_op_attention: group must be 1 or 3");
    const int w = heads * 64;
    if (q_stride < w || kv_stride < w) return fail("masr_op_attention: q_stride and kv_stride must be at least heads * 64");
    if (group == 3 && (heads != 4 || q_stride != 3 * w || kv_stride != 3 * w))
        return fail("masr_op_attention: the grouped kernels take 4 heads and planar rows of heads * 192 floats");
    if (chunk_size < 0 || pos_stride < 1 || n_pos < 0 || t_true < 0)
        return fail("masr_op_attention: chunk_size, n_pos and t_true must not be negative, pos_stride at least 1");
    if ((q_stride | kv_stride) & 3) return fail("masr_op_attention: strides must be multiples of 4 floats");
    for (const void* p : {(const void*)q_dev, (const void*)k_dev, (const void*)v_dev, (const void*)out_dev, (const void*)ptab_dev,
                          (const void*)bias_u_dev, (const void*)bias_v_dev})
        if ((uintptr_t)p & 15) return fail("masr_op_attention: device buffers must be 16-byte aligned");
    int max_nq = 0;
    std::vector<AttSeq> hs((size_t)nseq);
    for (int b = 0; b < nseq; ++b) {
        if (nq[b] < 0 || nk[b] < 0 || klen[b] < 0 || pos0[b] < 0 || q_abs0[b] < 0 || q_off[b] < 0 || k_off[b] < 0 || v_off[b] < 0 ||
            out_off[b] < 0)
            return fail("masr_op_attention: negative count or offset in sequence " + std::to_string(b));
        if (klen[b] > nk[b]) return fail("masr_op_attention: klen > nk in sequence " + std::to_string(b));
        if ((q_off[b] | k_off[b] | v_off[b] | out_off[b]) & 3)
            return fail("masr_op_attention: offsets must be multiples of 4 floats");
        if ((int64_t)nk[b] * kv_stride >= ((int64_t)1 << 30))
            return fail("masr_op_attention: the key rows of one sequence must span less than 4 GiB");
        // the last positional row a kernel may read: row pos0 + pos_stride * (nk - 1); grouped: frame pos0 + min(t_true, 3 nk) - 1
        const int64_t last = group == 3 ? (int64_t)pos0[b] + std::min<int64_t>(t_true, 3 * (int64_t)nk[b]) - 1
                                        : (int64_t)pos0[b] + (int64_t)pos_stride * (nk[b] - 1);
        if (pos && nk[b] > 0 && last >= n_pos) return fail("masr_op_attention: the positional table is too short for sequence " + std::to_string(b));
        AttSeq& a = hs[(size_t)b];
        a.q = q_dev + q_off[b];
        a.k = k_dev + k_off[b];
        a.v = v_dev + v_off[b];
        a.out = out_dev + out_off[b];
        a.nq = nq[b];
        a.nk = nk[b];
        a.klen = klen[b];
        a.pos0 = pos0[b];
        a.q_abs0 = q_abs0[b];
        a.pad_ = 0;
        max_nq = std::max(max_nq, nq[b]);
    }
    if (!e) return fail("null engine");
    ENTER(e);
    hipStream_t s = (hipStream_t)stream;
    struct Table {
        AttSeq* p = nullptr;
        ~Table() { if (p) (void)hipFree(p); }
    } tab;
    HIPCHK(hipMalloc((void**)&tab.p, hs.size() * sizeof(AttSeq)));
    HIPCHK(hipMemcpyAsync(tab.p, hs.data(), hs.size() * sizeof(AttSeq), hipMemcpyHostToDevice, s));
    {
        ProfScope ps(e, s, PROF_ATT, 6.0 * w * (double)max_nq * max_nq * nseq);
        if (group > 1) launch_attention_grouped(tab.p, nseq, max_nq, heads, group, ptab_dev, t_true, bias_u_dev, bias_v_dev, s, chunk_size);
        else launch_attention(tab.p, nseq, max_nq, heads, q_stride, kv_stride, ptab_dev, bias_u_dev, bias_v_dev, chunk_size, pos_stride, s, w, pos_mode);
    }
    LAUNCHCHK();
    HIPCHK(hipStreamSynchronize(s));       // the table is freed, and the host copy leaves scope, behind the kernel
    return 0;
}

extern "C" {

int masr_op_attention(masr_engine* e, const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev,
                      const float* ptab_dev, int32_t n_pos, const float* bias_u_dev, const float* bias_v_dev, int32_t nseq,
                      const int64_t* q_off, const int64_t* k_off, const int64_t* v_off, const int64_t* out_off, const int32_t* nq,
                      const int32_t* nk, const int32_t* klen, const int32_t* pos0, const int32_t* q_abs0, int32_t heads,
                      int32_t q_stride, int32_t kv_stride, int32_t chunk_size, int32_t pos_stride, int32_t group, int32_t t_true,
                      void* stream) {
    return op_attention(e, ATT_REL_POS, q_dev, k_dev, v_dev, out_dev, ptab_dev, n_pos, bias_u_dev, bias_v_dev, nseq, q_off, k_off, v_off,
                        out_off, nq, nk, klen, pos0, q_abs0, heads, q_stride, kv_stride, chunk_size, pos_stride, group, t_true, stream);
}

int masr_op_attention_plain(masr_engine* e, const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, int32_t nseq,
                            const int64_t* q_off, const int64_t* k_off, const int64_t* v_off, const int64_t* out_off,
                            const int32_t* nq, const int32_t* nk, const int32_t* klen, const int32_t* q_abs0, int32_t heads,
                            int32_t q_stride, int32_t kv_stride, int32_t chunk_size, int32_t pos_stride, void* stream) {
    if (nseq <= 0) return fail("masr_op_attention: nseq must be positive");
    const std::vector<int32_t> pos0((size_t)nseq, 0);         // (no positional rows: nothing is read at them)
    return op_attention(e, ATT_NO_POS, q_dev, k_dev, v_dev, out_dev, nullptr, 0, nullptr, nullptr, nseq, q_off, k_off, v_off, out_off, nq,
                        nk, klen, pos0.data(), q_abs0, heads, q_stride, kv_stride, chunk_size, pos_stride, 1, 0, stream);
}

int masr_select_lane(masr_engine* e, int32_t lane) {
    if (!e) return fail("null engine");
    if (lane < 0 || lane >= MASR_LANES) return fail("masr_select_lane: lane must be in [0, " + std::to_string(MASR_LANES) + ")");
    if (lane == e->lane) return 0;
    EngineWs& active = *e;                   // park the active set, bring the lane's own in (pointers and sizes only)
    e->parked[e->lane] = active;
    active = e->parked[lane];
    e->parked[lane] = EngineWs();
    e->lane = lane;
    return 0;
}

int masr_side_stream(masr_engine* e, int32_t kind, void** stream_out) {
    if (!e || !stream_out) return fail("null argument");
    if (kind < 0 || kind >= MASR_SIDE_STREAMS)
        return fail("masr_side_stream: kind must be 0 / 1 (prefix search), 2 (preparation), 3 (copy) or 4 (second encoder lane)");
    SideStreams* ss = nullptr;
    if (side_streams_of(e->cfg.device_id, &ss)) return 1;
    *stream_out = (void*)ss->s[kind];
    return 0;
}

int masr_debug_set(masr_engine* e, int32_t key, int32_t value) {
    if (!e) return fail("null engine");
    const KnobInfo* k = knob_find(key);
    if (k) {
        if (!MASR_EXPERIMENTS && k->experimental && value != 0)
            return fail("masr_debug_set: this key selects an experimental kernel that is not in this build (MASR_BUILD_EXPERIMENTS=1)");
        knob_set(key, value);
    } else if (key == 38) e->skip_padding = value;
    else if (key == 16) { e->prof_stride = value > 1 ? value : 1; e->prof_seen = 0; }
    else if (key == 2) {            // beam search phase profile of workgroup 0: value 1 = on, 0 = print + off
        if (value) {
            if (!e->beam_prof) {
                void* p = nullptr;
                HIPCHK(hipMalloc(&p, 16 * sizeof(long long)));
                e->owned.push_back(p);
                e->beam_prof = (long long*)p;
            }
        } else if (e->beam_prof) {
            long long h[16];
            HIPCHK(hipMemcpy(h, e->beam_prof, sizeof(h), hipMemcpyDeviceToHost));
            fprintf(stderr, "beam phases (cycles, last workgroup): setup+hash %lld  extensions %lld  prefixes+count %lld  select %lld  compact %lld\n",
                    h[0], h[1], h[2], h[3], h[4]);
            fprintf(stderr, "  narrow step (%lld frames): tables+candidates %lld  hash+contexts %lld  children+scorer table %lld  extensions %lld  "
                    "prefixes+select %lld  scan %lld  survivors %lld  new prefixes %lld\n", h[5], h[6], h[7], h[8], h[9], h[10], h[11], h[12], h[13]);
            if (h[15] > 0) fprintf(stderr, "  wide step (%lld frames): %.1f distinct scorer contexts per frame\n", h[15], (double)h[14] / (double)h[15]);
            e->beam_prof = nullptr;
        }
    }
    else return fail("unknown debug key");
    return 0;
}

int masr_debug_reset(masr_engine* e) {
    if (!e) return fail("null engine");
    knobs_reset();
    e->skip_padding = 7;
    e->prof_stride = 1;
    e->prof_seen = 0;
    return 0;
}

int masr_debug_key_info(int32_t index, int32_t* key, int32_t* default_value, int32_t* experimental, const char** name) {
    const KnobInfo* k = knob_info(index);
    if (!k) return 1;
    if (key) *key = k->key;
    if (default_value) *default_value = knob_default(*k);
    if (experimental) *experimental = k->experimental;
    if (name) *name = k->name;
    return 0;
}

int masr_ffn_plan(int32_t d_model, int32_t d_ff, int32_t m, const int32_t* ask, const int32_t* overrides, int32_t n_overrides,
                  int32_t* plan) {
    if (!ask || !plan || n_overrides < 0 || (n_overrides && !overrides)) return fail("masr_ffn_plan: null argument");
    if (d_ff <= 0 || d_ff % 128 || m <= 0) return fail("masr_ffn_plan: d_ff must be a positive multiple of 128 and m positive");
    Knobs k;                       // the defaults; the process's switches are neither read nor written
    for (int i = 0; i < n_overrides; ++i)
        if (!knob_set(overrides[2 * i], overrides[2 * i + 1], k))
            return fail("masr_ffn_plan: no process-wide switch has key " + std::to_string(overrides[2 * i]));
    const FfnPlan p = ffn_plan(k, d_model, d_ff, m, {ask[0], ask[1], ask[2], ask[3], ask[4]});
    const int32_t out[9] = {p.kernel, p.nsplit, p.cpb, p.ny, p.packed, p.tail_in_kernel, p.head_in_kernel, p.split_head, p.prof};
    std::copy(out, out + 9, plan);
    return 0;
}

int masr_profile_select(masr_engine* e, int32_t kind) {
    if (!e) return fail("null engine");
    e->prof_kind = kind;
    return 0;
}

int masr_profile_read(masr_engine* e, double* total_ms, int64_t* launches, double* flops, int32_t reset) {
    if (!e) return fail("null engine");
    ENTER(e);
    double tot = 0.0;
    for (size_t i = 0; i < e->prof_used; ++i) {
        HIPCHK(hipEventSynchronize(e->prof_events[i].second));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e->prof_events[i].first, e->prof_events[i].second));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = (int64_t)e->prof_used;
    if (flops) *flops = e->prof_flops;
    if (reset) {
        e->prof_used = 0;
        e->prof_flops = 0.0;
    }
    return 0;
}

}  // extern "C"
