// libmasr_hip.so -- engine: error state, weight store, engine and stream lifecycle, and the finalize / encode entry points of
// the C ABI (include/masr_hip.h) as dispatchers to the model families' files (map: engine_state.h).  Host-side only; every kernel
// lives in the sibling .hip files and is launched on the caller's stream.
#include <stdlib.h>

#include <mutex>

#include "engine_encoder.h"

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

int up(masr_engine* e, const std::string& name, std::vector<int64_t> shape, float** out) {
    const HostTensor* t;
    CHK(get(e, name, shape, &t));
    return upload(e, t->v, out);
}

// a module's weight of `shape` and its bias of the leading dimension: key + ".weight", then key + ".bias"
int up_wb(masr_engine* e, const std::string& key, std::vector<int64_t> shape, float** w, float** b) {
    const int64_t n = shape[0];
    CHK(up(e, key + ".weight", shape, w));
    return up(e, key + ".bias", {n}, b);
}

// fragment-ordered copy of a [N, 256] weight matrix (rows padded to a multiple of 256 with zeros): launch_pack_rows_pc's order,
// or launch_pack_rows16's (PACK_ROWS16)
const float* packed_rows_of(masr_engine* e, const float* W, int N, hipStream_t s, PackLayout layout) {
    const int Np = (N + 255) / 256 * 256;
    const PackedW* pk = packed_of(e, layout, W, (size_t)Np * 256 * sizeof(float), 0, s, [&](const PackedW& p, hipStream_t st) {
        (layout == PACK_ROWS16 ? launch_pack_rows16 : launch_pack_rows_pc)(W, p.a.as<float>(), Np, st, N);
    });
    return pk ? pk->a.as<float>() : nullptr;
}

// fragment-order copies of an FFN's two weight matrices, cached per W1 pointer: ffn_pc.hip's layout (PACK_FFN_PC,
// launch_pack_ffn_pc), the 16-row kernel's (PACK_FFN16, launch_pack_ffn16) or the two-chain kernel's (PACK_FFN_DUAL, launch_pack_ffn_dual)
int packed_ffn_of(masr_engine* e, const float* w1, const float* w2, hipStream_t s, const float** p1, const float** p2,
                  PackLayout layout, PackFfnFn pack) {
    const size_t bytes = (size_t)e->cfg.d_ff * e->cfg.d_model * sizeof(float);
    const PackedW* pk = packed_of(e, layout, w1, bytes, bytes, s, [&](const PackedW& p, hipStream_t st) {
        pack(w1, w2, p.a.as<float>(), p.b.as<float>(), e->cfg.d_ff, st);
    });
    if (!pk) return 1;
    *p1 = pk->a.as<float>();
    *p2 = pk->b.as<float>();
    return 0;
}
}  // namespace masr

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
    // layer layouts (the header states the accepted ranges under reserved[5]): the forward passes branch on these indices without
    // looking at them again, so everything outside is refused here, before anything is allocated
    if (cfg->model_kind == 1) {
        const int L = cfg->num_blocks, r = cfg->reserved[0], c = cfg->reserved[1];
        if (r < -1 || r >= L)
            return fail("squeezeformer: reduce_idx (masr_config.reserved[0]) = " + std::to_string(r) + " is not supported: -1 (null) or a "
                        "layer in [0, num_blocks = " + std::to_string(L) + ")");
        if (r >= 0 && (c < r || c >= L))
            return fail("squeezeformer: recover_idx (masr_config.reserved[1]) = " + std::to_string(c) + " with reduce_idx = " +
                        std::to_string(r) + " is not supported: a layer in [reduce_idx, num_blocks = " + std::to_string(L) + "); the "
                        "reference fails on a recovery in front of the reduction, and with recover_idx null (-1) or >= num_blocks its "
                        "output stays at half the frame rate, which this engine does not implement");
    }
    if (cfg->model_kind == 2) {
        const int L = cfg->num_blocks, s = cfg->reserved[0], g = cfg->reserved[1];
        if (s < 0 || s >= L)
            return fail("efficient_conformer: stride_layer_idx (masr_config.reserved[0]) = " + std::to_string(s) + " is not supported: "
                        "one stride layer in [0, num_blocks = " + std::to_string(L) + ")");
        if (g < 0 || g > s + 1)
            return fail("efficient_conformer: group_layer_idx (masr_config.reserved[1] = its length) = " + std::to_string(g) +
                        " leading grouped layers with stride_layer_idx = " + std::to_string(s) + " is not supported: 0 to "
                        "stride_layer_idx + 1 (grouped attention after the stride layer is not implemented)");
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

// device lengths in conv2d units for the conv2d6 / conv2d8 front-ends (nullptr in, or conv2d: lens itself).  The encoder's kernels
// treat frame t of a sequence as padding when mstride * t >= lens (mstride 4 at the conv2d rate); with rate r the reference keeps
// frame t iff r * t < len, i.e. iff t < ceil(len / r) -- the same test on 4 * ceil(len / r)
static const int* sub_lens(masr_engine* e, hipStream_t s, const int* lens, int B) {
    if (!lens || e->input_layer == IL_CONV2D || B <= 0) return lens;
    if (e->sublens.ensure(sizeof(int) * B)) return nullptr;
    launch_sub_lens(lens, B, sub_rate(e->input_layer), e->sublens.as<int>(), s);
    return e->sublens.as<int>();
}

int masr_finalize(masr_engine* e, void* stream) {
    if (!e) return fail("null engine");
    // the decoder first: the model's own finalize drops the host copies of every tensor when it is done
    if (e->dec.enabled) CHK(finalize_decoder(e));
    HIPCHK(hipSetDevice(e->cfg.device_id));
    hipStream_t s = (hipStream_t)stream;
    const int kind = e->cfg.model_kind;       // (0 and 2: the Efficient Conformer shares the Conformer's key names)
    CHK(kind == 1 ? finalize_squeezeformer(e, s) : kind == 3 ? finalize_ds2(e) : finalize_conformer(e, s));
    if (kind != 3) HIPCHK(hipStreamSynchronize(s));      // the finalize-time launches (ptab, gconst, packing) are over when the call returns
    e->host.clear();
    e->finalized = true;
    return 0;
}

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

// a stream given twice in one call would be advanced twice from one state
static int distinct_streams(const std::vector<Stream*>& st) {
    for (size_t i = 0; i < st.size(); ++i)
        for (size_t j = 0; j < i; ++j)
            if (st[i] == st[j]) return fail("duplicate stream id in one call");
    return 0;
}

// the chunk step of both entries: masr_encode_chunk (enc_out_dev == nullptr) and masr_encode_chunk_enc
static int encode_chunk_any(masr_engine* e, const int32_t* stream_ids, int32_t n, const float* feats_dev, int32_t Tc, float* probs_dev,
                            int32_t* argmax_dev, float* maxprob_dev, float* enc_out_dev, void* stream) {
    ENTER(e);
    CallGuard call_guard(e, (hipStream_t)stream);
    if (n <= 0) return fail("no streams");
    hipStream_t s = (hipStream_t)stream;
    std::vector<Stream*> st(n);
    for (int i = 0; i < n; ++i) CHK(stream_of(e, stream_ids[i], &st[i]));
    // (the Conformer step, model_kind 0, has never had this check and gets none here: whether it should is a behaviour decision)
    if (e->cfg.model_kind != 0) CHK(distinct_streams(st));
    switch (e->cfg.model_kind) {
    case 1: return encode_chunk_squeezeformer(e, s, st, feats_dev, Tc, probs_dev, argmax_dev, maxprob_dev, enc_out_dev);
    case 2: return encode_chunk_efficient(e, s, st, feats_dev, Tc, probs_dev, argmax_dev, maxprob_dev, enc_out_dev);
    case 3: return encode_chunk_ds2(e, s, st, feats_dev, Tc, probs_dev, argmax_dev, maxprob_dev, enc_out_dev);
    default: return encode_chunk_conformer(e, s, st, feats_dev, Tc, probs_dev, argmax_dev, maxprob_dev, enc_out_dev);
    }
}

int masr_encode_chunk(masr_engine* e, const int32_t* stream_ids, int32_t n, const float* feats_dev, int32_t Tc,
                      float* probs_dev, int32_t* argmax_dev, float* maxprob_dev, void* stream) {
    if (!e || !e->finalized) return fail("engine not finalized");
    return encode_chunk_any(e, stream_ids, n, feats_dev, Tc, probs_dev, argmax_dev, maxprob_dev, nullptr, stream);
}

int masr_encode_chunk_enc(masr_engine* e, const int32_t* stream_ids, int32_t n, const float* feats_dev, int32_t Tc,
                          float* probs_dev, int32_t* argmax_dev, float* maxprob_dev, float* enc_out_dev, void* stream) {
    if (!e || !e->finalized) return fail("engine not finalized");
    if (e->cfg.model_kind == 3)
        return fail("masr_encode_chunk_enc: use_model deepspeech2 has no attention decoder to hand its encoder rows to; use "
                    "masr_encode_chunk");
    if (!enc_out_dev) return fail("masr_encode_chunk_enc: enc_out_dev is null (masr_encode_chunk is the step without it)");
    return encode_chunk_any(e, stream_ids, n, feats_dev, Tc, probs_dev, argmax_dev, maxprob_dev, enc_out_dev, stream);
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
                // (reduce_idx: null with a recover_idx set: the reference ignores recover_idx, no layer runs at half rate)
                if (e->reduce_idx >= 0 && l >= e->reduce_idx && l < e->recover_idx)
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
}  // extern "C"
