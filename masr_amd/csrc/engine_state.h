// libmasr_hip.so -- what the engine's translation units share: the error plumbing, the engine's state structs and the
// declarations of the host helpers that cross a file boundary.  Private to csrc/ (the public C ABI is include/masr_hip.h).
//   engine.hip               error state, weight store, create / load / finalize and the encode calls as dispatchers, streams, lanes
//   engine_layers.hip        what the attention families share: GEMM and row-block calls, FFN block, front-end, conv module,
//                            attention projections, finalize pieces, chunk-step tables
//   engine_conformer.hip     Conformer: finalize (also the Efficient Conformer's), fused and width-generic forward, chunk step
//   engine_efficient.hip     Efficient Conformer: forward, chunk step
//   engine_squeezeformer.hip Squeezeformer: finalize, forward, chunk step
//   engine_ds2.hip           DeepSpeech2: finalize, forward, chunk step
//   engine_ctc.hip           CTC head, collapse, top-k, prefix beam search on the device
//   engine_frontend.hip      fbank / MFCC / linear features, resampling, masr_transcribe_*
//   engine_ops.hip           single ops of the tests, debug switches, profile calls
//   engine_attdecoder.hip    attention decoder: finalize, rescoring, autoregressive search (kernels: decoder.hip, decoder_step.hip)
//   ctc_align.hip            forced alignment: kernel and masr_ctc_align
// A helper that only one file uses stays static (or in an anonymous namespace) there and is not declared here; what only the
// encoder files share (engine_layers.hip's helpers, the families' entry points) is declared in engine_encoder.h.
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/masr_hip.h"
#include "common.h"
#include "ffn_plan.h"

namespace masr {
// the two that other parts of the library (pool.hip) call: exported, as they were
int engine_fail(const std::string& m);      // engine.hip: sets what masr_last_error() returns on this thread; returns 1
// frames behind the subsampling front-end (before the Efficient-Conformer's stride layer): the unit of a stream's cap and offset
int subsampled_frames(const masr_engine* e, int feature_frames);      // engine.hip
}  // namespace masr

// everything below is internal to the engine's translation units: kept out of the library's dynamic symbol table (in one
// translation unit these helpers were static or in an anonymous namespace)
#pragma GCC visibility push(hidden)
namespace masr {
inline int fail(const std::string& m) { return engine_fail(m); }
// errors noted by the kernel launchers (note_launch_error) since the last check on this thread: whether there is one (the
// check every LAUNCHCHK makes: no string is built on the way), and the first of them, cleared by the call
bool launch_error_pending();                // engine.hip
std::string take_launch_error();            // engine.hip
}  // namespace masr

#define HIPCHK(expr)                                                                                    \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return masr::fail(std::string(#expr) + ": " + hipGetErrorString(_e) + " (" + __FILE__ + ":" +     \
                        std::to_string(__LINE__) + ")");                                                \
    } while (0)
#define CHK(expr)              \
    do {                       \
        int _r = (expr);       \
        if (_r) return _r;     \
    } while (0)
// after a group of launches: a launcher-side error first, then the runtime's sticky launch error
#define LAUNCHCHK()                                     \
    do {                                                \
        if (masr::launch_error_pending()) {             \
            std::string _m = masr::take_launch_error(); \
            (void)hipGetLastError();                    \
            return masr::fail(_m);                            \
        }                                               \
        HIPCHK(hipGetLastError());                      \
    } while (0)
// every entry point that touches the device first makes the engine's GPU current on the calling thread (an engine on
// device != 0 may be driven from a worker thread whose current device is still 0)
#define ENTER(e) HIPCHK(hipSetDevice((e)->cfg.device_id))
// a wide.hip launch under its profile class (masr_profile_select kinds 9-12); a width the kernels are not built for is an error
#define WIDECHK(kind, launched)                                                                                      \
    do {                                                                                                             \
        ProfScope _ps(e, s, kind, 0.0);                                                                              \
        if (!(launched)) return masr::fail("no kernel for output_size " + std::to_string(e->cfg.d_model) + ": " #launched); \
    } while (0)

namespace masr {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t n) {
        if (n <= bytes) return 0;
        if (p) HIPCHK(hipFree(p));
        p = nullptr;
        bytes = 0;
        size_t want = n + n / 8 + 256;
        HIPCHK(hipMalloc(&p, want));
        // zero once: kernels that skip the padded row blocks of a batch (masr_debug_set key 38) leave those rows as they are, and
        // what is there must at least be finite -- a later 0 * stale product must not see the NaN patterns of fresh memory
        HIPCHK(hipMemset(p, 0, want));
        // (the fill runs on the NULL stream, which a non-blocking stream does not wait for: without this a lane's first launches
        // could write the buffer BEFORE it is cleared -- the first two-lane call lost its second pass that way)
        HIPCHK(hipStreamSynchronize(nullptr));
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

// one packed weight copy (masr_engine::packed): `a` alone, or the W1 | W2 pair of an FFN
struct PackedW {
    DevBuf a, b;
    void release() {
        a.release();
        b.release();
    }
};

// Pinned host staging for the per-call descriptor tables (AttSeq rows, cache pointers) of the streaming chunk step: the
// copies to the device are truly asynchronous, so the chunk step does not stall the host on the work queued before it.
// One call owns the area at a time: `begin` waits for the previous call's copies (normally long done).
struct PinnedStage {
    char* p = nullptr;
    size_t bytes = 0, used = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
    int begin(size_t need) {
        if (pending) {
            HIPCHK(hipEventSynchronize(ev));
            pending = false;
        }
        if (!ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (need > bytes) {
            if (p) HIPCHK(hipHostFree(p));
            p = nullptr;
            bytes = 0;
            const size_t want = need + need / 4 + 4096;
            HIPCHK(hipHostMalloc((void**)&p, want, hipHostMallocDefault));
            bytes = want;
        }
        used = 0;
        return 0;
    }
    // copy `n` bytes of `src` through the staging area to `dst` (device) on stream `s`
    int push(void* dst, const void* src, size_t n, hipStream_t s) {
        if (n == 0) return 0;
        const size_t at = (used + 15) & ~(size_t)15;
        if (at + n > bytes) return fail("descriptor staging area overflow");
        memcpy(p + at, src, n);
        used = at + n;
        HIPCHK(hipMemcpyAsync(dst, p + at, n, hipMemcpyHostToDevice, s));
        return 0;
    }
    int end(hipStream_t s) {
        HIPCHK(hipEventRecord(ev, s));
        pending = true;
        return 0;
    }
    void release() {
        if (pending) (void)hipEventSynchronize(ev);
        if (p) (void)hipHostFree(p);
        if (ev) (void)hipEventDestroy(ev);
        p = nullptr;
        ev = nullptr;
        bytes = 0;
        pending = false;
    }
};

struct LayerW {
    float *ln_ffm_w, *ln_ffm_b, *ffm_w1, *ffm_b1, *ffm_w2, *ffm_b2;
    float *ln_mha_w, *ln_mha_b, *wqkv, *bqkv, *wo, *bo, *pos_u, *pos_v, *wpos, *ptab;
    float *ln_conv_w, *ln_conv_b, *pw1_w, *pw1_b, *dw_w, *dw_b, *cln_w, *cln_b, *pw2_w, *pw2_b, *gconst;
    float *chain_w, *chain_b;     // [Wo; W_pw1] [768,256] and [bo; b_pw1] for the fused out-proj -> LN -> pw1 -> GLU kernel
    float *ln_ff_w, *ln_ff_b, *ff_w1, *ff_b1, *ff_w2, *ff_b2;
    float *ln_fin_w, *ln_fin_b;
};

struct SqLayerW {   // Squeezeformer block (post-LN, adaptive scale/bias, BatchNorm conv module)
    float *att_s, *att_b, *wqkv, *bqkv, *wo, *bo, *pos_u, *pos_v, *wpos, *ptab, *ln1_w, *ln1_b;
    float *f1_s, *f1_b, *f1_w1, *f1_b1, *f1_w2, *f1_b2, *ln2_w, *ln2_b;
    float *cv_s, *cv_b, *pw1_w, *pw1_b, *dw_w, *dw_b, *bn_scale, *bn_shift, *pw2_w, *pw2_b, *ln3_w, *ln3_b, *gconst;
    float *f2_s, *f2_b, *f2_w1, *f2_b1, *f2_w2, *f2_b2, *ln4_w, *ln4_b;
};

struct Ds2LayerW {  // DeepSpeech2 RNN layer: input projection of both directions stacked, recurrent weights, LayerNorm
    float *wih, *bih, *whh, *ln_w, *ln_b;
    float* bhn = nullptr;   // use_gru: b_hn [ndir][H] (inside the reset-gate product, not folded into bih)
    int kin;
};

struct HostTensor {
    std::vector<float> v;
    std::vector<int64_t> shape;
};

struct Stream {
    bool open = false;
    int offset = 0;
    int offset_r = 0;   // frames emitted at the reduced rate (Squeezeformer blocks between time reduction and recovery)
    int cap = 0;
    int history = -1;   // required_cache_size of forward_chunk: < 0 keep every key, >= 0 attend over at most that many cached keys
    int cache_t1 = 0;   // cached keys the next chunk attends over, in input-rate frames (= att_cache.size(2) of the reference)
    int first_half = 0; // half-rate layers (Squeezeformer between reduction and recovery, Efficient-Conformer behind the stride
                        // layer): index of their first kept cache entry (advances by next_cache_start // 2 per step)
    DevBuf att;  // [L][cap][2*d]  (k | v per row)
    DevBuf cnn;  // [L][kernel-1][d]   (DeepSpeech2: LSTM state [L][2 (h, c)][rnn_size]; GRU: h in both)
    DevBuf cnn2; // Conformer / Squeezeformer: second half of the double-buffered cnn cache (a chunk step reads `cnn`, writes
                 // `cnn2`, then the two are swapped -- lets one kernel read the history and write the new cache without ordering)
};

struct GBeam {        // device-resident streaming CTC prefix beam search (masr_gbeam_*)
    bool open = false, started = false;
    int beam = 0, blank = 0, cap = 0;
    DevBuf pool, state;
    masr_lm* lm = nullptr;       // external scorer bound with masr_gbeam_set_lm (not owned)
    float alpha = 0.f, beta = 0.f;
};
struct BeamLast {     // what the last whole-utterance search left in one workspace (masr_beam_nbest_gpu reads it back)
    bool valid = false;
    const void* lm = nullptr;    // the scorer that search had bound (not owned)
    float alpha = 0.f, beta = 0.f;   // ... with these weights: the reported scores take the scorer's share out with them
    int B = 0, beam = 0, pool_cap = 0;
};

enum ProfKind { PROF_NONE = 0, PROF_GEMM = 1, PROF_FFN1 = 2, PROF_CONV2 = 3, PROF_ATT = 4, PROF_FBANK = 5,
                PROF_FFN_TAIL = 6, PROF_FFN_HEAD = 7, PROF_RNN = 8,
                PROF_WIDE_LN = 9, PROF_WIDE_GLU = 10, PROF_WIDE_DWCONV = 11, PROF_WIDE_CACHE = 12 };   // 9-12: the row kernels of wide.hip (12 = conv_hist + kv_append)     // 2 = the plain fused FFN kernel; 6 = its variant with the QKV tail stage, 7 = with the conv-module head stage (own kernel names)

// Everything a forward call WRITES on the device (and the pinned descriptor staging of the chunk step): one set per LANE.
// masr_select_lane parks the active set and brings another one in, so two offline passes can be in flight on two streams of one
// engine (one set of weights) -- launches that share a lane must be ordered by their stream, as before.
struct EngineWs {
    DevBuf gx, rnn_out, hstate, cstate, ds2_lens;                               // DeepSpeech2 workspaces
    PinnedStage stage;
    DevBuf qplanes, attp, cnnptrs, ffpart;                                      // planar q|k|v and attention output, [B][Tpad][256]
    DevBuf fb_scratch;
    DevBuf x1, x2, x, ln, hid, qkv, att, lnpad, glu, dwo, logits, feats, enc, idx, maxp, attseq, gain, nframes, lens, xsave,
        xred, xh;      // xh: rows updated by the head stage of a d_ff-split FFN launch (few rows)
    DevBuf x3, sublens;   // conv2d8: the third subsampling conv's output; conv2d6 / conv2d8: the lengths in conv2d units (sub_lens)
    DevBuf posoff;        // abs_pos chunk steps: the streams' offsets (first positional row of each stream's new frames)
    // attention decoder (masr_rescore; allocated on the lane's first rescoring call, never by an engine without the decoder):
    // residual rows, LayerNorm rows, q | k | v (self) / q (source), attention output, source k | v of the encoder frames, FFN hidden
    // rows, logits, per-row log-probabilities
    DevBuf dec_x, dec_ln, dec_qkv, dec_att, dec_kv, dec_hid, dec_logits, dec_rowlp;
    // autoregressive search (masr_attention_decode / masr_op_decoder_step; allocated on the lane's first such call): the step's rows
    // (residual, LayerNorm, q, attention output, FFN hidden, logits), the self-attention k | v cache [blocks][Lrun][S][2 d], the
    // source k | v [blocks][B * Tp][2 d], top-N values | ids, the double-buffered token / ancestor / score tables and flags, and
    // the test op's [S, V] log-probabilities
    DevBuf st_x, st_ln, st_q, st_att, st_hid, st_logits, st_cache, st_src, st_top, st_tab, st_full;
    // joint CTC / attention search (masr_joint_decode / masr_op_ctc_prefix_scores; allocated on the lane's first such call): the
    // CTC prefix states r_n | r_b of every hypothesis, double-buffered [2][S][2][Tp], and the double-buffered A / psi / n tables
    // with the candidates' psi [S, M] (the scorer op keeps its host tables' device copies there)
    DevBuf jt_r, jt_tab;
    // forced alignment (masr_ctc_align; allocated on the lane's first such call): the predecessor choice of every state and frame,
    // [B][T'][2 Lmax + 1] bytes
    DevBuf align_bp;
    size_t decoder_bytes() const {
        return dec_x.bytes + dec_ln.bytes + dec_qkv.bytes + dec_att.bytes + dec_kv.bytes + dec_hid.bytes + dec_logits.bytes +
               dec_rowlp.bytes + st_x.bytes + st_ln.bytes + st_q.bytes + st_att.bytes + st_hid.bytes + st_logits.bytes + st_cache.bytes +
               st_src.bytes + st_top.bytes + st_tab.bytes + st_full.bytes + jt_r.bytes + jt_tab.bytes;
    }
    void release_all() {
        for (DevBuf* b : {&gx, &rnn_out, &hstate, &cstate, &ds2_lens, &qplanes, &attp, &cnnptrs, &ffpart, &fb_scratch, &x1, &x2, &x,
                          &ln, &hid, &qkv, &att, &lnpad, &glu, &dwo, &logits, &feats, &enc, &idx, &maxp, &attseq, &gain, &nframes,
                          &lens, &xsave, &xred, &xh, &x3, &sublens, &posoff, &dec_x, &dec_ln, &dec_qkv, &dec_att, &dec_kv, &dec_hid,
                          &dec_logits, &dec_rowlp, &st_x, &st_ln, &st_q, &st_att, &st_hid, &st_logits, &st_cache, &st_src, &st_top,
                          &st_tab, &st_full, &jt_r, &jt_tab, &align_bp})
            b->release();
        stage.release();
    }
};

// one block of the attention decoder (DecoderLayer, transformer/decoder.py:273-394): pre-norm self-attention (q | k | v fused),
// source attention (q; k | v of the encoder frames fused), ReLU feed-forward
struct DecLayerW {
    float *n1w, *n1b, *wqkv, *bqkv, *wo, *bo;
    float *n2w, *n2b, *wq2, *bq2, *wkv2, *bkv2, *wo2, *bo2;
    float *n3w, *n3b, *w1, *b1, *w2, *b2;
};
struct DecoderW {       // one TransformerDecoder: embedding, blocks, after_norm, output_layer
    float *emb = nullptr, *after_w = nullptr, *after_b = nullptr, *out_w = nullptr, *out_b = nullptr;
    std::vector<DecLayerW> layers;
};
struct DecoderState {   // masr_decoder_enable: the YAML decoder_conf; weights uploaded by masr_finalize
    bool enabled = false, ready = false;
    int heads = 0, dff = 0, nl = 0, nr = 0;
    DecoderW left, right;
    size_t weight_bytes = 0;
    std::vector<void*> owned;   // the decoder's device weights (a reload replaces the whole set; masr_destroy frees it)
};

}  // namespace masr
#pragma GCC visibility pop

// the global type the public header names; its members are masr:: types
struct masr_engine : masr::EngineWs {
    masr_config cfg;
    masr::DecoderState dec;
    masr::EngineWs parked[MASR_LANES];     // the workspace sets of the lanes that are not active (parked[lane] is unused)
    int lane = 0;
    hipEvent_t pack_ev = nullptr;    // recorded behind the last call that built a packed weight copy on first use ...
    void* pack_stream = nullptr;     // ... on this stream: calls on OTHER streams wait for it before they read the copies
    bool pack_pending = false;
    bool finalized = false;
    std::map<std::string, masr::HostTensor> host;
    std::vector<void*> owned;   // device weight allocations
    // weights
    float *cmvn_mean = nullptr, *cmvn_istd = nullptr, *conv1_w = nullptr, *conv1_b = nullptr, *conv2_w = nullptr,
          *conv2_b = nullptr, *conv3_w = nullptr, *conv3_b = nullptr, *embed_w = nullptr, *embed_b = nullptr, *after_w = nullptr, *after_b = nullptr,
          *ctc_w = nullptr, *ctc_b = nullptr, *pe = nullptr;
    std::vector<masr::LayerW> layers;
    std::vector<masr::SqLayerW> sq_layers;
    std::vector<masr::Ds2LayerW> ds2_layers;
    std::vector<masr::GBeam> gbeams;
    masr::DevBuf beam_pool, beam_state;
    // whole-utterance prefix searches launched on OTHER streams than the first one get workspaces of their own: two searches may
    // run next to each other (predict_batch: the passes' searches on two side streams), launches on one stream are ordered anyway
    std::map<void*, std::pair<masr::DevBuf, masr::DevBuf>> beam_ws;
    std::map<void*, masr::BeamLast> beam_last;       // by stream, the first stream's workspace included
    // masr_mean_square runs on whatever stream prepares the NEXT pass (the facade's side stream, the contract step's copy stream)
    // while the feature launch of the current pass reads e->gain on the compute stream: its chunk sums and its unused gain slots
    // live in a scratch of their own, one per calling stream (launches on one stream are ordered anyway)
    std::map<void*, masr::DevBuf> ms_ws;
    int skip_padding = 7;            // masr_debug_set key 38: the offline Squeezeformer launches skip the all-padding row blocks of a batch
    void* beam_first_stream = nullptr;
    bool beam_first_set = false;
    // every fragment-ordered weight copy, built on first use by packed_of(): (common.h PackLayout, source device pointer) -> copy
    std::map<std::pair<int, const float*>, masr::PackedW> packed;
    long long* beam_prof = nullptr;                                             // debug: phase cycle counters (masr_debug_set key 2)                                               // GPU beam search scratch                               // DeepSpeech2 workspaces
    float *preln_w = nullptr, *preln_b = nullptr, *tr_dw_w = nullptr, *tr_dw_b = nullptr, *tr_pw_w = nullptr,
          *tr_pw_b = nullptr, *rec_w = nullptr, *rec_b = nullptr;
    int reduce_idx = -1, recover_idx = -1;
    int stride_idx = -1, n_group_layers = 0, group_size = 3;   // Efficient-Conformer (model_kind 2)
    int input_layer = masr::IL_CONV2D;     // Conformer / Efficient-Conformer subsampling front-end (cfg.reserved[3], common.h InputLayer)
    bool conv_bn = false;            // cnn_module_norm: batch_norm (Conformer: cfg.reserved[0] = 1, Efficient Conformer: cfg.reserved[4] = 1): LayerW::cln_w / cln_b hold the folded scale / shift
    bool ds2_gru = false;            // DeepSpeech2 with use_gru: True (cfg.reserved[0] = 1): nn.GRU recurrent layers (gru.hip)
    int pos_enc = masr::POS_ENC_REL;       // Conformer pos_enc_layer_type (cfg.reserved[2], common.h PosEnc): rel_pos, abs_pos or no_pos
    int act = masr::ENC_ACT_SWISH;         // Conformer activation_type (cfg.reserved[4], common.h EncAct); anything but swish runs the width-generic layer
    // fbank tables
    float *window = nullptr, *melwt = nullptr, *tw512 = nullptr, *twr4 = nullptr;
    masr::FbankTables fbank_tables() const { return masr::FbankTables{window, melwt, tw512, twr4, mel_lo}; }
    int* mel_lo = nullptr;
    // mfcc / linear tables (built on first use)
    float *dct = nullptr, *lifter = nullptr;
    int dct_ceps = 0;
    double *lin_win = nullptr, *lin_tw = nullptr;
    double lin_scale = 0.0;
    // streams
    std::vector<masr::Stream> streams;
    // profiling
    int prof_kind = 0;
    int prof_stride = 1, prof_seen = 0;                     // every prof_stride-th matching launch is timed (masr_debug_set key 16)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    size_t prof_used = 0;
    double prof_flops = 0.0;
};

#pragma GCC visibility push(hidden)
namespace masr {

template <class T>
int upload(masr_engine* e, const std::vector<T>& v, T** out) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, std::max<size_t>(v.size(), 1) * sizeof(T)));
    HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    e->owned.push_back(p);
    *out = reinterpret_cast<T*>(p);
    return 0;
}

// ---- profiling helpers ------------------------------------------------------------------------------
struct ProfScope {
    masr_engine* e;
    hipStream_t s;
    bool on;
    ProfScope(masr_engine* e_, hipStream_t s_, int kind, double flops) : e(e_), s(s_) {
        on = e->prof_kind != 0 && (e->prof_kind == kind || (e->prof_kind == PROF_GEMM && (kind == PROF_FFN1 || kind == PROF_CONV2 || kind == PROF_FFN_TAIL || kind == PROF_FFN_HEAD)));
        if (on && e->prof_stride > 1) on = (e->prof_seen++ % e->prof_stride) == 0;     // a sample of the launches: two event
        if (!on) return;                                                                // records cost ~6 us of stream time
        if (e->prof_used == e->prof_events.size()) {
            hipEvent_t a, b;
            hipEventCreate(&a);
            hipEventCreate(&b);
            e->prof_events.push_back({a, b});
        }
        hipEventRecord(e->prof_events[e->prof_used].first, s);
        e->prof_flops += flops;
    }
    ~ProfScope() {
        if (!on) return;
        hipEventRecord(e->prof_events[e->prof_used].second, s);
        e->prof_used++;
    }
};

// Packed weight copies are built on first use by whatever call needs them first, on that call's stream.  With two lanes a call
// on ANOTHER stream may find the copy in the cache while the packing launch is still queued: the call that packed (the cache has
// grown under it) records an event behind itself, and calls on other streams wait for that event until it has completed.
struct CallGuard {
    masr_engine* e;
    hipStream_t s;
    size_t n0;
    CallGuard(masr_engine* e_, hipStream_t s_) : e(e_), s(s_), n0(e_->packed.size()) {
        if (!e->pack_pending) return;
        if (hipEventQuery(e->pack_ev) == hipSuccess) {
            e->pack_pending = false;
        } else {
            (void)hipGetLastError();          // (hipErrorNotReady is not an error of ours)
            if ((void*)s != e->pack_stream) (void)hipStreamWaitEvent(s, e->pack_ev, 0);
        }
    }
    ~CallGuard() {
        if (e->packed.size() == n0) return;
        if (!e->pack_ev && hipEventCreateWithFlags(&e->pack_ev, hipEventDisableTiming) != hipSuccess) return;
        // (a pending event of another stream: this call waited for it at its start, so the new record covers it)
        if (hipEventRecord(e->pack_ev, s) == hipSuccess) {
            e->pack_stream = (void*)s;
            e->pack_pending = true;
        }
    }
};

// ---- engine.hip ---------------------------------------------------------------------------------------------------------------
int get(masr_engine* e, const std::string& name, std::vector<int64_t> shape, const HostTensor** out);
// ---- engine_frontend.hip (masr_create builds the tables: a weight-less engine can already run the feature front-end) -----------
int build_fbank_tables(masr_engine* e);
// ---- engine_layers.hip --------------------------------------------------------------------------------------------------------
void gemm(masr_engine* e, hipStream_t s, const float* A, int lda, const float* W, const float* bias, float* C, int ldc,
          int M, int N, int K, int act, float alpha, const float* R, int ldr, int kind = PROF_GEMM,
          const int* lens = nullptr, int mask_tp = 0);
// C[M, N] = A . W^T + bias with row m of A = row rows[m] of pool [n_rows, lda] (A_ROWS of gemm_f32.hip; never the split-bf16 variant,
// so bit-equal to gemm() on the gathered copy only while masr_debug_set key 20 is off)
void gemm_rows(masr_engine* e, hipStream_t s, const float* pool, int lda, const int64_t* rows, int64_t n_rows, const float* W,
               const float* bias, float* C, int ldc, int M, int N, int K);

// ---- engine_attdecoder.hip ----------------------------------------------------------------------------------------------------
int finalize_decoder(masr_engine* e);       // masr_finalize: the decoder's weights, before the model's finalize drops the host copies

}  // namespace masr
#pragma GCC visibility pop
