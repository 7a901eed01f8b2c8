// libmasr_hip.so -- what the encoder side of the engine shares across its translation units (file map: engine_state.h).  Private to
// csrc/ and included only by the engine*.hip files that run or dispatch an encoder; pool.hip, ctc_align.hip and
// engine_attdecoder.hip keep to engine_state.h.  A helper that only one file uses stays static there and is not declared here.
#pragma once
#include "engine_state.h"

#pragma GCC visibility push(hidden)
namespace masr {

struct EncodeCtx {
    int nseq;        // sequences (utterances or streams)
    int Tq;          // encoder frames per sequence in this call
    const int* lens; // device feature lengths for pad masking, or nullptr (streaming)
};

// what ffn() did with the stages asked for; as an int: the error code (0 = launched)
struct FfnDone {
    int err;
    bool tail_done = false;   // the kernel ran the tail stage; otherwise the caller launches it
    bool head_done = false;   // the kernel ran the head stage; otherwise ffn() has launched it in front of the block
    FfnDone(int err_ = 0) : err(err_) {}
    operator int() const { return err; }
};

// forward_chunk's cache bookkeeping (conformer/encoder.py:390-410, squeezeformer/encoder.py:288-297,338-347,
// efficient_conformer/encoder.py:316-336,365-381), as a window into append-only caches: a chunk of T0 input-rate frames attends
// over the last cache_t1 cached frames + itself; afterwards the cache is cut at next_cache_start.
struct ChunkWindow {
    int cache_t1, first_full;    // cached frames attended over; absolute index of the first of them (= positional index of key 0)
    int next_cache_t1, ncs;      // after the step
};

// a depthwise launch of elementwise.hip; a tap count it has no kernel for is an error, never a launch that did not happen
#define DWCHK(launched, ktaps)                                                                                        \
    do {                                                                                                              \
        if (!(launched)) return fail("no depthwise kernel for cnn_module_kernel " + std::to_string(ktaps) + ": " #launched); \
    } while (0)

// ---- engine.hip: the weight store ---------------------------------------------------------------------------------------------
int up(masr_engine* e, const std::string& name, std::vector<int64_t> shape, float** out);      // get() + upload()
int up_wb(masr_engine* e, const std::string& key, std::vector<int64_t> shape, float** w, float** b);
// The packed copy of `src` in `layout`, built on first use and kept: buffers of bytes_a (and bytes_b, 0 = none), filled by
// pack(copy, s), which issues the packing launch on the caller's stream.  nullptr = an allocation failed (masr_last_error says
// which): what was allocated is freed and nothing is cached.  (A template: its callers' packing lambdas are in other files.)
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
const float* packed_rows_of(masr_engine* e, const float* W, int N, hipStream_t s, PackLayout layout = PACK_ROWS_PC);
typedef void (*PackFfnFn)(const float*, const float*, float*, float*, int, hipStream_t);
int packed_ffn_of(masr_engine* e, const float* w1, const float* w2, hipStream_t s, const float** p1, const float** p2,
                  PackLayout layout = PACK_FFN_PC, PackFfnFn pack = launch_pack_ffn_pc);

// ---- engine_layers.hip: what the attention families share ---------------------------------------------------------------------
int enc_dim(const masr_engine* e);
int layer_kernel(const masr_engine* e, int i);
bool layer_grouped(const masr_engine* e, int i);
RowGemmArgs rg_args(const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int M, int N);
void rowgemm(masr_engine* e, hipStream_t s, int pro, int epi, RowGemmArgs a, int kind = PROF_GEMM);
void resid_gemm(masr_engine* e, hipStream_t s, const float* A, const float* W, const float* bias, const float* R, int M,
                const int* lens = nullptr, int mask_tp = 0, int mstride = 4, int a_seq_t = 0, int a_seq_stride = 0);
FfnArgs ffn_macaron(const LayerW& w, int M);
FfnArgs ffn_final(const LayerW& w, int M, float* y = nullptr);
FfnArgs ffn_of(int M, const float* lnw, const float* lnb, const float* w1, const float* b1, const float* w2, const float* b2);
FfnTail qkv_tail(const masr_engine* e, const LayerW& w, float* out, int ldo);
FfnHead conv_head(const masr_engine* e, const LayerW& w, const int* lens, int Tq, int ktaps, int mstride);
FfnDone ffn(masr_engine* e, hipStream_t s, FfnArgs a);
int embed(masr_engine* e, hipStream_t s, const float* feats, int nseq, int T, int* Tq_out, const int* skip_lens = nullptr);
int ensure_layer_ws(masr_engine* e, int nseq, int Tq);
int conv_module(masr_engine* e, hipStream_t s, const LayerW& w, const EncodeCtx& c, bool hist, int K = 0, int mstride = 4,
                bool pw1_done = false, bool pw2_later = false);
int conv_module_stream(masr_engine* e, hipStream_t s, const LayerW& w, int n, int Tq, float* const* cache_rd,
                       float* const* cache_wr, int K, bool pw2_later = false);
void qkv_proj(masr_engine* e, hipStream_t s, int pro, const float* lnw, const float* lnb, const float* wqkv, const float* bqkv, int M,
              const AttSeq* kv_seqs = nullptr, int kv_tq = 0);
void mhsa(masr_engine* e, hipStream_t s, const LayerW& w, int M, const AttSeq* kv_seqs = nullptr, int kv_tq = 0);
void mhsa_out(masr_engine* e, hipStream_t s, const LayerW& w, int M);
void mhsa_out_pw1(masr_engine* e, hipStream_t s, const LayerW& w, const EncodeCtx& c, int mstride = 4, int K = 0,
                  const float* att = nullptr, int a_seq_t = 0, int a_seq_stride = 0);
// finalize pieces (two calls for the front-end, so that a caller's own refusals keep their place between them)
int upload_conv_frontend(masr_engine* e, const std::string& c1, const std::string& c2, int ks, const char* c3, int d = 0);
int upload_embed_proj(masr_engine* e, const std::string& proj, int F2);
int upload_pos_table(masr_engine* e);
int get_conv_bn(masr_engine* e, const std::string& p, const HostTensor* bn[4]);
int upload_qkv(masr_engine* e, const std::string& p, float** wqkv, float** bqkv);
int upload_depthwise(masr_engine* e, const std::string& p, int K, float** dw_w, float** dw_b);
int build_ptab(masr_engine* e, hipStream_t s, const float* wpos, float** ptab);
int upload_gconst(masr_engine* e, hipStream_t s, const float* pw1_b, bool wide, float** gconst);
ChunkWindow chunk_window(const Stream& st, int T0);
int half_rate_window(const Stream& st, int want, int* first, int* count);
AttSeq interleaved_seq(const float* q, float* cache, int d, int first, int ncached, int Tl, float* out, int pos0, int q_abs0);
std::vector<float*> cnn_cache_table(const std::vector<Stream*>& st, int L, size_t layer_floats);
int upload_chunk_tables(masr_engine* e, hipStream_t s, const std::vector<AttSeq>& hs, const std::vector<float*>& hp,
                        void* third_dev = nullptr, const void* third = nullptr, size_t third_bytes = 0);
void advance_half_rate(std::vector<Stream*>& st, const std::vector<ChunkWindow>& win, int T0, int Tr);

// ---- engine_ctc.hip -----------------------------------------------------------------------------------------------------------
int chunk_ctc(masr_engine* e, hipStream_t s, const float* enc, int rows, float* probs, int32_t* argmax, float* maxprob,
              float* enc_out = nullptr);

// ---- the families: engine_conformer.hip, engine_efficient.hip, engine_squeezeformer.hip, engine_ds2.hip --------------------------
bool is_wide(const masr_engine* e);
int finalize_conformer(masr_engine* e, hipStream_t s);
int finalize_squeezeformer(masr_engine* e, hipStream_t s);
int finalize_ds2(masr_engine* e);
int ds2_forward(masr_engine* e, hipStream_t s, const float* feats, const int* lens, int nseq, int T, float* enc_out, Stream** st,
                int* Tq_out);
typedef int EncodeFullFn(masr_engine* e, hipStream_t s, const float* feats, const int* lens, int B, int T, float* enc_out, int chunk);
EncodeFullFn encode_full_conformer, encode_full_wide, encode_full_efficient, encode_full_squeezeformer;
// enc_out_dev (masr_encode_chunk_enc; nullptr: masr_encode_chunk): the step's encoder rows, handed on to chunk_ctc
typedef int EncodeChunkFn(masr_engine* e, hipStream_t s, std::vector<Stream*>& st, const float* feats, int Tc, float* probs_dev,
                          int32_t* argmax_dev, float* maxprob_dev, float* enc_out_dev);
EncodeChunkFn encode_chunk_conformer, encode_chunk_efficient, encode_chunk_squeezeformer, encode_chunk_ds2;

}  // namespace masr
#pragma GCC visibility pop
