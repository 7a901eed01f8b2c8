/*
 * libmasr_hip.so -- C ABI of the MI355X (gfx950) MASR inference hot path.
 *
 * The reference (yeyupiaoling/MASR) has no FFI of its own: its boundary is three Python call
 * sites.  This header is the C-ABI a binding for that path would use; the
 * Python mirror of the reference classes lives in masr_amd/ and calls these functions via ctypes.
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on error; masr_last_error() gives the message
 *  - all *_dev pointers are DEVICE pointers owned by the caller (e.g. torch tensors); the library
 *    never frees them, launches on the caller's hipStream_t (passed as void*) and never
 *    synchronises unless stated
 *  - host pointers are plain arrays read during the call
 *  - an engine is bound to one GPU and is not thread-safe (one engine per rank)
 *  - all arithmetic is fp32 ("f32" MFMA v_mfma_f32_32x32x2_f32), like the reference's CPU path
 */
#ifndef MASR_HIP_H
#define MASR_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct masr_engine masr_engine;

/* Model hyper-parameters = the YAML `encoder_conf` block (reference configs/conformer.yml:1-16)
 * + vocabulary size (masr/trainer.py:174-203 builds the model from exactly these). */
typedef struct masr_config {
    int32_t model_kind;      /* 0 = conformer                                                   */
    int32_t d_model;         /* encoder_conf.output_size        (256); deepspeech2: encoder_conf.rnn_size, a multiple of
                              * 256 in [256, 2048] (1024 in configs/deepspeech2.yml)           */
    int32_t heads;           /* encoder_conf.attention_heads    (4)                             */
                             /* (d_model, heads): (256, 4) for model kinds 0-2; model kind 0 also (512, 8), with layer_norm
                              * (reserved[0] = 0) and input_layer conv2d (reserved[3] = 0) only.  masr_create refuses every other
                              * pair with a message that names output_size / attention_heads.  (512, 8) runs a width-generic path
                              * of separate launches (csrc/wide.hip + the tiled GEMM): every entry point works as at 256 -- both
                              * lanes, chunk steps, cache export [L, 8, t, 128] / [L, 1, 512, 14] -- but it builds no packed weight
                              * copies and none of the fused row-block kernels run, so the masr_debug_set keys that choose between
                              * them have no effect there; the attention keys (attention_fewq, attention_fold, ...) keep theirs */
    int32_t d_ff;            /* encoder_conf.linear_units       (2048); squeezeformer: encoder_dim x
                              * feed_forward_expansion_factor.  Model kinds 0-2: any positive multiple of 128;
                              * masr_create refuses 0, negative values and non-multiples              */
    int32_t num_blocks;      /* encoder_conf.num_blocks         (12)                            */
    int32_t cnn_kernel;      /* encoder_conf.cnn_module_kernel  (15; squeezeformer 31).  Model kinds 0 and 1: any value in
                              * [3, 31] with causal = 1, the odd ones with causal = 0 (symmetric padding of (K - 1) / 2
                              * frames); model kind 2: 15.  masr_create refuses everything else by name.  The stream
                              * caches and masr_stream_export_cache's cnn rows hold cnn_kernel - 1 frames          */
    int32_t n_mels;          /* preprocess_conf.n_mels          (80)                            */
    int32_t vocab_size;      /* len(vocabulary.txt)                                             */
    int32_t causal;          /* `streaming: True` => causal conv + dynamic-chunk masks (model.py:37-42) */
    int32_t max_pos;         /* positional table length (reference max_len = 5000, embedding.py:14)  */
    int32_t device_id;
    int32_t reserved[5];     /* squeezeformer: [0] reduce_idx, [1] recover_idx; efficient_conformer: [0] stride layer, [1] grouped layers,
                                [2] group size, [4] = 1 -> cnn_module_norm: batch_norm (full-context and chunked; [0] is taken by the
                                stride layer); conformer: [0] = 1 -> cnn_module_norm: batch_norm (convolution.py:60-67; full-context only);
                                conformer and efficient_conformer: [3] input_layer, 0 = conv2d (x4), 1 = conv2d6 (x6), 2 = conv2d8 (x8)
                                (conformer/subsampling.py:65-211); deepspeech2 (model_kind 3): [0] recurrent cell, 0 = LSTM,
                                1 = GRU (encoder_conf.use_gru, deepspeech2/encoder.py:21-33), any other value is refused;
                                conformer: [2] pos_enc_layer_type (conformer/encoder.py:239-281), 0 = rel_pos (RelPositionalEncoding +
                                RelPositionMultiHeadedAttention), 1 = abs_pos (PositionalEncoding: x * sqrt(d) + pe[offset : offset + T],
                                plain MultiHeadedAttention), 2 = no_pos (NoPositionalEncoding: x unscaled, plain attention), at
                                (256, 4) and (512, 8), every entry point; 1 and 2 load checkpoints WITHOUT self_attn.linear_pos /
                                pos_bias_u / pos_bias_v (masr_finalize refuses one that holds them, and a rel_pos engine one that
                                lacks them, naming pos_enc_layer_type and the key) and build no positional key tables.  masr_create
                                refuses any other value by name, and a non-zero [2] for the squeezeformer (rel_pos only there; the
                                efficient_conformer's [2] is its group size: that family has no such slot and runs rel_pos only);
                                conformer: [4] activation_type (utils/common.py get_activation, torch's defaults), 0 = swish, 1 = relu,
                                2 = gelu (erf-exact), 3 = tanh, 4 = hardtanh (clamp to [-1, 1]), 5 = selu: the hidden activation of
                                both feed-forward modules and the one behind the conv module's norm (the GLU keeps its sigmoid), at
                                (256, 4) and (512, 8), every entry point.  A non-zero [4] runs the width-generic path of separate
                                launches at (256, 4) too: no packed weight copies for the layers, none of the fused row-block
                                kernels, and the masr_debug_set keys that choose between them have no effect there (as at 512; the
                                attention keys keep theirs); 0 keeps the launches and bits it had.  masr_create refuses any other
                                value by name (activation_type), and a non-zero [4] together with [0] = 1 (batch_norm runs with
                                swish only).  No other model kind reads [4] as an activation (the efficient_conformer's [4] is its
                                norm selector): those families run swish only.  An activation has no weights: nothing in a checkpoint
                                can confirm the value.
                                Layer layouts, L = num_blocks (masr_create refuses everything else before any allocation, naming
                                the YAML key):
                                  squeezeformer: [0] reduce_idx = -1 (null: no time reduction; [1] is then ignored, as the reference
                                  ignores it) or a layer in [0, L); with [0] >= 0, [1] recover_idx is a layer in [reduce_idx, L)
                                  ([1] = [0]: reduction and recovery in front of the same layer).  recover_idx < reduce_idx is
                                  refused (the reference fails there on an empty stack).  reduce_idx set with recover_idx null
                                  (-1) or >= L is a legal reference configuration whose output stays at HALF the frame rate: this
                                  engine REFUSES it, naming recover_idx -- every entry point, masr_encoder_frames and
                                  masr_frame_reduction included, keeps the Squeezeformer's output at the input frame rate;
                                  efficient_conformer: [0] stride_layer_idx in [0, L) (one stride-2 layer: the output is always at
                                  half the rate of the input layer); [1] = number of leading grouped layers (len(group_layer_idx))
                                  in [0, [0] + 1]: grouped attention behind the stride layer is not implemented */
} masr_config;

const char* masr_last_error(void);
int masr_version(void);

/* Lifecycle.  Replaces InferencePredictor.__init__'s torch.jit.load + .to(device)
 * (masr/infer_utils/inference_predictor.py:31-41). */
int masr_create(const masr_config* cfg, masr_engine** out);
void masr_destroy(masr_engine* e);

/* Weight upload keyed by the reference state_dict names (produced by
 * masr/trainer.py:308,684-689).  `host` is fp32, `shape` has `ndim` entries.  Names outside
 * `encoder.*` / `ctc.*` are ignored (attention decoder, unused by get_encoder_out*) -- unless masr_decoder_enable came
 * first: then `decoder.left_decoder.*` / `decoder.right_decoder.*` are kept for masr_rescore.
 * The optional name "__pos_table__" [max_pos, d_model] overrides the built-in sin/cos table
 * (conformer/embedding.py:31-37) so that it is bit-identical to torch's. */
int masr_load_tensor(masr_engine* e, const char* name, const float* host, const int64_t* shape, int32_t ndim);
/* Builds the derived device tensors (fused QKV, GLU-permuted pointwise_conv1, channels-last conv
 * weights, per-layer positional keys W_pos*PE) -- call once after all tensors are loaded. */
int masr_finalize(masr_engine* e, void* stream);

/* Feature front-end.  Replaces AudioFeaturizer.featurize
 * (masr/data_utils/featurizer/audio_featurizer.py:37-69,120-138) for a padded batch of 16 kHz
 * audio: per-utterance RMS-dB normalisation + int16 truncation + Kaldi fbank.  Works on an engine
 * without weights (tables are built by masr_create).
 *   samples_dev  [B, n_max] int16 PCM (sample_format 0; AudioSegment scales by 1/32768,
 *                audio.py:532-546) or float32 samples in [-1,1] scale (sample_format 1)
 *   n_samples_dev [B] int32
 *   feats_dev    [B, T_max, n_mels] f32, T_max = 1 + (n_max - 400) / 160; frames >= T_b are zero
 *   n_frames_dev [B] int32 (out, may be NULL)
 *   norm_pcm_dev [B, n_max] int16 (out, may be NULL): the normalised int16 samples (audio.py:549-574)
 *   gain_dev     [B] f32 (out, may be NULL): linear gain 10^(gain_dB/20) applied by normalize()
 *                (audio.py:256-264) -- lets the host mirror the reference's in-place mutation
 *   use_db_normalization  0 = off; 1 = gains computed on the device (every scalar step of rms_db / normalize / gain_db evaluated
 *                in double and rounded once to float32); 2 = gains SUPPLIED in gain_dev (in): the caller evaluated
 *                audio.py:287-304,519-529 with its own numpy on the mean square returned by masr_mean_square -- numpy's float32
 *                log10 / power are not correctly rounded and differ between hosts, so this is the mode that reproduces the
 *                reference's int16 samples bit for bit on the host it runs on.  Same meaning in masr_mfcc_batch / masr_linear_batch. */
int masr_fbank_batch(masr_engine* e, const void* samples_dev, int32_t sample_format, const int32_t* n_samples_dev,
                     int32_t B, int32_t n_max, int32_t use_db_normalization, float target_db, float* feats_dev,
                     int32_t* n_frames_dev, int16_t* norm_pcm_dev, float* gain_dev, void* stream);

/* mean_square_dev[b] = float32 np.mean(samples ** 2) of utterance b in numpy's own summation order (8192-element buffered
 * pairwise sums) -- the quantity AudioSegment.rms_db starts from (masr/data_utils/audio.py:519-529), bit-identical to numpy. */
int masr_mean_square(masr_engine* e, const void* samples_dev, int32_t sample_format, const int32_t* n_samples_dev, int32_t B,
                     int32_t n_max, float* mean_square_dev, void* stream);

/* MFCC front-end.  Replaces AudioFeaturizer._compute_mfcc (masr/data_utils/featurizer/audio_featurizer.py:98-117:
 * torchaudio.compliance.kaldi.mfcc(num_mel_bins=n_mels=80, num_ceps=n_mfcc, frame 25/10 ms, dither 0)) behind the same
 * AudioSegment handling as masr_fbank_batch (featurize(), :36-62).  mfcc_dev [B, T, n_ceps] f32, T = 1 + (n_max-400)/160. */
int masr_mfcc_batch(masr_engine* e, const void* samples_dev, int32_t sample_format, const int32_t* n_samples_dev, int32_t B,
                    int32_t n_max, int32_t use_db_normalization, float target_db, int32_t n_ceps, float* mfcc_dev,
                    int32_t* n_frames_dev, float* gain_dev, void* stream);
/* Linear log power spectrogram.  Replaces AudioFeaturizer._compute_linear (audio_featurizer.py:73-95; float64 arithmetic,
 * 20 ms Hann frames every 10 ms, 161 bins) on the float32 samples of the segment (:51-53).
 * feats_dev [B, T, 161] f32, T = (n_max-320)/160 + 1; n_frames_dev [B] = frames per utterance. */
int masr_linear_batch(masr_engine* e, const void* samples_dev, int32_t sample_format, const int32_t* n_samples_dev, int32_t B,
                      int32_t n_max, int32_t use_db_normalization, float target_db, float* feats_dev, int32_t* n_frames_dev,
                      float* gain_dev, void* stream);

/* Full-context encoder.  Replaces ConformerEncoder.forward called from
 * ConformerModel.get_encoder_out (masr/model_utils/conformer/model.py:152-167, encoder.py:305-346).
 *   feats_dev [B, T, n_mels] f32 (zero padded), feat_lens_dev [B] int32 (frames)
 *   decoding_chunk_size: -1 = full attention (get_encoder_out), >0 = chunk mask (encoder.forward(..., c, -1))
 *   enc_out_dev [B, T', d_model] f32, T' = ((T-1)/2-1)/2 (conv2d), ((T-1)/2-2)/3 (conv2d6), (((T-1)/2-1)/2-1)/2 (conv2d8);
 *   the Efficient Conformer's stride layer halves T' once more, (T'+1)/2 -- masr_encoder_frames gives it for any model */
int masr_encode_full(masr_engine* e, const float* feats_dev, const int32_t* feat_lens_dev, int32_t B, int32_t T,
                     int32_t decoding_chunk_size, float* enc_out_dev, void* stream);

/* CTC head.  Replaces CTCLoss.softmax (masr/model_utils/loss/ctc.py:62-70): probs = softmax(Linear).
 *   enc_dev [M, d_model] -> probs_dev [M, V] ; optional per-frame argmax / max-prob outputs */
int masr_ctc_probs(masr_engine* e, const float* enc_dev, int32_t M, float* probs_dev, int32_t* argmax_dev,
                   float* maxprob_dev, void* stream);
/* Same head without materialising probs for the caller: per-frame (argmax, max prob) only --
 * all that greedy_decoder (masr/decoders/ctc_greedy_decoder.py:20-21) reads from probs. */
int masr_ctc_greedy_frames(masr_engine* e, const float* enc_dev, int32_t M, int32_t* argmax_dev, float* maxprob_dev,
                           void* stream);
/* Best-path collapse + score.  Replaces the list logic of greedy_decoder
 * (ctc_greedy_decoder.py:20-30): tokens_dev [B, Tp] (-1 padded), n_tokens_dev [B],
 * score_dev [B] = fp32 sequential mean of the non-blank max-probs (caller multiplies by 100).
 * n_frames_dev [B] (may be NULL = all Tp frames, the reference's batch behaviour trainer.py:340).
 * Tp > 16384 is refused by name, nothing launched (the kernel stages Tp max-probs in dynamic LDS); masr_transcribe_batch /
 * masr_transcribe_rows and masr_pool_step refuse the same way. */
int masr_ctc_collapse(masr_engine* e, const int32_t* argmax_dev, const float* maxprob_dev, const int32_t* n_frames_dev,
                      int32_t B, int32_t Tp, int32_t blank, int32_t* tokens_dev, int32_t* n_tokens_dev,
                      float* score_dev, void* stream);
/* Stand-alone argmax/max-prob over host-provided probabilities already on the device
 * (greedy_decoder's np.argmax, ctc_greedy_decoder.py:20). */
int masr_argmax_rows(masr_engine* e, const float* probs_dev, int32_t M, int32_t V, int32_t* argmax_dev,
                     float* maxprob_dev, void* stream);

/* CTC forced alignment: when each token of a hypothesis was spoken (an addition: the reference has no such function).  Per
 * utterance the best path through the CTC trellis of its hypothesis -- extended labels blank, y1, blank, ..., yL, blank
 * (S = 2 L + 1 states, blank = id 0); transitions stay, advance by one, skip the blank between two DIFFERENT tokens; the path starts
 * in state 0 or 1 and ends in state S - 1 or S - 2 -- whichever decoder produced the hypothesis.
 *   post_dev [B, T', V] f32: input_is_log = 1: log-probabilities (the kernel only adds and compares float32 values, so a float32
 *     restatement on a CPU matches to the bit); 0: probabilities as masr_ctc_probs writes them, the kernel takes the logarithm
 *     itself and a probability <= 0 (or NaN) counts as MASR_ALIGN_NEG
 *   n_frames_dev [B] valid frames, tokens_dev [B, Lmax] with n_tokens_dev [B] ids in [1, V); frames behind n_frames[b] and slots
 *     behind n_tokens[b] are never read
 *   start_dev / end_dev [B, Lmax] int32: first and last frame (inclusive) the path spends in the token's state; peak_dev [B, Lmax]
 *     f32: the token's largest log-probability over those frames; score_dev [B]: the path's log-probability
 *   status_dev [B]: 0 = aligned; 1 = the trellis has no path: n_frames < L + (number of adjacent equal tokens); 2 = n_frames /
 *     n_tokens outside [0, T'] / [0, Lmax] or a token id outside [1, V).  With status != 0, and behind n_tokens[b] always, start / end
 *     are -1 and peak / score 0.  L = 0 aligns to the all-blank path (n_frames = 0: score 0).
 * Tie rule (part of the contract): the predecessor of a state is taken in the order stay, s - 1, s - 2, and a later candidate
 * replaces an earlier one only if STRICTLY greater; at the end state S - 1 wins a tie against S - 2.  "Unreachable" is the finite
 * MASR_ALIGN_NEG, never an infinity; a hypothesis whose best path crosses a zero probability scores <= MASR_ALIGN_NEG / 2 and its
 * frames mean nothing.
 * One workgroup per utterance; per frame only the L + 1 needed columns of the V-wide row are read.  The predecessor choices
 * ([B, T', 2 Lmax + 1] bytes) live in a workspace of the engine's CURRENT lane (masr_select_lane): two passes on two lanes never
 * share it.  Refused (non-zero, masr_last_error): Lmax > MASR_ALIGN_MAX_TOKENS (the trellis rows in LDS hold S <= 2 * that + 1),
 * Lmax > T', V > 16384. */
#define MASR_ALIGN_NEG (-1.0e30f)
#define MASR_ALIGN_MAX_TOKENS 1024
int masr_ctc_align(masr_engine* e, const float* post_dev, int32_t input_is_log, int32_t B, int32_t Tp, int32_t V,
                   const int32_t* n_frames_dev, const int32_t* tokens_dev, const int32_t* n_tokens_dev, int32_t Lmax,
                   int32_t* start_dev, int32_t* end_dev, float* peak_dev, float* score_dev, int32_t* status_dev, void* stream);
/* The same alignment over frames that are NOT contiguous: frame t of utterance b is row frame_row_dev[b, t] of the matrix
 * rows_dev [n_rows, V] -- the posterior history of streaming sessions, whose chunks land wherever the row pool had room, so that
 * nothing has to be packed into a dense [B, T', V] batch before it is aligned (the kernel reads L + 1 values per frame; a packed
 * copy would move whole V-wide rows of every session on every step).
 *   frame_row_dev [B, Tmax] int64: row numbers in frame order; they need be neither contiguous nor increasing, and a row may
 *     appear more than once.  Entries behind n_frames[b] are never read.
 *   A row number outside [0, n_rows) among the n_frames[b] valid frames gives status 2 for THAT utterance (start / end -1,
 *     peak / score 0) before any of its rows is read; the other utterances are not disturbed.
 *   Every address made from a row number is 64-bit: n_rows * V * 4 bytes may exceed 2^31.
 * Everything else -- the trellis, the tie rule, MASR_ALIGN_NEG, input_is_log, the status codes, one workgroup per utterance, the
 * predecessor workspace ([B, Tmax, 2 Lmax + 1] bytes of the CURRENT lane) -- is masr_ctc_align's: it is the same kernel with
 * another way to find a frame, and the outputs equal, bit for bit, those of masr_ctc_align on the gathered dense copy.  Refused
 * alike: Lmax > MASR_ALIGN_MAX_TOKENS, Lmax > Tmax, V > 16384; and n_rows <= 0.  The row number of a frame is fetched once per
 * frame and workgroup, two frames ahead of its use. */
int masr_ctc_align_rows(masr_engine* e, const float* rows_dev, int64_t n_rows, int32_t V, int32_t input_is_log,
                        const int64_t* frame_row_dev, int32_t B, int32_t Tmax, const int32_t* n_frames_dev,
                        const int32_t* tokens_dev, const int32_t* n_tokens_dev, int32_t Lmax, int32_t* start_dev, int32_t* end_dev,
                        float* peak_dev, float* score_dev, int32_t* status_dev, void* stream);

/* External n-gram language model scorer of the beam search.  Replaces the `Scorer` of paddlespeech_ctcdecoders (scorer.cpp on
 * KenLM; constructed in masr/decoders/beam_search_decoder.py:29-35, swig_wrapper.py:4-18; parameters alpha / beta of
 * configs/conformer.yml:74-88).  Character-based ARPA models up to order 5; `vocab_utf8` = the model's vocabulary tokens (the
 * LM words are matched to them by string; <s> / </s> get ids V / V + 1; n-grams with words the model cannot emit are dropped).
 * KenLM binaries are not parsed (returns non-zero, masr_lm_last_error()).  The table is uploaded to a GPU on first use there.
 *   masr_lm_cond_log_prob      ln P(ids[n-1] | ids[..n-2]) as Scorer::get_log_cond_prob scores the <s>-padded n-gram
 *                              (OOV_SCORE = -1000 as soon as one word is unknown to the LM)
 *   masr_lm_sentence_log_prob  Scorer::get_sent_log_prob: sum over the words and </s> */
typedef struct masr_lm masr_lm;
int masr_lm_load_arpa(const char* path, const char* const* vocab_utf8, int32_t V, masr_lm** out);
void masr_lm_destroy(masr_lm* lm);
const char* masr_lm_last_error(void);
int masr_lm_info(const masr_lm* lm, int32_t* max_order, int64_t* n_ngrams, int32_t* char_based, int64_t* skipped);
int masr_lm_cond_log_prob(const masr_lm* lm, const int32_t* ids, int32_t n, float* out);
int masr_lm_sentence_log_prob(const masr_lm* lm, const int32_t* ids, int32_t n, float* out);
/* Word-based models (an LM word longer than one character: Scorer::is_character_based() false, scorer.cpp load_lm): the words get
 * their own ids -- masr_lm_word_id (-1: not an LM word; the two scoring calls above then take word ids) -- and the scorer owns the
 * spelling dictionary of Scorer::fill_dictionary (every LM word spelled with vocabulary tokens + the space token);
 * masr_lm_dict_size = the number of words in it (Scorer::get_dict_size, printed by beam_search_decoder.py:38-42). */
int masr_lm_word_id(const masr_lm* lm, const char* word_utf8, int32_t* id);
int masr_lm_dict_size(const masr_lm* lm, int32_t* dict_size);

/* CTC prefix beam search.  Replaces BeamSearchDecoder.* -> paddlespeech_ctcdecoders
 * (masr/decoders/beam_search_decoder.py:45-96, swig_wrapper.py:35-121; third-party, un-vendored: parity
 * unpinned, external LM scorer not implemented = the alpha 0 path).
 * masr_ctc_topk (GPU): per-frame vocabulary pruning (cutoff_prob / cutoff_top_n, conformer.yml:74-88):
 *   idx_dev/logp_dev [M, top_n] candidates in descending probability (log(p + FLT_MIN)), count_dev [M].
 * masr_beam_* (host, like the reference's C++ thread pool): prefix search over those candidates.
 *   offline batch: masr_beam_search_batch over [B, T_stride, K] candidate arrays, frames_host [B] valid frames,
 *   tokens_host [B, max_len] out, len_host [B], score_host [B] = log probability of the best prefix;
 *   streaming: masr_beam_create / advance / result / reset / destroy (decode_chunk, reset_decoder). */
typedef struct masr_beam masr_beam;
int masr_ctc_topk(masr_engine* e, const float* probs_dev, int32_t M, int32_t V, int32_t top_n, float cutoff_prob,
                  int32_t* idx_dev, float* logp_dev, int32_t* count_dev, void* stream);
/* the same + blank_logp_dev [M] = ln p(blank) of every frame: the input of the decoder's pruning rule when an external scorer is
 * bound (ctc_beam_search_decoder.cpp: with a full beam, (prefix, c) is skipped once log p(c) + score(prefix) <
 * min_cutoff = score(worst live prefix) + ln p(blank) - max(0, beta)).  The *_lm searches below take that array
 * (blank_logp_*; NULL = rule off, every candidate of a frame is scored -- not what the reference decoder does). */
int masr_ctc_topk_blank(masr_engine* e, const float* probs_dev, int32_t M, int32_t V, int32_t top_n, float cutoff_prob,
                        int32_t blank, int32_t* idx_dev, float* logp_dev, int32_t* count_dev, float* blank_logp_dev,
                        void* stream);
int masr_beam_create(int32_t beam_size, int32_t blank, masr_beam** out);
void masr_beam_destroy(masr_beam* h);
int masr_beam_reset(masr_beam* h);
int masr_beam_advance(masr_beam* h, const int32_t* idx_host, const float* logp_host, const int32_t* count_host,
                      int32_t T, int32_t K);
int masr_beam_advance_lm(masr_beam* h, const int32_t* idx_host, const float* logp_host, const int32_t* count_host,
                         const float* blank_logp_host, int32_t T, int32_t K);
int masr_beam_result(masr_beam* h, int32_t* tokens_host, int32_t max_len, int32_t* len, float* score);
/* binds the external scorer (or NULL) and restarts the search: a prefix extended by a character adds
 * alpha * ln P_LM(character | last words of the prefix) + beta to its score (ctc_beam_search_decoder.cpp); the reported score is
 * the decoder's approx_ctc (scorer share removed again).  The *_lm variants of the batch searches take the same three values. */
int masr_beam_set_lm(masr_beam* h, const masr_lm* lm, float alpha, float beta);
int masr_beam_search_batch(const int32_t* idx_host, const float* logp_host, const int32_t* count_host,
                           const int32_t* frames_host, int32_t B, int32_t T_stride, int32_t K, int32_t beam_size,
                           int32_t blank, int32_t num_threads, int32_t* tokens_host, int32_t max_len, int32_t* len_host,
                           float* score_host);
int masr_beam_search_batch_lm(const int32_t* idx_host, const float* logp_host, const int32_t* count_host,
                              const int32_t* frames_host, int32_t B, int32_t T_stride, int32_t K, int32_t beam_size,
                              int32_t blank, int32_t num_threads, const masr_lm* lm, float alpha, float beta,
                              const float* blank_logp_host, int32_t* tokens_host, int32_t max_len, int32_t* len_host,
                              float* score_host);

/* CTC prefix beam search of a whole batch ON THE GPU (one workgroup per utterance; live prefixes, candidate scores and
 * the top-`beam_size` selection live in LDS, trie nodes of survivors in HBM).  Same inputs as masr_beam_search_batch but
 * DEVICE pointers (the outputs of masr_ctc_topk stay on the device), same outputs (token ids of the best prefix, its
 * length and log probability) as device arrays.  Replaces ctc_beam_search_decoding_batch of the third-party
 * paddlespeech_ctcdecoders (masr/decoders/swig_wrapper.py:67-103, beam_search_decoder.py:59-73), LM-free.
 * Limits: cutoff_top_n <= 64, beam_size <= 512, beam_size * cutoff_top_n * 6 B + tables <= 160 KB of LDS; returns non-zero (masr_last_error) beyond them -- use masr_beam_search_batch then. */
int masr_beam_search_gpu(masr_engine* e, const int32_t* idx_dev, const float* logp_dev, const int32_t* count_dev,
                         const int32_t* frames_dev, int32_t B, int32_t T_stride, int32_t K, int32_t beam_size,
                         int32_t blank, int32_t* tokens_dev, int32_t max_len, int32_t* len_dev, float* score_dev,
                         void* stream);
/* the same with the external scorer applied inside the kernel (LM table, known-word map in HBM; every live prefix carries its
 * packed last words, matched context length and backoff weights in LDS) */
int masr_beam_search_gpu_lm(masr_engine* e, const int32_t* idx_dev, const float* logp_dev, const int32_t* count_dev,
                            const int32_t* frames_dev, int32_t B, int32_t T_stride, int32_t K, int32_t beam_size,
                            int32_t blank, masr_lm* lm, float alpha, float beta, const float* blank_logp_dev,
                            int32_t* tokens_dev, int32_t max_len, int32_t* len_dev, float* score_dev, void* stream);

/* Streaming variant: a device-resident search per stream.  masr_gbeam_advance consumes the pruned candidates of the next T
 * frames (device arrays from masr_ctc_topk) and returns the best prefix so far (tokens/len/score device arrays); the
 * live prefixes and the trie nodes stay on the device between calls.  Replaces CTCBeamSearchDecoder.next / decode / reset
 * of the third-party module (masr/decoders/swig_wrapper.py:106-121, beam_search_decoder.py:75-96), LM-free.
 * max_frames bounds the number of frames of one utterance (trie node pool = max_frames * beam_size). */
int masr_gbeam_open(masr_engine* e, int32_t beam_size, int32_t blank, int32_t max_frames, int32_t* handle);
int masr_gbeam_advance(masr_engine* e, int32_t handle, const int32_t* idx_dev, const float* logp_dev,
                       const int32_t* count_dev, int32_t T, int32_t K, int32_t* tokens_dev, int32_t max_len,
                       int32_t* len_dev, float* score_dev, void* stream);
int masr_gbeam_advance_lm(masr_engine* e, int32_t handle, const int32_t* idx_dev, const float* logp_dev,
                          const int32_t* count_dev, const float* blank_logp_dev, int32_t T, int32_t K, int32_t* tokens_dev,
                          int32_t max_len, int32_t* len_dev, float* score_dev, void* stream);
int masr_gbeam_reset(masr_engine* e, int32_t handle);
int masr_gbeam_close(masr_engine* e, int32_t handle);
/* external scorer of a streaming search (between utterances only: after open or reset) */
int masr_gbeam_set_lm(masr_engine* e, int32_t handle, masr_lm* lm, float alpha, float beta);

/* The N best prefixes of the GPU search (csrc/beam_nbest.hip): a second, small kernel (one 512-thread workgroup per utterance) over
 * what the search left on the device -- the live set it persists when it ends and the trie nodes of its survivors.  The search
 * itself is untouched, so its own result stays what it is.  Order: the search's own best pick -- higher score first (the search
 * score, scorer share included); of bit-equal scores the smaller last character; of equal (score, character) the smaller live
 * index -- so entry 0 is the search's result bit for bit.  Outputs (device arrays): tokens_dev [B, nbest, max_len] (positions
 * below max_len only), len_dev / score_dev [B, nbest] with the conventions of masr_beam_search_gpu (with a scorer: approx_ctc where
 * the prefix fits max_len), count_dev [B] = min(nbest, live prefixes); rows past count have len 0, score -inf, tokens untouched.
 * masr_beam_nbest_gpu reads the workspace of the last masr_beam_search_gpu(_lm) on the SAME stream of this engine (the stream
 * orders the two).  Non-zero (masr_last_error, nothing launched): no search on that stream yet, B or beam_size other than that
 * search's, lm_or_null other than the scorer it had bound (or, with it, alpha / beta other than that search's), nbest outside 1 .. beam_size, max_len < 1, a null output.
 * masr_gbeam_nbest: the same for a streaming search after at least one masr_gbeam_advance since open or reset, with the stream's
 * own scorer, alpha and beta. */
int masr_beam_nbest_gpu(masr_engine* e, int32_t B, int32_t beam_size, int32_t nbest, masr_lm* lm_or_null, float alpha, float beta,
                        int32_t* tokens_dev, int32_t max_len, int32_t* len_dev, float* score_dev, int32_t* count_dev, void* stream);
int masr_gbeam_nbest(masr_engine* e, int32_t handle, int32_t nbest, int32_t* tokens_dev, int32_t max_len, int32_t* len_dev,
                     float* score_dev, int32_t* count_dev, void* stream);

/* Silero VAD network (the segmentation model of MASRPredictor.predict_long).  Replaces the onnxruntime session of the reference's
 * VADPredictor (masr/infer_utils/vad_predictor.py:36 InferenceSession(silero_vad.onnx), :83-104 session.run per window): the
 * weights are read out of the user's copy of that ONNX file by the host side (masr_amd/infer_utils/silero_vad.py) and handed
 * over tensor by tensor (names and shapes: csrc/silero.hip masr_vad_finalize), per sample rate (the file holds a 16 kHz and an
 * 8 kHz model).  masr_vad_forward runs B sequences x n_win consecutive windows of `window` samples (audio_dev [B, n_win * window]
 * float32, zero-padded by the caller like vad_predictor.py:126-127) from the LSTM state h_dev / c_dev [2, B, 64] (updated in
 * place: the reference's self._h / self._c) to probs_dev [B, n_win] -- n_win = 1 is one session.run, n_win = all windows of a
 * recording is the loop of get_speech_timestamps (:122-129) in two launches.  No CPU path: masr_vad_create fails without a GPU. */
typedef struct masr_vad masr_vad;
int masr_vad_create(int32_t device_id, masr_vad** out);
void masr_vad_destroy(masr_vad* v);
const char* masr_vad_last_error(void);
int masr_vad_load_tensor(masr_vad* v, int32_t sample_rate, const char* name, const float* data_host, int64_t n);
int masr_vad_finalize(masr_vad* v, int32_t sample_rate);
int masr_vad_forward(masr_vad* v, int32_t sample_rate, const float* audio_dev, int32_t B, int32_t n_win, int32_t window,
                     float* h_dev, float* c_dev, float* probs_dev, void* stream);

/* One call for the whole offline hot path (MASRPredictor.predict semantics, masr/predict.py:167-192,
 * batched like MASRTrainer.evaluate, trainer.py:632): PCM -> fbank -> encoder -> CTC greedy.
 * decode_all_frames != 0 reproduces the reference batch quirk of decoding padded frames. */
int masr_transcribe_batch(masr_engine* e, const int16_t* pcm_dev, const int32_t* n_samples_dev, int32_t B,
                          int32_t n_max, int32_t use_db_normalization, float target_db, int32_t decode_all_frames,
                          int32_t* tokens_dev, int32_t* n_tokens_dev, float* score_dev, void* stream);
/* The same pass as the facade drives it (MASRPredictor.predict / predict_batch, masr/predict.py:167-192): samples in either
 * format of masr_fbank_batch, use_db_normalization 0 / 1 / 2 with its meaning there (2: gains SUPPLIED in gain_dev [B], read
 * only -- the bit-exact int16 route of AudioSegment.normalize, audio.py:287-304), and the hypotheses as ONE packed int32 row per
 * utterance, rows_dev [B, T' + 2] = token ids (-1 padded) | token count | score bits (f32), so that a caller needs ONE copy
 * back per pass (T' = encoder frames of n_max samples, halved once more for the Efficient Conformer). */
int masr_transcribe_rows(masr_engine* e, const void* samples_dev, int32_t sample_format, const int32_t* n_samples_dev, int32_t B,
                         int32_t n_max, int32_t use_db_normalization, float target_db, const float* gain_dev,
                         int32_t decode_all_frames, int32_t* rows_dev, void* stream);

/* Serving pool: any number of concurrent predict_stream sessions on one engine, ONE call per step.  Replaces, per session, the
 * stream framing of MASRPredictor.predict_stream (masr/predict.py:237-343: carried-over samples re-normalised on every call,
 * :274-281; feature frames cached until a 67-frame decoding window is full, :283-306; 3 overlap frames kept, :329; the greedy
 * decoder's history, decoders/ctc_greedy_decoder.py:52-89) and, across sessions, the one-predictor-per-websocket loop of
 * infer_server.py:103-156 -- all sessions fed since the last step share one upload, one feature launch, lock-step chunk steps
 * (masr_encode_chunk), one collapse launch and one copy back.  Greedy decoding; a handle is the engine's stream id.
 *   masr_pool_create: feature_method 0 fbank / 1 mfcc (n_mfcc) / 2 linear (audio_featurizer.py:51-69), use_db_normalization and
 *                     target_db of preprocess_conf, max_frames_out as in masr_stream_open
 *   masr_pool_step:   the feeds since the last step, in order: feed_handle[k], feed_samples[k] (host memory: int16 PCM, format 0,
 *                     scaled by 1 / 2^15 like buf_to_float, data_utils/utils.py:382-411; or float32, format 1), feed_n[k] samples,
 *                     feed_is_end[k] (a session's flags are OR-ed).  gain_fn: evaluator of AudioSegment.normalize's scalar
 *                     expressions (audio.py:287-304,519-529) on the mean squares the device returns -- the python facade passes
 *                     its numpy evaluation, which is what makes the normalised samples bit-identical to the reference's on the
 *                     same host; NULL = libm (log10f / powf).  Returns non-zero to abort the step (gain beyond max_gain_db).
 *                     All feeds are validated (known handle, format, 0 <= feed_n <= 2^28, non-null samples) before any session
 *                     state changes: a rejected call commits nothing.
 *                     Out: the sessions of the step in first-fed order (handles_out[i], state_out[i] = 1 when the session
 *                     advanced by at least one window, 0 = the reference returns None; then, state -1, the sessions LEFT OUT of
 *                     the step because their stream has no room for the frames it would emit -- their feeds of this step are
 *                     dropped, their state is untouched, the other sessions advance), and for the advanced ones, in that
 *                     order, packed rows [row_width] = token ids (-1 padded) | count | score bits, in pinned host memory
 *                     (rows_host) and in HBM (rows_dev: what a multi-GPU front-end all-gathers); all out pointers stay valid
 *                     until the next step of this pool. */
typedef struct masr_pool masr_pool;
typedef int (*masr_gain_fn)(const float* mean_square, int32_t n, float target_db, float* gain_out, void* user);
int masr_pool_create(masr_engine* e, int32_t feature_method, int32_t n_mfcc, int32_t use_db_normalization, float target_db,
                     int32_t max_frames_out, masr_pool** out);
void masr_pool_destroy(masr_pool* p);
int masr_pool_open(masr_pool* p, int32_t* handle);
int masr_pool_close(masr_pool* p, int32_t handle);
int masr_pool_reset(masr_pool* p, int32_t handle);      /* MASRPredictor.reset_stream, predict.py:346-353 */
int masr_pool_step(masr_pool* p, int32_t n_feeds, const int32_t* feed_handle, const void* const* feed_samples,
                   const int64_t* feed_n, const int32_t* feed_format, const int32_t* feed_is_end, masr_gain_fn gain_fn,
                   void* gain_user, int32_t* n_sessions, const int32_t** handles_out, const int32_t** state_out,
                   const int32_t** rows_host, int32_t* row_width, int32_t** rows_dev, void* stream);
/* Sessions fed OFF the model's sample rate (8 kHz telephony, 44.1 / 48 kHz recordings): the step resamples their feeds on the
 * device.  Replaces the per-chunk AudioSegment.resample of the stream facade (masr/predict.py:260-281 ->
 * masr/data_utils/audio.py:306-317) that a caller of masr_pool_step runs on the host, one chunk at a time.
 *   masr_pool_set_rate:   registers a source rate once per pool -> *slot.  ratio = model rate / sr_orig, table_host [nwin][2]
 *                         float64 (win, dwin) pairs as masr_resample_rows takes them, uploaded here with synchronous copies: the
 *                         first feed of a new source rate blocks on the device once (at most 64 rates per pool).  The pool
 *                         does not know the model's rate: a ratio that is not model rate / sr_orig is the caller's mistake.
 *                         Idempotent per sr_orig: a second call returns the slot of the first and ignores its other arguments.
 *   masr_pool_step_rates: masr_pool_step with feed_rate_slot[k]: -1 = the feed is at the model's rate (handled exactly as by
 *                         masr_pool_step, which is this call with feed_rate_slot == NULL); a slot = feed_samples[k] are feed_n[k]
 *                         samples AT THE SOURCE RATE, staged raw; the feed gives (int)(feed_n * ratio) samples (every length of
 *                         the step's bookkeeping is known on the host), resampled on its own (no filter state across feeds, like
 *                         the reference) by ONE masr_resample_feeds launch for all off-rate feeds of the step, behind the upload
 *                         and ahead of the mean squares, with no additional synchronisation; the carried-over samples of such a
 *                         session return through pinned memory.  Refused before any state changes, on top of masr_pool_step's
 *                         checks: an unknown slot, a feed too short to give one sample. */
int masr_pool_set_rate(masr_pool* p, int32_t sr_orig, double ratio, const double* table_host, int64_t nwin, int32_t num_table,
                       int32_t* slot);
int masr_pool_step_rates(masr_pool* p, int32_t n_feeds, const int32_t* feed_handle, const void* const* feed_samples,
                         const int64_t* feed_n, const int32_t* feed_format, const int32_t* feed_is_end,
                         const int32_t* feed_rate_slot, masr_gain_fn gain_fn, void* gain_user, int32_t* n_sessions,
                         const int32_t** handles_out, const int32_t** state_out, const int32_t** rows_host, int32_t* row_width,
                         int32_t** rows_dev, void* stream);
/* diagnostics: host time of masr_pool_step per phase, accumulated over `steps` calls (ms): assemble the samples | upload + mean
 * squares + wait | gains | features + frame bookkeeping | windows (lock-step chunk steps enqueued) | collapse + copy back + wait */
int masr_pool_profile(masr_pool* p, double* phase_ms, int64_t* steps, int32_t reset);
/* The decoding windows a session with n_frames pending feature frames advances by in one step (csrc/pool_plan.h: the function the
 * step's room check and its lock-step loop use; predict.py:283-306): 67-frame windows a stride of 64 apart, and at the end of a
 * stream (is_end != 0) a short last window while 7 frames remain.  No pool, no engine, no GPU; no process state is read or written.
 *   first_last [cap][2]: (first, last) of the first min(cap, *n_windows) windows; *n_windows: always the full count */
int masr_pool_window_plan(int32_t n_frames, int32_t is_end, int32_t* first_last, int32_t cap, int32_t* n_windows);
/* encoder frames that T feature frames give (Conv2dSubsampling4 / 6 / 8 by masr_config.reserved[3], subsampling.py:65-211; halved once more behind the Efficient
 * Conformer's stride layer) and the engine's geometry -- what a host needs to size the buffers above */
int masr_encoder_frames(masr_engine* e, int32_t feature_frames, int32_t* encoder_frames);
/* nominal time reduction of the loaded model, in feature frames per encoder frame: 4 / 6 / 8 by the input layer (DeepSpeech2's two
 * stride-2 convs: 4), doubled by the Efficient Conformer's stride layer; the Squeezeformer's reduce / recover pair cancels.  For large
 * F, masr_encoder_frames(F + r) - masr_encoder_frames(F) == 1.  Encoder frame t starts at feature frame r * t: what turns the frames
 * of masr_ctc_align into times. */
int masr_frame_reduction(masr_engine* e, int32_t* feature_frames_per_encoder_frame);
int masr_engine_info(masr_engine* e, int32_t* device_id, int32_t* n_mels, int32_t* vocab_size);

/* Streaming.  Replaces InferencePredictor.predict_chunk_conformer / reset_stream
 * (inference_predictor.py:80-102) -> ConformerEncoder.forward_chunk (encoder.py:348-420) with
 * required_cache_size < 0 (keep all history, predict.py:312-313).  Stream state (attention KV
 * cache, conv cache, offset) lives in the engine; `n` streams advance in lock-step per call.
 *   stream_ids [n] host int32, feats_dev [n, Tc, n_mels] (Tc <= 67), probs_dev [n, Tc', V] */
int masr_stream_open(masr_engine* e, int32_t max_frames_out, int32_t* stream_id);
int masr_stream_reset(masr_engine* e, int32_t stream_id);
int masr_stream_close(masr_engine* e, int32_t stream_id);
/* required_cache_size of forward_chunk for one stream (conformer/encoder.py:397-410): < 0 (default) every cached key stays
 * visible -- what MASRPredictor.predict_stream passes (predict.py:312-313); >= 0 a chunk attends over at most that many cached
 * keys, in frames of the encoder's input rate (Conformer, Squeezeformer: squeezeformer/encoder.py:292-297,338-347, and
 * Efficient-Conformer: efficient_conformer/encoder.py:323-336,365-381 -- their half-rate layers follow the reference's
 * next_cache_start // 2 trimming of the repeat-interleaved cache).  masr_stream_export_cache then returns the kept rows;
 * masr_stream_cache_len = their number (att_cache.size(2) of the reference after the last step). */
int masr_stream_set_history(masr_engine* e, int32_t stream_id, int32_t required_cache_size);
int masr_stream_offset(masr_engine* e, int32_t stream_id, int32_t* offset);
int masr_stream_cache_len(masr_engine* e, int32_t stream_id, int32_t* cache_len);
/* Subsampled frames the stream can still take before masr_encode_chunk refuses it (max_frames_out / the positional table's
 * max_len, conformer/embedding.py:48-50): lets a caller that advances many streams in one call leave a full one out instead of
 * failing the call. */
int masr_stream_room(masr_engine* e, int32_t stream_id, int32_t* frames_left);

/* Host side of the boundary: the utterances of one device pass -- B separate host arrays src[i] of n_samples[i] samples of
 * sample_bytes (2: int16 PCM, 4: float32) -- into ONE padded staging buffer dst [B rows of row_bytes], the rest of every row
 * zeroed: the padded batch the reference's collate_fn forms (masr/data_utils/collate_fn.py:6-34), built on the audio so that a
 * single transfer brings the pass to the device.  `threads` (1..16) library-owned worker threads take rows in turn; dst is
 * normally pinned memory.  No engine, no GPU. */
int masr_stage_rows(void* dst, int64_t row_bytes, const void* const* src, const int32_t* n_samples, int32_t B, int32_t sample_bytes,
                    int32_t threads);

/* Host-side resampling of one utterance to the model's rate.  Replaces resampy.resample(samples, sr, target, filter) behind
 * AudioSegment.resample (masr/data_utils/audio.py:306-317; resampy is third-party: its published band-limited sinc interpolation
 * is restated, parity unpinned).  x [n_orig] float32 host, ratio = sr_new / sr_orig, win / dwin [nwin] the right wing of the
 * windowed sinc (already scaled by ratio when ratio < 1) and its first differences, num_table samples per zero crossing,
 * y [n_out] with n_out = (int)(n_orig * ratio).  No engine, no GPU: an input-format step in front of the hot path. */
int masr_resample_f32(const float* x, int64_t n_orig, double ratio, const double* win, const double* dwin, int64_t nwin,
                      int32_t num_table, float* y, int64_t n_out);
/* The same resampling on the device, for the rows of ONE source rate of a device pass.  Replaces, per row, resampy.resample behind
 * AudioSegment.resample (masr/data_utils/audio.py:306-317) with the arithmetic of masr_resample_f32, operation for operation (one
 * thread per output sample; no fused multiply-add, denormals kept): every row comes out bit for bit as the host entry makes it
 * (third-party algorithm restated, parity unpinned, as above).
 *   src_dev    [R, src_stride] int16 PCM (sample_format 0, scaled by 2^-15 in the kernel) or float32 (1), at the source rate
 *   rows_host / rows_dev [R][3] int32, the same table in host and in device memory: samples in | samples out = (int)(samples in *
 *              ratio), computed by the caller | destination row.  The host copy is read during the call only
 *   table_dev  [nwin][2] float64: (win[k], dwin[k]) pairs of the filter as masr_resample_f32 takes them (scaled by ratio when
 *              ratio < 1); NULL with ratio == 1: the rows are at the target rate already and are converted and copied
 *   dst_dev    [dst_rows, dst_stride] float32: row rows[i][2] receives the resampled row i and zeros from its length to dst_stride
 * Returns non-zero (masr_last_error) where masr_resample_f32 returns 1 -- a ratio that is not positive, index_step <= 0, a row whose
 * last output would read at or beyond its input (n >= n_orig) -- and for rows that do not fit their buffers; nothing is launched
 * then.  Launches on `stream`, never synchronises. */
int masr_resample_rows(masr_engine* e, const void* src_dev, int32_t sample_format, int64_t src_stride, const int32_t* rows_host,
                       const int32_t* rows_dev, int32_t R, double ratio, const double* table_dev, int64_t nwin, int32_t num_table,
                       float* dst_dev, int32_t dst_rows, int64_t dst_stride, void* stream);
/* The same resampling for MANY SHORT FEEDS OF MIXED RATES in one launch: the chunks a streaming pool was fed since its last step
 * (8 kHz telephony next to 44.1 / 48 kHz recordings), each landing at its own offset inside a session's row.  Replaces, per feed,
 * the resample of the stream facade (masr/predict.py:260-281 -> AudioSegment.resample, masr/data_utils/audio.py:306-317): every
 * feed is resampled on its own, no filter state carried from chunk to chunk, bit for bit as masr_resample_f32 makes it.
 *   masr_resample_feed  one feed: src_offset (bytes into src_dev; 2-byte aligned for int16 PCM, 4-byte for float32), format
 *                       (0 int16 PCM, scaled by 2^-15 in the kernel / 1 float32), n_in samples at the source rate, n_out =
 *                       (int)(n_in * ratio) samples written to dst[dst_row][dst_offset .. dst_offset + n_out) and NOTHING else
 *                       (no zero tails), rate_slot = index into the rate table
 *   masr_resample_rate  one source rate: what masr_resample_rows derives per call, derived once by masr_resample_rate_fill from
 *                       (ratio, table_dev [nwin][2] float64 (win, dwin) pairs, nwin, num_table)
 *   tiles               [n_tiles][2] int32 = (feed, first output): a workgroup owns up to 256 consecutive outputs of one feed, so
 *                       a short feed costs one workgroup, whatever the longest feed.  masr_resample_plan (host only, no engine, no
 *                       GPU) validates the feeds and builds the list: tiles == NULL counts (n_tiles), else at most tiles_cap
 *                       entries are written.  It returns 0, or non-zero with *bad_feed (-1: not about one feed) and *why (static
 *                       text) for: an unknown rate slot, a rate that masr_resample_rate_fill did not make, a bad format, an
 *                       unaligned or out-of-range source, n_out != (int)(n_in * ratio), a last output that would read at or beyond
 *                       its input (n >= n_orig), a destination range outside its row.
 *   masr_resample_feeds feeds / rates / tiles in host AND device memory (the same tables; the host copies are read during the call
 *                       only).  Everything is validated (masr_resample_plan, and tiles_host against the list it builds) before
 *                       anything is launched.  ONE launch on `stream`, never synchronises. */
typedef struct masr_resample_feed {
    int64_t src_offset;
    int32_t format, n_in, n_out, dst_row, dst_offset, rate_slot;
} masr_resample_feed;
typedef struct masr_resample_rate {
    double ratio, time_increment, scale;
    const double* table_dev;
    int32_t index_step, nwin, num_table, reserved;
} masr_resample_rate;
#define MASR_RESAMPLE_TILE 256          /* outputs per workgroup */
#define MASR_RESAMPLE_LDS_FLOATS 16000 /* a tile's inputs are staged in LDS up to this span, read from global memory beyond */
int masr_resample_rate_fill(double ratio, const double* table_dev, int64_t nwin, int32_t num_table, masr_resample_rate* out);
/* input samples one tile of a rate can touch (its span / ratio + both filter wings): what the launcher compares with
 * MASR_RESAMPLE_LDS_FLOATS */
int64_t masr_resample_tile_span(const masr_resample_rate* rate);
int masr_resample_plan(const masr_resample_feed* feeds, int32_t n_feeds, const masr_resample_rate* rates, int32_t n_rates,
                       int64_t src_bytes, int32_t dst_rows, int64_t dst_stride, int32_t* tiles, int64_t tiles_cap, int64_t* n_tiles,
                       int32_t* bad_feed, const char** why);
int masr_resample_feeds(masr_engine* e, const void* src_dev, int64_t src_bytes, const masr_resample_feed* feeds_host,
                        const masr_resample_feed* feeds_dev, int32_t n_feeds, const masr_resample_rate* rates_host,
                        const masr_resample_rate* rates_dev, int32_t n_rates, const int32_t* tiles_host, const int32_t* tiles_dev,
                        int64_t n_tiles, float* dst_dev, int32_t dst_rows, int64_t dst_stride, void* stream);
int masr_encode_chunk(masr_engine* e, const int32_t* stream_ids, int32_t n, const float* feats_dev, int32_t Tc,
                      float* probs_dev, int32_t* argmax_dev, float* maxprob_dev, void* stream);
/* The same chunk step, which also hands out its encoder rows: enc_out_dev [n, Tq, d_model] (Tq = the step's encoder frames per
 * stream, the row count of probs_dev) receives exactly the rows the step's CTC head read -- what an attention second pass at the
 * end of the utterance attends over (masr_rescore_rows).  The final LayerNorm writes where it always did and ONE device-to-device
 * copy of n * Tq * d_model floats follows the CTC head on `stream`; every launch in front of it is masr_encode_chunk's, so probs /
 * argmax / maxprob and the streams' caches equal masr_encode_chunk's bit for bit.  masr_encode_chunk itself runs what it ran.
 * Conformer (the width-generic 512 / 8 path included), Squeezeformer and Efficient Conformer (there Tq is the half-rate count).
 * Refused by name: DeepSpeech2 (no attention decoder), a null enc_out_dev. */
int masr_encode_chunk_enc(masr_engine* e, const int32_t* stream_ids, int32_t n, const float* feats_dev, int32_t Tc,
                          float* probs_dev, int32_t* argmax_dev, float* maxprob_dev, float* enc_out_dev, void* stream);
/* Read back a stream's caches in the reference layout (for parity tests):
 * att [L, H, t, 2*dk], cnn [L, 1, d, kernel-1] -- device pointers, t = current offset.  DeepSpeech2: att <- h [L, rnn_size],
 * cnn <- c [L, rnn_size]; a GRU stream returns h in both (deepspeech2/gru.py: final_state_c = final_state_h). */
int masr_stream_export_cache(masr_engine* e, int32_t stream_id, float* att_dev, float* cnn_dev, void* stream);

/* Single kernels, exposed for unit tests and profiling. */
int masr_op_layernorm(masr_engine* e, const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev,
                      int32_t M, float eps, void* stream);
int masr_op_gemm(masr_engine* e, const float* a_dev, const float* w_dev, const float* bias_dev, const float* res_dev,
                 float* c_dev, int32_t M, int32_t N, int32_t K, int32_t act, float alpha, void* stream);
/* The two packed-row forms of the CTC collapse, which otherwise run only inside masr_transcribe_rows (in_rows NULL) and
 * masr_pool_step (in_rows given): rows_dev [B, Tp + 2] = tokens (-1 padded) | token count | score bits, the values masr_ctc_collapse
 * gives.  in_rows_dev_or_null [B]: utterance b reads row in_rows[b] of argmax_dev / maxprob_dev, whose rows are ld_in frames apart
 * (ld_in is not read without it: the rows are then Tp apart).  n_frames_dev [B] is required.  Non-zero: a null pointer, B < 0,
 * Tp < 0, ld_in < Tp, Tp > 16384. */
int masr_op_ctc_collapse_rows(masr_engine* e, const int32_t* argmax_dev, const float* maxprob_dev, const int32_t* n_frames_dev,
                              const int32_t* in_rows_dev_or_null, int32_t ld_in, int32_t B, int32_t Tp, int32_t blank,
                              int32_t* rows_dev, void* stream);
/* The n-best kernel of masr_beam_nbest_gpu on a host-supplied live set and node pool, LM-free: per utterance n_live_host [B] live
 * prefixes with node_host / ch_host / score_host [B, beam_size] (entries below n_live are read) over pool_parent_host /
 * pool_ch_host [B, pool_cap]; outputs as above but HOST arrays (tokens_host is read first: positions no row writes come back as
 * given).  Returns when done.  Non-zero: a null pointer, B < 1, beam_size outside 1 .. 512, pool_cap outside 1 .. 2^24, nbest
 * outside 1 .. beam_size, max_len < 1, an n_live outside 0 .. beam_size, a live node outside [0, pool_cap), a pool node (>= 1)
 * whose parent is not below it. */
int masr_op_beam_nbest(masr_engine* e, const int32_t* n_live_host, const int32_t* node_host, const int32_t* ch_host,
                       const float* score_host, const int32_t* pool_parent_host, const int32_t* pool_ch_host, int32_t B,
                       int32_t beam_size, int32_t pool_cap, int32_t nbest, int32_t* tokens_host, int32_t max_len, int32_t* len_host,
                       float* score_host_out, int32_t* count_host);
/* One relative-position attention launch on the caller's buffers: builds the per-sequence descriptor table from the host arrays
 * [nseq] and calls the launcher the encoder calls, so the process-wide switches (keys 7, 14, 26, 28) pick the kernel as they do
 * in a forward pass.  group = 1: q rows of q_stride floats, k / v rows of kv_stride floats (>= heads * 64), out rows of heads * 64;
 * key j of a sequence reads positional row pos0 + pos_stride * j of ptab_dev [n_pos, heads * 64].  group = 3 (4 heads): q / k / v /
 * out are planar, zero-padded [3 * nq, 256] = [nq, 4, 192] buffers (both strides 768), ptab frames pos0 .. pos0 + t_true - 1 are
 * read and frames from t_true on count as zero, pos_stride is not used.  *_off: element offsets of a sequence's first row from the
 * buffer's pointer; keys j >= klen are masked; chunk_size > 0 adds the chunk mask of query q_abs0 + i (group 3: of frame 3 i).
 * Returns when the launch has finished.  Non-zero: a null pointer, nseq <= 0, heads other than 4 / 8, group other than 1 / 3, a
 * negative count or offset, klen > nk, a stride below heads * 64, strides / offsets / pointers that are not 16-byte aligned, a
 * positional table shorter than the rows the keys name. */
int masr_op_attention(masr_engine* e, const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev,
                      const float* ptab_dev, int32_t n_pos, const float* bias_u_dev, const float* bias_v_dev, int32_t nseq,
                      const int64_t* q_off, const int64_t* k_off, const int64_t* v_off, const int64_t* out_off, const int32_t* nq,
                      const int32_t* nk, const int32_t* klen, const int32_t* pos0, const int32_t* q_abs0, int32_t heads,
                      int32_t q_stride, int32_t kv_stride, int32_t chunk_size, int32_t pos_stride, int32_t group, int32_t t_true,
                      void* stream);
/* The same for the plain attention of pos_enc_layer_type abs_pos / no_pos (score = q . k^T / sqrt(64): no positional table, no
 * biases; group 1 only): launch_attention's instantiations with the positional term compiled out, chosen by the same switches
 * (keys 7, 28; key 14 has nothing to act on).  pos_stride scales the chunk mask only.  Same refusals, under the same name. */
int masr_op_attention_plain(masr_engine* e, const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, int32_t nseq,
                            const int64_t* q_off, const int64_t* k_off, const int64_t* v_off, const int64_t* out_off,
                            const int32_t* nq, const int32_t* nk, const int32_t* klen, const int32_t* q_abs0, int32_t heads,
                            int32_t q_stride, int32_t kv_stride, int32_t chunk_size, int32_t pos_stride, void* stream);

/* Attention decoder (second pass, `decoder: attention_rescoring`).  Replaces BiTransformerDecoder.forward
 * (masr/model_utils/transformer/decoder.py:68-99: left_decoder, and right_decoder on the reversed hypotheses) + the
 * log_softmax / gather / sum of WeNet's attention_rescoring, for the n-best prefixes of the CTC search.
 *   masr_decoder_enable  before masr_load_tensor / masr_finalize: from then on the engine keeps the `decoder.left_decoder.*` and
 *                        `decoder.right_decoder.*` tensors and masr_finalize uploads them (fused q | k | v and source k | v
 *                        projections).  An engine that never calls it ignores those names, allocates and launches exactly what
 *                        it did before.  attention_heads / linear_units / num_blocks / r_num_blocks = the YAML decoder_conf; the
 *                        checkpoint has to hold exactly num_blocks left and r_num_blocks right blocks of these shapes
 *                        (masr_finalize names the tensor or the key that disagrees).  Refused by name: model kind 3 (DeepSpeech2:
 *                        its `decoder.` prefix is the CTC head), heads other than d_model / 64, linear_units no positive multiple
 *                        of 32, num_blocks < 1, r_num_blocks < 0.  The numbers are checked before the engine is touched.
 *                        A later masr_finalize that again carries decoder tensors replaces the whole set (the old weights are
 *                        freed after the device has drained); one that fails midway leaves the engine without a decoder.
 *   masr_rescore         enc_dev [B, Tp, d_model] (the encoder output of a pass), enc_lens_dev [B] valid encoder frames, hyp_dev
 *                        [B, N, Lmax] int32 token ids, hyp_lens_dev [B, N] (0 <= L <= Lmax; ids past L are never read) ->
 *                        att_dev, r_att_dev [B, N] f32: sum over the L + 1 positions of log_softmax(logits)[target] of the left
 *                        and (with_right != 0; else zeros) the right decoder, sos = eos = vocab_size - 1.  Runs on `stream` and
 *                        the active lane's workspaces, never synchronises.  A hypothesis' scores do not depend on N, B, the other
 *                        hypotheses, the ids past its length or the lane.  Refused: N outside 1 .. 64, Lmax > max_pos - 1
 *                        (hypotheses longer than max_pos - 1), B * N > 65535, with_right without a right decoder.
 *   masr_rescore_rows    masr_rescore over frames that are NOT contiguous: frame t of utterance b is row frame_row_dev[b, t] of
 *                        the matrix rows_dev [n_rows, d_model] -- the kept encoder output of streaming sessions
 *                        (masr_encode_chunk_enc), whose chunks land wherever the row pool had room, so that nothing is packed into
 *                        a dense [B, Tmax, d_model] block before the second pass at the end of an utterance.
 *                          frame_row_dev [B, Tmax] int64: row numbers in frame order; they need be neither contiguous nor
 *                            increasing, and a row may appear more than once, in one utterance or in several.  n_frames_dev [B]
 *                            takes enc_lens_dev's place.  Entries behind n_frames[b] are never used: they may be any number.
 *                          A row number outside [0, n_rows) among the valid frames (the -1 padding, too) stands for a frame of
 *                            zeros and is never dereferenced.
 *                          Every address made from a row number is 64-bit: n_rows * d_model * 4 bytes may exceed 2^31.
 *                        Only the per-layer source k | v projection differs: the tiled f32 GEMM reads its A rows through the
 *                        table (one fetch of the row number per row and thread, ahead of the K loop) on the tile shape the dense
 *                        projection takes at the same size, so every output element sees the same MFMA chain and att_dev /
 *                        r_att_dev equal, bit for bit, masr_rescore's on the gathered block rows[frame_row] with enc_lens =
 *                        n_frames.  Everything else -- the hypothesis table, sos / eos, with_right, the active lane's workspaces,
 *                        never synchronising -- is masr_rescore's.  Refused alike (under its own name), and: n_rows <= 0,
 *                        Tmax < 1, B * Tmax > 2^31 - 1.  (The bit equality holds in the product configuration: the row-table
 *                        operand has no split-bf16 variant, so with the experimental masr_debug_set key 20 on, which moves
 *                        masr_rescore's dense projection to that variant, the two differ by its rounding.)
 *   masr_op_decoder_scores  the same launches driven alone, from HOST tables (hyp_host, hyp_lens_host, enc_lens_host), every
 *                        entry validated (lengths in [0, Lmax], ids in [0, vocab_size), frames in [1, Tp]); outputs to host
 *                        arrays; returns when the work has finished.
 *   masr_decoder_info    enabled | left blocks | right blocks | bytes of decoder weights on the device | bytes of decoder
 *                        workspace of the ACTIVE lane (0 until its first masr_rescore / masr_attention_decode /
 *                        masr_op_decoder_step / masr_joint_decode(_lm) / masr_op_ctc_prefix_scores / masr_op_lm_scores; the step
 *                        workspaces of the search, the CTC prefix states and the LM candidate scores of the joint search are
 *                        counted).  Null outputs are skipped. */
int masr_decoder_enable(masr_engine* e, int32_t attention_heads, int32_t linear_units, int32_t num_blocks, int32_t r_num_blocks);
int masr_rescore(masr_engine* e, const float* enc_dev, const int32_t* enc_lens_dev, int32_t B, int32_t Tp, const int32_t* hyp_dev,
                 const int32_t* hyp_lens_dev, int32_t N, int32_t Lmax, int32_t with_right, float* att_dev, float* r_att_dev,
                 void* stream);
int masr_rescore_rows(masr_engine* e, const float* rows_dev, int64_t n_rows, const int64_t* frame_row_dev,
                      const int32_t* n_frames_dev, int32_t B, int32_t Tmax, const int32_t* hyp_dev, const int32_t* hyp_lens_dev,
                      int32_t N, int32_t Lmax, int32_t with_right, float* att_dev, float* r_att_dev, void* stream);
int masr_op_decoder_scores(masr_engine* e, const float* enc_dev, const int32_t* enc_lens_host, int32_t B, int32_t Tp,
                           const int32_t* hyp_host, const int32_t* hyp_lens_host, int32_t N, int32_t Lmax, int32_t with_right,
                           float* att_host, float* r_att_host, void* stream);
int masr_decoder_info(masr_engine* e, int32_t* enabled, int32_t* num_blocks, int32_t* r_num_blocks, int64_t* weight_bytes,
                      int64_t* workspace_bytes);

/* Attention decoding (`decoder: attention`): left-to-right beam search driven by the LEFT decoder alone, one decoder row per
 * hypothesis and step (TransformerDecoder.forward_one_step, masr/model_utils/transformer/decoder.py:233-270), everything on the
 * device.  sos = eos = vocab_size - 1; N = beam_size.  Per utterance b over its valid frames enc[b, :enc_lens[b]]:
 *   start    N hypotheses [sos] with scores [0, -inf, ..., -inf], none finished.
 *   step i   logp = log_softmax(output_layer(after_norm(x_last))) of every hypothesis; its top N, the LARGER value first and of
 *            bit-equal values the SMALLER token id first.  A hypothesis whose last token is eos offers (0, eos), (-inf, eos), ...
 *            instead.  Candidate score = hypothesis score + logp; the top N of the utterance's N x N candidates, of bit-equal
 *            scores (-inf included) the SMALLER flat index parent_rank * N + candidate_rank first; the new hypotheses are parent +
 *            token in that order.  (torch.topk leaves the order of ties open; these rules are this library's.)
 *   stop     after limit_b = min(enc_lens[b], max_len when max_len > 0, max_pos - 1, Lcap) steps -- per utterance, so that an
 *            utterance's result is that of the same search run on it alone -- or earlier when all N are finished.  Steps past
 *            that add +0 and eos and change no result.
 *   result   per rank n (best first): tokens_dev [B, N, Lcap] = the tokens behind sos up to and excluding the first eos (eos from
 *            there on), lens_dev [B, N] their count, scores_dev [B, N] the summed log-probability.  The best hypothesis is rank
 *            0 (the highest score, an exact tie to the earlier rank).  No CTC score, no length penalty (masr_joint_decode below
 *            adds both), no right decoder.
 * Self-attention k | v of a position are projected once and kept per layer ([blocks][steps][B * N][2 d]); reordering the beam
 * rewrites a small ancestor table, never the cache.  The encoder k | v projection is one GEMM per layer before the loop.
 *   masr_attention_decode  enc_dev [B, Tp, d_model], enc_lens_dev [B] -> the result above; *steps_host_or_null = steps launched.
 *                        Runs on `stream` and the active lane's workspaces.  The only host round trip is the end poll: every
 *                        MASR_ATTENTION_POLL steps (environment, read per call; default 8, 0 = never) the host waits for the
 *                        count of utterances still running and stops launching at 0; results do not depend on it.  A hypothesis'
 *                        tokens and score are bit-identical whatever B, the other utterances, Tp or the lane: every launch is row-
 *                        local or per utterance, and the tiled f32 GEMM accumulates an element over K in the same order in each of
 *                        its tile shapes (the shape is chosen by the row count).  This does not extend to the experimental split-
 *                        bf16 GEMM (masr_debug_set, experiment builds only).  Memory: the self-attention cache holds blocks x
 *                        steps x B x N x 2 d_model floats for steps = min(Tp, Lcap, max_len, max_pos - 1) (488 MB at 32 utterances
 *                        of 248 frames, beam 10, 3 blocks, d_model 256): the caller bounds it through max_len or Lcap, and a
 *                        failed allocation is reported by name.  Refused by name:
 *                        no decoder (masr_decoder_enable), beam_size outside 1 .. 64 or above vocab_size, B * beam_size > 65535,
 *                        Lcap < 1, max_len < 0.
 *   masr_op_decoder_step  the step's launches driven alone from HOST tables (teacher forced): prefix_host [B * N, L] tokens behind
 *                        sos, prefix_lens_host [B * N] in 0 .. L, enc_lens_host [B] in 1 .. Tp, ids in [0, vocab_size), every
 *                        entry validated.  The prefixes are fed one position at a time through the same launches and the same
 *                        k | v cache as the search (row s is its own ancestor); each row reports at its last position:
 *                        top_ids_host / top_logp_host [B * N, top_n] (top_n in 1 .. min(64, vocab_size)) and, when given,
 *                        logp_host_or_null [B * N, vocab_size].  Returns when the work has finished. */
int masr_attention_decode(masr_engine* e, const float* enc_dev, const int32_t* enc_lens_dev, int32_t B, int32_t Tp, int32_t beam_size,
                          int32_t max_len, int32_t* tokens_dev, int32_t Lcap, int32_t* lens_dev, float* scores_dev,
                          int32_t* steps_host_or_null, void* stream);
int masr_op_decoder_step(masr_engine* e, const float* enc_dev, const int32_t* enc_lens_host, int32_t B, int32_t Tp,
                         const int32_t* prefix_host, const int32_t* prefix_lens_host, int32_t N, int32_t L, int32_t top_n,
                         int32_t* top_ids_host, float* top_logp_host, float* logp_host_or_null, void* stream);
/* Joint CTC / attention decoding (`decoder: joint`): the search of masr_attention_decode -- its step launches, k | v cache, tie
 * rules, step limit, early stop and end poll -- ranked by a key that adds the CTC prefix probability of every hypothesis over the
 * utterance's valid frames and a length bonus.  Every hypothesis carries A (the sum of its attention log-probabilities), psi (the
 * log of its CTC prefix probability) and n (its tokens other than eos); its key is
 *     J = ((1 - ctc_weight) * A + ctc_weight * psi) + length_bonus * n        float32, in that order;
 * with ctc_weight = 0 the psi term is left out and no CTC launch happens at all.  N = beam_size, M = ctc_candidates.
 *   step     per live hypothesis g: the top M of its attention log-probabilities (the order and tie rule of the top N above),
 *            psi(g . c) of those M candidates, J of each; a finished hypothesis offers itself once with its own A, psi, n and
 *            -inf otherwise.  Per utterance the top N of the N x M keys, of bit-equal keys the SMALLER parent_rank * M +
 *            candidate_rank first.
 *   result   per rank: tokens, length, J in scores_dev; A in att_or_null and psi in ctc_or_null [B, N] when given (psi is 0
 *            with ctc_weight = 0).  Hypotheses still unfinished at the limit are returned as they stand.
 * The prefix score, over the utterance's frames t = 0 .. T - 1 (T = enc_lens[b]), lp = ln of the CTC posterior, blank = id 0:
 *   state    r_n[t], r_b[t]: the log-probabilities of the alignments of g over frames 0 .. t that end in a non-blank / a blank.
 *   empty    r_n = -inf, r_b[t] = sum of lp[0 .. t][blank], psi = 0.
 *   c        neither blank nor eos; phi[t] = r_b(g)[t] when c equals the last token of g, else logaddexp(r_n(g)[t], r_b(g)[t]).
 *            r_n'[0] = lp[0][c] when g is empty, else -inf;  r_b'[0] = -inf;  psi' = r_n'[0];  for t >= 1:
 *            r_n'[t] = logaddexp(r_n'[t - 1], phi[t - 1]) + lp[t][c]
 *            r_b'[t] = logaddexp(r_n'[t - 1], r_b'[t - 1]) + lp[t][blank]
 *            psi'    = logaddexp(psi', phi[t - 1] + lp[t][c])
 *   eos      c = vocab_size - 1 is always read as eos: psi' = logaddexp(r_n(g)[T - 1], r_b(g)[T - 1]).
 *   blank    -inf.  A prefix longer than the frames can carry comes out as -inf by this arithmetic.
 * All of it in float32 with logf / expf, sequential over t.  psi of a winner is the value the scorer produced for it as a
 * candidate: it is carried through the merge, never recomputed.
 *   masr_joint_decode    enc_dev [B, Tp, d_model], enc_lens_dev [B]; post_dev [B, Tp, vocab_size] the CTC posteriors as
 *                        masr_ctc_probs leaves them (input_is_log = 0: probabilities, the kernels take the logarithm and read an
 *                        entry that is not > 0 as -inf; 1: log-probabilities), an argument of its own, so a caller may pass
 *                        posteriors that did not come from enc_dev; only frames below enc_lens[b] are read.  Stream, lane, end
 *                        poll and the bit-for-bit independence of an utterance's result from B, its neighbours, Tp and the
 *                        lane are masr_attention_decode's.  With ctc_weight = 0, length_bonus = 0 and ctc_candidates =
 *                        beam_size the tokens and scores are masr_attention_decode's bit for bit.  Memory on top of that
 *                        search: the prefix states, 2 x B x N x 2 x Tp floats in the active lane's decoder workspace.  Refused
 *                        by name: what masr_attention_decode refuses, ctc_candidates outside beam_size .. min(64, vocab_size),
 *                        ctc_weight outside [0, 1), a length_bonus that is not finite, ctc_weight > 0 without post_dev.
 *   masr_op_ctc_prefix_scores  the scorer alone from HOST tables: R rows of (utterance index row_utt_host [R], prefix_host
 *                        [R, L] with prefix_lens_host [R] in 0 .. L, cand_host [R, M] candidate ids), frames_host [B] in
 *                        1 .. Tp, every entry validated (prefix ids in 1 .. vocab_size - 2, candidate ids in the vocabulary, M
 *                        in 1 .. 64).  The prefixes are fed one position at a time through the advance kernel;
 *                        psi_prefix_host [R] = psi of each prefix, psi_cand_host [R, M] = psi of each prefix extended by each
 *                        candidate.  Needs no attention decoder.  Returns when the work has finished.
 * Shallow fusion with an n-gram language model (masr_lm above; `joint_decoder_conf.language_model_path` / `lm_weight`): every
 * hypothesis carries a fourth part beside A, psi and n,
 *     Lm(g . c) = Lm(g) + lm(g, c)        float32, the sum added in that order; Lm of the empty hypothesis is 0,
 * and the key is
 *     J = ((((1 - ctc_weight) * A + ctc_weight * psi) + lm_weight * Lm) + length_bonus * n)        float32, in that order.
 *   lm(g, c) EXACTLY what masr_lm_cond_log_prob returns for the tokens of g (behind sos) followed by c: the <s>-padded window of
 *            the last max_order - 1 tokens (the empty hypothesis: <s> alone), natural logarithm, the ARPA backoff recursion,
 *            and -1000 (the scorer's OOV score, as it is) for a candidate or a context word the model does not know -- the same
 *            float32 additions in the same order, so the device's value is the host's bit for bit.  Candidate vocab_size - 1
 *            (eos) is scored as the model's </s>; every other token id is its own LM word id, as in the CTC beam search (blank
 *            and the other tokens that are no single character are unknown words).
 *   step     the M candidates of a hypothesis stay its top ctc_candidates by ATTENTION log-probability: the model is a partial
 *            scorer over the same M, like the CTC scorer.  A finished hypothesis offers itself once with its own J, A, psi, Lm,
 *            n.  Tie rules, step limit, early stop and end poll are unchanged.  Lm of a winner is the sum that ranked it as a
 *            candidate: carried through the merge, never recomputed.
 *   lm_weight = 0  the Lm term is left out and no LM kernel is launched, whether or not a model was passed: tokens and every
 *            score are masr_joint_decode's bit for bit (Lm comes back 0).  A model that is passed is still validated then: a
 *            word-based one or one of another vocabulary size is refused at lm_weight = 0 too.  With ctc_weight = 0 and
 *            lm_weight > 0 the call is attention + LM, still with no CTC launch and no use for post_dev.
 *   masr_joint_decode_lm  masr_joint_decode (which is this call with no model) with lm_or_null / lm_weight and lm_or_null_out
 *                        [B, N] = Lm per rank when given.  The model's table is uploaded to the engine's device on its first
 *                        use there, before the first launch of the call, and the host waits for that upload once.  One more
 *                        launch per step (one wave per hypothesis, lane m = candidate m) between the step's top M and the
 *                        merge; memory on top of masr_joint_decode: B x N x M floats.  Refused by name: everything
 *                        masr_joint_decode refuses, an lm_weight that is not finite or is negative, lm_weight > 0 without a
 *                        model, a word-based model (its words are spelt out of several tokens: host-thread CTC search only), a
 *                        model loaded for a vocabulary of another size than the engine's.
 *   masr_op_lm_scores    the LM score kernel alone from HOST tables: R rows (1 .. 65535) of prefix_host [R, L] with
 *                        prefix_lens_host [R] in 0 .. L and cand_host [R, M] (M in 1 .. 64), every entry validated (prefix and
 *                        candidate ids in [0, vocab_size); a candidate vocab_size - 1 is read as </s>, a prefix token
 *                        vocab_size - 1 as its own -- unknown -- word) -> out_host [R, M] = lm(prefix, candidate).  Needs no
 *                        attention decoder.  Returns when the work has finished. */
int masr_joint_decode(masr_engine* e, const float* enc_dev, const int32_t* enc_lens_dev, int32_t B, int32_t Tp, const float* post_dev,
                      int32_t input_is_log, int32_t beam_size, int32_t ctc_candidates, float ctc_weight, float length_bonus,
                      int32_t max_len, int32_t* tokens_dev, int32_t Lcap, int32_t* lens_dev, float* scores_dev, float* att_or_null,
                      float* ctc_or_null, int32_t* steps_host_or_null, void* stream);
int masr_op_ctc_prefix_scores(masr_engine* e, const float* post_dev, int32_t input_is_log, const int32_t* frames_host, int32_t B,
                              int32_t Tp, const int32_t* row_utt_host, const int32_t* prefix_host, const int32_t* prefix_lens_host,
                              int32_t R, int32_t L, const int32_t* cand_host, int32_t M, float* psi_prefix_host, float* psi_cand_host,
                              void* stream);
int masr_joint_decode_lm(masr_engine* e, const float* enc_dev, const int32_t* enc_lens_dev, int32_t B, int32_t Tp, const float* post_dev,
                         int32_t input_is_log, int32_t beam_size, int32_t ctc_candidates, float ctc_weight, float length_bonus,
                         masr_lm* lm_or_null, float lm_weight, int32_t max_len, int32_t* tokens_dev, int32_t Lcap, int32_t* lens_dev,
                         float* scores_dev, float* att_or_null, float* ctc_or_null, float* lm_or_null_out, int32_t* steps_host_or_null,
                         void* stream);
int masr_op_lm_scores(masr_engine* e, masr_lm* lm, const int32_t* prefix_host, const int32_t* prefix_lens_host, const int32_t* cand_host,
                      int32_t R, int32_t L, int32_t M, float* out_host, void* stream);
/* The N best prefixes of the LM-free host-thread search (masr_beam_search_batch's search, same pruned candidates): per utterance
 * tokens_host [B, nbest, max_len], len_host [B, nbest], score_host [B, nbest] = log probability of each prefix, count_host [B] =
 * prefixes returned (<= min(nbest, beam_size)), best first in the search's own order (score, then the smaller last character), so
 * entry 0 is masr_beam_search_batch's result. */
int masr_beam_search_batch_nbest(const int32_t* idx_host, const float* logp_host, const int32_t* count_host,
                                 const int32_t* frames_host, int32_t B, int32_t T_stride, int32_t K, int32_t beam_size,
                                 int32_t blank, int32_t num_threads, int32_t nbest, int32_t* tokens_host, int32_t max_len,
                                 int32_t* len_host, float* score_host, int32_t* nbest_count_host);

/* Side streams owned by the library: kind 0 / 1 = prefix searches of consecutive device passes, 2 = per-pass preparation (upload,
 * mean squares, gains), 3 = copies, 4 = the encoder passes of lane 1 (masr_select_lane).  One set per DEVICE, made with the first
 * masr_create on it and shared by every engine there; non-blocking, default priority.  The streams are CHOSEN BY PROBING which
 * hardware queue a candidate landed on (the runtime deals queues round-robin in creation order, so that depends on everything
 * the process created before): none of them shares the NULL stream's queue, kinds 0 and 1 are on different queues; kinds 0 and 4
 * are one stream (never used together), kinds 2 and 3 are one stream (short work only) -- see engine.hip.  The caller borrows them (torch.cuda.ExternalStream) and never destroys
 * them.  They take the place of the worker processes of the reference's batch decoder (masr/decoders/beam_search_decoder.py:59-73:
 * num_processes search workers beside the model's forward). */
#define MASR_SIDE_STREAMS 5
int masr_side_stream(masr_engine* e, int32_t kind, void** stream_out);

/* Lanes: an engine holds MASR_LANES sets of forward workspaces (activations, descriptor tables; ONE set of weights).  The calls
 * that follow masr_select_lane(e, k) use set k, so two offline passes of one engine can be in flight on two streams -- the
 * length-sorted device passes of a batch (the reference forms them one after the other: trainer.py:592-651 evaluates batch by
 * batch, predict.py:194-234 utterance by utterance) side by side: a pass whose row blocks do not fill the last round of a launch
 * leaves CUs to the other pass's kernels (BASELINE configs[2], two passes of 32: 17.0 -> 14.9 ms of encoder time).  Launches that
 * share a lane must be ordered by their stream, exactly as all launches of an engine had to be before; a set is allocated on its
 * lane's first use and sized by the largest pass it has seen.  Results do not depend on the lane.  Lane 0 is active after
 * masr_create; streaming sessions (masr_stream_*) keep their caches outside the lanes.  Not thread-safe, like every call. */
#define MASR_LANES 2
int masr_select_lane(masr_engine* e, int32_t lane);

/* Diagnostics: A/B switches of the kernels, for in-process measurements (tools/ *_ab.py); production = the defaults.
 * SCOPE: every key but 2, 16 and 38 is PROCESS-WIDE -- it holds for every engine of the process, whichever handle sets it; keys 2, 16
 * and 38 belong to the engine whose handle sets them.  key, name (masr_debug_key_info), meaning:
 *   1  ffn_variant: fused-FFN variant (0 production, 81 without weight loads)
 *   2  beam-search phase profile of workgroup 0 (per engine)
 *   5  no_chain: 1 = no out-proj + pw1 chain kernel                  6  rowgemm_small: 0 = no K-split projection kernel
 *   7  attention_fewq: 0 = always the query-tiled attention kernel   8  no_ffn_tail: 1 = no QKV tail stage on the first FFN
 *   9  no_ffn_head: 1 = no conv-module head stage on the second FFN
 *  12  rowgemm_small_blocks: row blocks below which the K-split projection kernel runs
 *  13  ffn_split_blocks: row blocks below which the FFN splits d_ff
 *  14  attention_fold: 0 = two-term attention scores (no positional-key fold)
 *  15  embed_split: 0 = the offline embed projection never splits K
 *  16  time every n-th matching launch (masr_profile_*; per engine)
 *  17  gemm_waves: waves per workgroup of the offline conv2 launch (8 | 4)
 *  18  conv1_nt: 0 = conv1 writes with plain instead of streaming stores
 *  19  hot_weights: timing experiment: every chunk-step layer on layer 0's weights
 *  20  bf16x3: 1 = EXPLORATORY split-bf16 precision mode (not the reference's fp32 arithmetic, never the contract path): conv2, the
 *      embed projection and the other launches of the generic GEMM in the offline forward as a_hi*w_hi + a_hi*w_lo + a_lo*w_hi on
 *      the bf16 matrix pipe, fp32 accumulation (csrc/gemm_bf16x3.hip); 3 = also the FFN, unfused (slower than the fused fp32 FFN)
 *  21  gemm_bf16x3_waves: waves per workgroup of the split-bf16 conv2 launch (8 | 4)
 *  22  ffn_x3_rotation: 0 = no per-workgroup chunk rotation in the split-bf16 FFN
 *  23  ffn_packed: 0 = the full FFN launches stream their weights through the wave-private LDS slabs instead of reading the packed
 *      copies straight into registers (bit-identical either way); 2 (default) = the d_ff-split launches read packed copies too
 *  24  ffn_dual: 1 = the full FFN launches run two accumulator chains per wave (ffn_dual.hip) instead of one (ffn_pc.hip;
 *      bit-identical)
 *  25  rowgemm_packed: 0 = the offline out-proj + pw1 chain kernel and the CTC head stream their weights through LDS slabs instead
 *      of reading packed copies with buffer loads (bit-identical)
 *  26  attention_grouped_fold: 0 = the two-wave, two-term grouped attention kernel
 *  27  ctc_fused_blocks: row blocks from which the fused CTC head runs
 *  28  attention_fewq_wgs: offline launches with fewer attention workgroups than this take the key-split kernel
 *  29  few_rows_path: 0 = offline Conformer layers of few row blocks keep the row-block chain kernel
 *  30  split_head: 1 = few rows: the conv-module head stage rides on the d_ff-split FFN launch
 *  31  efficient_fused: 0 = Efficient-Conformer layers keep separate out-proj / pw1 / dwconv / pw2 launches
 *  32  beam_lm_cache: 0 = the GPU prefix search probes the scorer once per (prefix, candidate) pair
 *  33  conv2_mid_fill: percent below which a thin last round of the 128x128 conv2 grid switches to 128x64 tiles (0 = never)
 *  34  attn_chain: 1 = offline Conformer layers run attention and the out-proj + pw1 chain as one launch
 *  35  ffn_coop: 1 = one-chunk d_ff slices of few rows run ffn_coop.hip
 *  36  sqz_fused_blocks: row blocks from which a full-context Squeezeformer layer runs the fused stage kernels (0 = never)
 *  37  beam_narrow: 0 = every frame of the GPU prefix search on the wide (1024-thread) step
 *  38  the offline Squeezeformer launches skip the all-padding row blocks of a batch (per engine; bits: 1 stage kernels, 2 conv2 +
 *      input projection, 4 attention; default 7, 0 = the padded frames are computed too)
 *  39  ffn16: 0 = the full packed FFN launches run the 32-row kernel instead of the 16-row one (two workgroups per CU; bit-identical)
 *  40  conv2_rows: 0 = the offline conv2 runs on 128x128 tiles instead of full-width 64-row blocks with packed weights
 *      (bit-identical)
 *  41  conv1_fused: 0 = conv1 runs as its own launch (writing its output to a workspace) instead of inside the A gather of the
 *      row-block conv2 (key 40; bit-identical)
 *  42  embed_rows: 0 = the K quarters of the offline embed projection run on 128x128 tiles instead of full-width 64-row blocks with
 *      packed weights (bit-identical)
 *  43  rnn_mfma_units: hidden units per workgroup of the DeepSpeech2 matrix-core recurrent step (4 < B <= 32): 8 = production (4
 *      units at rnn_size <= 512, 8 above); 16 = 16 units (GRU at rnn_size 1024 only); -8 = 8 units at every size (bit-identical: a
 *      column's dot product does not depend on the grouping)
 * At d_model 512 (masr_config.d_model) only the attention keys (7, 14, 28) and the tile choice of the tiled GEMM change the launches: the fused
 * FFN / row-block / chain keys select between kernels built for d_model 256.
 * Keys 20, 21, 22, 24, 30, 34 and 35 select experimental kernels: a build without MASR_BUILD_EXPERIMENTS=1 refuses a non-zero value.
 * masr_debug_reset puts every process-wide switch back to its default, and this engine's keys 16 and 38 (1 and 7); key 2 is left
 * alone.  masr_debug_key_info (no engine) describes row `index` of the table of process-wide switches -- its key, default,
 * whether it is experimental, and its name (a static string) -- and returns non-zero past the last row; null outputs are skipped. */
int masr_debug_set(masr_engine* e, int32_t key, int32_t value);
int masr_debug_reset(masr_engine* e);
int masr_debug_key_info(int32_t index, int32_t* key, int32_t* default_value, int32_t* experimental, const char** name);

/* Which kernel of the fused FFN family one FFN call on m rows launches, and how (csrc/ffn_plan.h: the function the engine itself
 * evaluates on the process's switches).  No engine and no GPU: the plan is computed on the DEFAULTS of the process-wide switches
 * with n_overrides (key, value) pairs from overrides [2 * n_overrides] applied to a local copy -- the process's switches are neither
 * read nor written, and experimental keys are accepted in every build.
 *   ask [5]:  affine prologue (Squeezeformer) | weight rows of the tail stage, 0 = none | 1 = planar tail output | depthwise taps
 *             of the head stage, 0 = none | head norm (0 LayerNorm, 1 folded BatchNorm)
 *   plan [9]: kernel (0 split-bf16, 1 cooperative split, 2 two-chain, 3 16-row, 4 32-row) | nsplit | chunks of 128 hidden units
 *             per slice | slices launched | packed weights | tail stage in the kernel | head stage in the kernel | head stage on
 *             the d_ff-split launch | masr_profile_select kind of the launch (2, 6 with tail, 7 with head)
 * Non-zero: d_ff no positive multiple of 128, m <= 0, an unknown key, a null argument. */
int masr_ffn_plan(int32_t d_model, int32_t d_ff, int32_t m, const int32_t* ask, const int32_t* overrides, int32_t n_overrides,
                  int32_t* plan);

/* Profiling: time every launch of one kernel class with HIP events on the launch stream.
 * kind: 0 none, 1 gemm (all), 2 ffn-w1 gemm, 3 conv2 gemm, 4 attention, 5 fbank, 8 the step loop of a DeepSpeech2 recurrent
 * layer (one "launch" = the T' step launches of one layer); the row kernels of the d_model 512 path (csrc/wide.hip): 9 LayerNorm,
 * 10 GLU, 11 depthwise conv + LayerNorm + SiLU, 12 the streaming cache kernels (conv history, key / value append).
 * masr_profile_read synchronises the events and returns total ms / launch count / flops since reset. */
int masr_profile_select(masr_engine* e, int32_t kind);
int masr_profile_read(masr_engine* e, double* total_ms, int64_t* launches, double* flops, int32_t reset);

/* Summation-order probe (no engine): c32_dev, c16_dev [16][16] = a_dev [16][k] . b_dev [16][k]^T as a chain of 32x32x2 MFMAs in the
 * fused FFN kernels' k order and as a chain of 16x16x4 MFMAs whose lanes take, in group g of 8 k, the k values 8g + perm[0..3]
 * (first MFMA, lane groups 0..3) and 8g + perm[4..7] (second MFMA).  k a multiple of 8. */
int masr_mfma_order_probe(const float* a_dev, const float* b_dev, float* c32_dev, float* c16_dev, int32_t k, const int32_t* perm,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
