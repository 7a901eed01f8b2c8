"""BeamSearchDecoder with the reference's constructor / method contract
(masr/decoders/beam_search_decoder.py:9-96).  The reference hands the search to the third-party SWIG
module ``paddlespeech_ctcdecoders`` (+ a KenLM language model); here the per-frame vocabulary pruning runs
on the GPU (masr_ctc_topk) and so does the CTC prefix beam search of whole utterances
(masr_beam_search_gpu_lm: one workgroup per utterance) and of streams (masr_gbeam_*: the live prefixes stay on the device
between decode_chunk calls); sizes beyond the kernel's limits use the host-thread search inside libmasr_hip.so
(masr_beam_*).

External scorer (alpha, beta): ``language_model_path`` is read as an ARPA n-gram model (decoders/lm_scorer.py; KenLM's binary
.klm format is not parsed -> an error that says so).  Character-based models (every LM word one character, the reference's
Mandarin models) are applied inside the search on the GPU table or the host table: a prefix extended by a character adds
alpha * ln P_LM + beta.  Word-based models (an LM word longer than one character, the English configurations): the scorer owns
the spelling dictionary, a word is scored when its space arrives and the unfinished last word at the end of the utterance;
that search runs on host threads.  With a scorer bound the decoder's min_cutoff / full_beam pruning applies (ln p(blank) of
every frame comes out of the pruning kernel).  The returned score is the decoder's approx_ctc.

A missing language model file: the reference downloads its default model and otherwise ASSERTS
(beam_search_decoder.py:19-28) -- there is no network here, so the assertion is what a caller sees.  The scorer-free search
(alpha = beta = 0, no pruning rule) is still available, but only when asked for: ``language_model_path=None``."""
import ctypes as C
import logging
import os

import numpy as np
import torch

from masr_amd import _lib, runtime
from masr_amd._lib import check

logger = logging.getLogger(__name__)


class BeamSearchDecoder:
    def __init__(self, alpha, beta, beam_size, cutoff_prob, cutoff_top_n, vocab_list, num_processes=10, blank_id=0,
                 language_model_path='lm/zh_giga.no_cna_cmn.prune01244.klm'):
        self.alpha, self.beta = alpha, beta
        self.beam_size = int(beam_size)
        self.cutoff_prob = float(cutoff_prob)
        self.cutoff_top_n = int(cutoff_top_n)
        self.vocab_list = vocab_list
        self.num_processes = int(num_processes)
        self.blank_id = int(blank_id)
        self.use_gpu_search = True       # False: prefix search on host threads (masr_beam_search_batch)
        self._gstream = None             # device-resident streaming search (masr_gbeam_*), opened on first use
        self._geng = None                # ... and the (per-device) auxiliary engine that owns it
        self._gout = None
        self.last_tokens = []            # token ids of the last decode_chunk result
        self.last_nbest, self.last_nbest_tokens = [], []     # decode_chunk(nbest=N): [(score, text)] and [token ids], best first
        self._lib = _lib.lib()
        self._ext_scorer = None
        self.prune_min_cutoff = True     # the decoder's min_cutoff / full_beam rule (only ever applies with a scorer bound)
        if language_model_path is None:
            # explicit scorer-free mode (not a reference configuration: its decoder always owns a Scorer)
            logger.info('masr_amd BeamSearchDecoder: language_model_path=None, searching with the acoustic CTC scores only')
            self.alpha = self.beta = 0
        else:
            import os
            # beam_search_decoder.py:28 (the download of the default model that precedes it needs a network)
            assert os.path.exists(language_model_path), f'语言模型不存在：{language_model_path}'
            from masr_amd.decoders.lm_scorer import LanguageModel
            self._ext_scorer = LanguageModel(language_model_path, vocab_list)
            logger.info(f'language model: model path = {language_model_path}, is_character_based = '
                        f'{self._ext_scorer.is_character_based}, max_order = {self._ext_scorer.get_max_order()}, '
                        f'dict_size = {self._ext_scorer.get_dict_size()}')
        h = C.c_void_p()
        if self._lib.masr_beam_create(self.beam_size, self.blank_id, C.byref(h)) != 0:
            raise _lib.MasrError('masr_beam_create failed')
        self._stream = h
        self._bind_host_lm()

    def _lm_args(self):
        """(lm handle or NULL, alpha, beta) for the *_lm entry points"""
        if self._ext_scorer is None:
            return C.c_void_p(0), C.c_float(0.0), C.c_float(0.0)
        return self._ext_scorer.h, C.c_float(float(self.alpha)), C.c_float(float(self.beta))

    def _bind_host_lm(self):
        if self._ext_scorer is not None:
            self._lib.masr_beam_set_lm(self._stream, *self._lm_args())

    def fork(self):
        """a decoder with the same configuration (and the same language model tables) but its own streaming search state --
        one per concurrent ``predict_stream`` session (serving.StreamPool)"""
        other = object.__new__(BeamSearchDecoder)
        other.__dict__.update(self.__dict__)
        other._gstream, other._geng, other._gout, other.last_tokens = None, None, None, []
        other.last_nbest, other.last_nbest_tokens = [], []
        h = C.c_void_p()
        if self._lib.masr_beam_create(self.beam_size, self.blank_id, C.byref(h)) != 0:
            raise _lib.MasrError('masr_beam_create failed')
        other._stream = h
        other._bind_host_lm()
        return other

    def close(self):
        """release the streaming search state (host trie + device-resident beam)"""
        if getattr(self, '_gstream', None) is not None:
            check(self._lib.masr_gbeam_close(self._geng.h, self._gstream))
            self._gstream = self._geng = None
        if getattr(self, '_stream', None):
            self._lib.masr_beam_destroy(self._stream)
            self._stream = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- GPU: per-frame candidate pruning ----------------------------------------------------------
    def _candidates(self, probs, to_host=True):
        """probs np/torch [M, V] -> idx [M,K] int32, logp [M,K] f32, count [M] int32, blank_lp [M] f32 or None, K (host arrays,
        or device tensors).  blank_lp = ln p(blank) per frame, produced when a scorer is bound (the pruning rule's input)."""
        # device-resident probabilities are searched on the GPU they live on (one worker thread per GPU, server.WorkerRouter)
        eng = runtime.aux_engine(probs.device if torch.is_tensor(probs) and probs.is_cuda else None)
        p = torch.as_tensor(np.asarray(probs) if not torch.is_tensor(probs) else probs, dtype=torch.float32)
        p = p.to(eng.device).contiguous()
        M, V = p.shape
        K = min(self.cutoff_top_n, V)
        idx = torch.zeros(M, K, dtype=torch.int32, device=eng.device)
        logp = torch.zeros(M, K, dtype=torch.float32, device=eng.device)
        cnt = torch.zeros(M, dtype=torch.int32, device=eng.device)
        blp = None
        if self._ext_scorer is not None and self.prune_min_cutoff:
            blp = torch.zeros(max(M, 1), dtype=torch.float32, device=eng.device)
        if M:
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if blp is None:
                check(self._lib.masr_ctc_topk(eng.h, C.c_void_p(p.data_ptr()), M, V, K, C.c_float(self.cutoff_prob),
                                              C.c_void_p(idx.data_ptr()), C.c_void_p(logp.data_ptr()),
                                              C.c_void_p(cnt.data_ptr()), stream))
            else:
                check(self._lib.masr_ctc_topk_blank(eng.h, C.c_void_p(p.data_ptr()), M, V, K, C.c_float(self.cutoff_prob),
                                                    self.blank_id, C.c_void_p(idx.data_ptr()), C.c_void_p(logp.data_ptr()),
                                                    C.c_void_p(cnt.data_ptr()), C.c_void_p(blp.data_ptr()), stream))
        if not to_host:
            return idx, logp, cnt, blp, K
        return idx.cpu().numpy(), logp.cpu().numpy(), cnt.cpu().numpy(), None if blp is None else blp.cpu().numpy(), K

    @staticmethod
    def _ptr(x):
        """device tensor / host array / None -> void* for the C ABI"""
        if x is None:
            return C.c_void_p(0)
        return C.c_void_p(x.data_ptr()) if torch.is_tensor(x) else x.ctypes.data_as(C.c_void_p)

    def gpu_search_supported(self, T, V):
        """limits of masr_beam_search_gpu (include/masr_hip.h): LDS-resident entry table and 32-bit trie keys; word-based
        scorers (spelling dictionary) are searched on host threads."""
        K = min(self.cutoff_top_n, V)
        lm = self._ext_scorer is not None
        if lm and not self._ext_scorer.is_character_based:
            return False
        # beam_gpu_lds_bytes (beam_gpu.hip): extension keys + survivor list, 29 (+ 15 with a scorer) words of live-prefix state,
        # fixed tables
        return (K <= 64 and 2 <= self.beam_size <= 512 and
                self.beam_size * K * 6 + (176 if lm else 116) * self.beam_size + 24752 <= 160 * 1024)

    def _text(self, toks):
        return ''.join(self.vocab_list[t] for t in toks).replace('<space>', ' ')

    # ---- reference API -----------------------------------------------------------------------------
    def decode_beam_search_offline(self, probs_split):
        """one utterance: probs [T, V] -> (score, text)  (beam_search_decoder.py:45-56)."""
        score, text = self._batch([np.asarray(probs_split)])[0]
        return score, text

    def decode_batch_beam_search_offline(self, probs_split):
        """list of [T_i, V] -> list of texts (beam_search_decoder.py:59-73), num_processes host threads."""
        return [t for _, t in self._batch([np.asarray(p) for p in probs_split])]

    def _pinned_out(self, n):
        """a pinned host buffer of >= n int32 for the results of one deferred search, from a small free list"""
        pool = self.__dict__.setdefault('_pin_free', [])
        for i, b in enumerate(pool):
            if b.numel() >= n:
                return pool.pop(i)
        return torch.empty(max(n, 1 << 15), dtype=torch.int32, pin_memory=True)

    def _results(self, toks, lens, scores, want_tokens):
        """host arrays of a search -> [(token ids, score)] (what a multi-GPU caller gathers instead of text, and what is aligned)
        or [(score, text)]"""
        ids = [toks[i, :lens[i]].tolist() for i in range(len(lens))]
        if want_tokens:
            return [(ids[i], float(scores[i])) for i in range(len(ids))]
        return [(float(scores[i]), self._text(ids[i])) for i in range(len(ids))]

    def _unpacked(self, rows, max_len, want_tokens):
        """packed host rows [B, max_len + 2] int32 = tokens | length | score bits -> results"""
        return self._results(rows[:, :max_len], rows[:, max_len].copy(), rows[:, max_len + 1].copy().view(np.float32), want_tokens)

    def check_nbest(self, nbest):
        """``nbest`` as an int in 1 .. beam_size (None stays None: one result, today's path), refused by name otherwise"""
        if nbest is None:
            return None
        if isinstance(nbest, bool) or not isinstance(nbest, (int, np.integer)) or not 1 <= int(nbest) <= self.beam_size:
            raise ValueError(f'nbest={nbest!r}: nbest must be an integer in 1 .. beam_size = {self.beam_size}')
        return int(nbest)

    def _unpacked_nbest(self, flat, B, N, max_len, want_tokens):
        """packed host int32 [B * N * (max_len + 2) + B] = per utterance N rows of tokens | length | score bits, best first, then
        the B row counts -> per utterance the list of its count results, each as ``_results`` gives them"""
        flat = np.asarray(flat)
        rows = flat[:B * N * (max_len + 2)].reshape(B, N, max_len + 2)
        count = flat[B * N * (max_len + 2):B * N * (max_len + 2) + B]
        return [self._unpacked(rows[b, :int(count[b])], max_len, want_tokens) for b in range(B)]

    def _nbest_gpu(self, eng, B, max_len, N):
        """masr_beam_nbest_gpu behind the ``_search_gpu`` launch on the current stream -> (packed int32 [B * N * (max_len + 2) + B]
        on the device, what must stay alive until it is read)"""
        toks = torch.zeros(B, N, max_len, dtype=torch.int32, device=eng.device)
        lens = torch.zeros(B, N, dtype=torch.int32, device=eng.device)
        scores = torch.zeros(B, N, dtype=torch.float32, device=eng.device)
        count = torch.zeros(B, dtype=torch.int32, device=eng.device)
        check(self._lib.masr_beam_nbest_gpu(eng.h, B, self.beam_size, N, *self._lm_args(), C.c_void_p(toks.data_ptr()), max_len,
                                            C.c_void_p(lens.data_ptr()), C.c_void_p(scores.data_ptr()),
                                            C.c_void_p(count.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        rows = torch.cat([toks, lens[:, :, None], scores.view(torch.int32)[:, :, None]], 2)
        return torch.cat([rows.view(-1), count]), (toks, lens, scores, count)

    def _search_gpu(self, eng, cand, frames, B, Ts, pack=True):
        """masr_beam_search_gpu_lm over the candidates ``cand`` = (idx, logp, cnt, blp, K) of ``_candidates`` on the current stream
        -> (packed rows [B, max_len + 2] on the device, max_len, what must stay alive until they are read)"""
        idx, logp, cnt, blp, K = cand
        max_len = max(Ts, 1)
        fr = eng.to_device(frames)
        toks = torch.zeros(B, max_len, dtype=torch.int32, device=eng.device)
        lens = torch.zeros(B, dtype=torch.int32, device=eng.device)
        scores = torch.zeros(B, dtype=torch.float32, device=eng.device)
        check(self._lib.masr_beam_search_gpu_lm(eng.h, C.c_void_p(idx.data_ptr()), C.c_void_p(logp.data_ptr()),
                                                C.c_void_p(cnt.data_ptr()), C.c_void_p(fr.data_ptr()), B, Ts, K,
                                                self.beam_size, self.blank_id, *self._lm_args(), self._ptr(blp),
                                                C.c_void_p(toks.data_ptr()), max_len,
                                                C.c_void_p(lens.data_ptr()), C.c_void_p(scores.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        # one contiguous copy back (not packed for a caller that reads the n-best rows instead: entry 0 of them is this result)
        packed = torch.cat([toks, lens[:, None], scores.view(torch.int32)[:, None]], 1) if pack else None
        return packed, max_len, (idx, logp, cnt, blp, fr, toks, lens, scores)

    def _search_host(self, idx, logp, cnt, blp, frames, B, Ts, K, want_tokens):
        """masr_beam_search_batch_lm on ``num_processes`` host threads over host candidates -> results"""
        max_len = max(Ts, 1)
        toks = np.zeros((B, max_len), np.int32)
        lens = np.zeros(B, np.int32)
        scores = np.zeros(B, np.float32)
        fr = np.ascontiguousarray(frames, np.int32)
        rc = self._lib.masr_beam_search_batch_lm(idx.ctypes.data_as(C.c_void_p), logp.ctypes.data_as(C.c_void_p),
                                                 cnt.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p), B, Ts, K,
                                                 self.beam_size, self.blank_id, self.num_processes, *self._lm_args(),
                                                 self._ptr(blp), toks.ctypes.data_as(C.c_void_p), max_len,
                                                 lens.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise _lib.MasrError('masr_beam_search_batch failed')
        return self._results(toks, lens, scores, want_tokens)

    def _search_host_nbest(self, idx, logp, cnt, frames, B, Ts, K, N, want_tokens):
        """masr_beam_search_batch_nbest (LM-free) on ``num_processes`` host threads -> per utterance its n-best results"""
        if self._ext_scorer is not None:
            kind = 'character-based' if self._ext_scorer.is_character_based else 'word-based'
            raise ValueError(f'nbest is not available from the host-thread search with a language model bound (here a {kind} '
                             'scorer; word-based scorers and sizes beyond the GPU search run there): its n-best search '
                             '(masr_beam_search_batch_nbest) is LM-free')
        max_len = max(Ts, 1)
        toks = np.zeros((B, N, max_len), np.int32)
        lens = np.zeros((B, N), np.int32)
        scores = np.zeros((B, N), np.float32)
        count = np.zeros(B, np.int32)
        fr = np.ascontiguousarray(frames, np.int32)
        rc = self._lib.masr_beam_search_batch_nbest(idx.ctypes.data_as(C.c_void_p), logp.ctypes.data_as(C.c_void_p),
                                                    cnt.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p), B, Ts, K,
                                                    self.beam_size, self.blank_id, self.num_processes, N,
                                                    toks.ctypes.data_as(C.c_void_p), max_len, lens.ctypes.data_as(C.c_void_p),
                                                    scores.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise _lib.MasrError('masr_beam_search_batch_nbest failed')
        return [self._results(toks[b, :count[b]], lens[b, :count[b]], scores[b, :count[b]], want_tokens) for b in range(B)]

    def _say_host_search(self, beyond_gpu=False):
        """once per decoder: why the prefix search runs on host threads"""
        if getattr(self, '_said_host', False):
            return
        if self._ext_scorer is not None and not self._ext_scorer.is_character_based:
            self._said_host = True
            logger.info('masr_amd BeamSearchDecoder: word-based language model -> prefix search on host threads')
        elif beyond_gpu:
            self._said_host = True
            logger.warning(f'masr_amd BeamSearchDecoder: beam_size={self.beam_size} x cutoff_top_n={self.cutoff_top_n} is beyond the '
                           f'GPU search (LDS), using {self.num_processes} host threads')

    def _batch_collect(self, pending, want_tokens=False):
        """results of a ``_batch(..., defer=True)`` launch.  The host waits for the EVENT behind this pass's search, then copies
        the packed rows (tokens | length | score bits, int32) back on the library's copy stream and waits for that copy only.
        Round 6 measured the three simpler ways and why they stall: through the current (main) stream the first of three passes
        came back at 35 instead of 15 ms (the encoders of the later passes are queued there); an asynchronous copy enqueued right
        behind the search kernel is a DMA-engine command that waits 6 ms and holds up the next pass's upload on the same engine
        (the host sat 17 ms in the next pass's preparation); a copy enqueued on the search's stream at collection time queues
        behind the search of pass k + 2, which shares that stream."""
        _, B, max_len, packed, _keep, done = pending[:6]
        N = pending[6] if len(pending) > 6 else None      # an n-best launch: [B, N, max_len + 2] rows + [B] counts, the same one copy
        n = B * (max_len + 2) if N is None else packed.numel()
        host = self._pinned_out(n)
        done.synchronize()                           # the search (and the packing behind it) of THIS pass
        with torch.cuda.stream(runtime.aux_engine(packed.device).side_stream(3)):          # the library's copy stream: idle
            host[:n].copy_(packed.view(-1), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        ev.synchronize()
        if N is None:
            res = self._unpacked(host[:n].view(B, max_len + 2).numpy(), max_len, want_tokens)
        else:
            res = self._unpacked_nbest(host[:n].numpy(), B, N, max_len, want_tokens)
        self._pin_free.append(host)
        return res

    def _batch(self, probs_list, defer=False, want_tokens=False, frames=None, nbest=None):
        """``defer=True`` (device-resident probabilities, GPU search): launch pruning + search on the current torch stream and
        return a handle for ``_batch_collect`` without synchronising -- lets the caller run the search of one sub-batch on a
        side stream while the encoder works on the next one (the search occupies one workgroup per utterance).
        ``frames`` given: ``probs_list`` is ONE padded [B, Ts, V] array / device tensor (what the CTC head of a device pass
        leaves behind) with ``frames[i]`` valid rows per utterance -- searched in place, no restacking (round 6: the 32 slice
        copies + the fill of a 134 MB buffer were 3 ms on the critical path of every BASELINE configs[2] pass).
        ``nbest=N``: every utterance's result is the LIST of its (at most N) best prefixes, best first, entry 0 being what the
        call returns without it -- on the GPU a second small kernel over what the search left (masr_beam_nbest_gpu), whose rows
        come back in the same single packed copy; None: one result, nothing else launched."""
        nbest = self.check_nbest(nbest)
        if frames is not None:
            stacked = probs_list
            B, Ts, V = stacked.shape
            frames = np.asarray(frames, np.int32)
            assert frames.shape == (B,) and (B == 0 or int(frames.max()) <= Ts)
        else:
            B = len(probs_list)
            frames = np.array([p.shape[0] for p in probs_list], np.int32)
            Ts = int(frames.max()) if B else 0
            V = probs_list[0].shape[1]
            if torch.is_tensor(probs_list[0]):          # device-resident probabilities: no host round trip
                stacked = torch.zeros(B, Ts, V, dtype=torch.float32, device=probs_list[0].device)
            else:
                stacked = np.zeros((B, Ts, V), np.float32)
            for i, p in enumerate(probs_list):
                stacked[i, :p.shape[0]] = p
        if B and Ts and self.use_gpu_search and self.gpu_search_supported(Ts, V):
            # whole search on the device: candidates never leave HBM, one workgroup per utterance
            eng = runtime.aux_engine(stacked.device if torch.is_tensor(stacked) else None)
            packed, max_len, keep = self._search_gpu(eng, self._candidates(stacked.reshape(B * Ts, V), to_host=False), frames, B, Ts,
                                                     pack=nbest is None)
            if nbest is not None:          # the n-best rows take the single result's place in the packed copy (entry 0 is that result)
                packed, keep_n = self._nbest_gpu(eng, B, max_len, nbest)
                keep = keep + keep_n
            if defer:                      # nothing has been synchronised: _batch_collect() fetches the result later
                done = torch.cuda.Event()
                done.record()
                pending = ('gpu', B, max_len, packed, (stacked, probs_list) + keep, done)
                return pending if nbest is None else pending + (nbest,)
            if nbest is not None:
                return self._unpacked_nbest(packed.cpu().numpy(), B, nbest, max_len, want_tokens)
            return self._unpacked(packed.cpu().numpy(), max_len, want_tokens)
        if defer:
            raise Exception('deferred batch search needs the GPU search (device-resident probabilities within its limits)')
        if nbest is not None and not (B and Ts):
            return [[r] for r in self._batch(probs_list, want_tokens=want_tokens, frames=frames)]
        self._say_host_search(beyond_gpu=bool(self.use_gpu_search and B and Ts))
        idx, logp, cnt, blp, K = self._candidates(stacked.reshape(B * Ts, V))
        if nbest is not None:
            return self._search_host_nbest(idx, logp, cnt, frames, B, Ts, K, nbest, want_tokens)
        return self._search_host(idx, logp, cnt, blp, frames, B, Ts, K, want_tokens)

    # ---- host-thread search of a device pass, deferred ---------------------------------------------------------------------------
    def prune_padded(self, probs, frames):
        """vocabulary pruning of ONE device pass (padded probabilities [B, Ts, V] on the device, ``frames[i]`` valid rows) on the
        current stream; the probabilities are not needed afterwards.  -> a part for ``search_host_deferred``."""
        B, Ts, V = probs.shape
        idx, logp, cnt, blp, K = self._candidates(probs.reshape(B * Ts, V), to_host=False)
        return {'idx': idx.view(B, Ts, K), 'logp': logp.view(B, Ts, K), 'cnt': cnt.view(B, Ts), 'blp': None if blp is None else blp.view(B, Ts),
                'frames': np.asarray(frames, np.int32), 'B': B, 'Ts': Ts, 'K': K}

    def search_host_deferred(self, probs, frames, want_tokens=False):
        """The host-thread prefix search (word-based scorers, sizes beyond the GPU kernel) of ONE device pass without stalling the
        device: the vocabulary pruning is queued on the current stream right behind the pass's CTC head, and a function is
        returned that -- when called -- waits for the pruning, brings the candidates to the host on the library's copy stream
        (5 MB for 32 x 494 frames x 40; NOT queued behind the encoder, see ``_batch_collect``) and runs the search on
        ``num_processes`` host threads.  The caller launches the encoders of the next passes first and collects afterwards: host
        searches run under device passes instead of between them."""
        part = self.prune_padded(probs, frames)
        done = torch.cuda.Event()
        done.record()
        self._say_host_search()

        def collect():
            dev = [part['idx'].view(-1), part['logp'].view(-1).view(torch.int32), part['cnt'].view(-1)]
            if part['blp'] is not None:
                dev.append(part['blp'].view(-1).view(torch.int32))
            host = self._pinned_out(sum(t.numel() for t in dev))
            done.synchronize()
            with torch.cuda.stream(runtime.aux_engine(part['idx'].device).side_stream(3)):
                at, views = 0, []
                for t in dev:
                    host[at:at + t.numel()].copy_(t, non_blocking=True)
                    views.append(host[at:at + t.numel()].numpy())
                    at += t.numel()
                ev = torch.cuda.Event()
                ev.record()
            ev.synchronize()
            blp = views[3].view(np.float32) if part['blp'] is not None else None
            try:
                return self._search_host(views[0], views[1].view(np.float32), views[2], blp, part['frames'], part['B'], part['Ts'],
                                         part['K'], want_tokens)
            finally:
                self._pin_free.append(host)
        return collect

    def decode_chunk(self, probs, logits_lens, nbest=None):
        """streaming: feed a chunk probs [1, T, V]; returns (score, text) of the best prefix so far
        (beam_search_decoder.py:75-91).  ``nbest=N`` (the device-resident search only): ``last_nbest`` / ``last_nbest_tokens``
        then hold the (at most N) best prefixes so far as [(score, text)] / [token ids], best first, entry 0 being the returned
        result (masr_gbeam_nbest behind the chunk's advance); None launches nothing else."""
        nbest = self.check_nbest(nbest)
        n_valid = int(np.asarray(logits_lens).reshape(-1)[0])
        p = probs[0][:n_valid] if torch.is_tensor(probs) else np.asarray(probs)[0][:n_valid]     # device tensors stay there
        if self.use_gpu_search and self.gpu_search_supported(1, p.shape[1]):
            return self._decode_chunk_gpu(p, nbest)
        if nbest is not None:
            raise ValueError('nbest of a streaming search comes from the device-resident search (masr_gbeam_nbest); this decoder '
                             'streams on the host (word-based scorer, use_gpu_search off or sizes beyond the GPU search)')
        idx, logp, cnt, blp, K = self._candidates(p)
        if p.shape[0]:
            self._lib.masr_beam_advance_lm(self._stream, idx.ctypes.data_as(C.c_void_p), logp.ctypes.data_as(C.c_void_p),
                                           cnt.ctypes.data_as(C.c_void_p), self._ptr(blp), p.shape[0], K)
        toks = np.zeros(4096, np.int32)
        n, sc = C.c_int32(), C.c_float()
        self._lib.masr_beam_result(self._stream, toks.ctypes.data_as(C.c_void_p), 4096, C.byref(n), C.byref(sc))
        self.last_tokens = toks[:n.value].tolist()
        return float(sc.value), self._text(toks[:n.value])

    def _decode_chunk_gpu(self, p, nbest=None):
        """device-resident search state (masr_gbeam_*): only the best prefix (with ``nbest``: the N best) travels back per chunk"""
        eng = self._geng if self._gstream is not None else runtime.aux_engine()
        if self._gstream is None:
            self._geng = eng             # the stream's state lives in THIS device's engine until close()
            h = C.c_int32()
            check(self._lib.masr_gbeam_open(eng.h, self.beam_size, self.blank_id, 5000, C.byref(h)))
            self._gstream = h.value
            if self._ext_scorer is not None:
                check(self._lib.masr_gbeam_set_lm(eng.h, self._gstream, *self._lm_args()))
        T = p.shape[0]
        idx, logp, cnt, blp, K = self._candidates(p, to_host=False)
        max_len = 5000
        if self._gout is None:
            self._gout = (torch.zeros(1, max_len, dtype=torch.int32, device=eng.device),
                          torch.zeros(1, dtype=torch.int32, device=eng.device),
                          torch.zeros(1, dtype=torch.float32, device=eng.device))
        toks, lens, scores = self._gout
        check(self._lib.masr_gbeam_advance_lm(eng.h, self._gstream, C.c_void_p(idx.data_ptr()), C.c_void_p(logp.data_ptr()),
                                              C.c_void_p(cnt.data_ptr()), self._ptr(blp), T, K, C.c_void_p(toks.data_ptr()),
                                              max_len, C.c_void_p(lens.data_ptr()), C.c_void_p(scores.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        if nbest is not None:
            return self._read_nbest(eng, nbest)
        n = int(lens.item())
        self.last_tokens = toks[0, :n].cpu().numpy().tolist()
        return float(scores.item()), self._text(self.last_tokens)

    def live_nbest(self, nbest):
        """the (at most ``nbest``) best prefixes of the device-resident streaming search as it stands, nothing advanced
        (masr_gbeam_nbest alone) -> (score, text) of the best; ``last_nbest`` / ``last_nbest_tokens`` / ``last_tokens`` as after
        ``decode_chunk(nbest=)``.  For a session whose last feed decoded no window; the search must have seen a chunk."""
        nbest = self.check_nbest(nbest)
        if self._gstream is None:
            raise _lib.MasrError('live_nbest: this decoder has no device-resident search yet (no chunk was decoded)')
        return self._read_nbest(self._geng, nbest)

    def _read_nbest(self, eng, nbest):
        """masr_gbeam_nbest on the current stream and its one packed copy back"""
        # the chunk's one result is entry 0 of the rows: ONE packed copy brings everything back.  Prefixes of a stream are far
        # shorter than the 5000 frames its pool allows: the rows hold 512 tokens and a longer prefix is an error by name
        nl = 512
        ntoks = torch.zeros(1, nbest, nl, dtype=torch.int32, device=eng.device)
        nlens = torch.zeros(1, nbest, dtype=torch.int32, device=eng.device)
        nscores = torch.zeros(1, nbest, dtype=torch.float32, device=eng.device)
        count = torch.zeros(1, dtype=torch.int32, device=eng.device)
        check(self._lib.masr_gbeam_nbest(eng.h, self._gstream, nbest, C.c_void_p(ntoks.data_ptr()), nl,
                                         C.c_void_p(nlens.data_ptr()), C.c_void_p(nscores.data_ptr()),
                                         C.c_void_p(count.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        rows = torch.cat([ntoks, nlens[:, :, None], nscores.view(torch.int32)[:, :, None]], 2)
        flat = torch.cat([rows.view(-1), count]).cpu().numpy()
        if int(flat[:nbest * (nl + 2)].reshape(nbest, nl + 2)[:, nl].max()) > nl:
            raise _lib.MasrError(f'decode_chunk(nbest={nbest}): a prefix of more than {nl} tokens does not fit the n-best rows')
        ids = self._unpacked_nbest(flat, 1, nbest, nl, True)[0]
        self.last_nbest_tokens = [t for t, _ in ids]
        self.last_nbest = [(sc, self._text(t)) for t, sc in ids]
        self.last_tokens = list(ids[0][0])
        return self.last_nbest[0]

    def reset_decoder(self):
        """beam_search_decoder.py:93-96."""
        self._lib.masr_beam_reset(self._stream)
        if self._gstream is not None:
            check(self._lib.masr_gbeam_reset(self._geng.h, self._gstream))
