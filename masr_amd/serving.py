"""Multi-stream session manager: any number of concurrent ``predict_stream`` sessions on ONE engine (SURVEY.md 8(f) rank 1,
BASELINE configs[4]); ``MASRPredictor.predict_stream`` itself is a pool with one session.

The reference server holds one MASRPredictor -- i.e. one stream -- per websocket and decodes them one after the other
(infer_server.py:42-46,103-156).  Here every session keeps the state the reference keeps per stream (samples not yet framed,
feature frames not yet consumed, decoder history; predict.py:237-343) but the device work of all sessions that have audio
pending is done together.  Three classes:

``StreamPool`` -- the public name and the base: the configuration read, the refusals, ``errors`` / ``device_resampled`` /
``last_tokens``, and the front of ``feed`` (``route_feed`` + the host decode).  ``StreamPool(predictor, ...)`` returns one of the
two classes below, chosen once, there; ``pool.framing`` says which.

``CStepPool`` (``framing == 'c'``; ``ctc_greedy`` without timestamps) -- the whole step is ONE C-ABI call (``masr_pool_step``,
csrc/pool.hip); the class keeps the handles, hands over the fed buffers and builds the text.

``LockStepPool`` (``framing == 'python'``; ``ctc_beam_search``, ``timestamps=True`` and MASR_POOL_PY=1 (A/B), and what the C step
is tested against):

  * ONE ragged feature launch for the new samples of all sessions (dB normalisation gains evaluated like the reference); the
    feature frames never leave the device: they are appended to a device-resident pool [session, frame, F] and the 67-frame
    decoding windows are gathered from it;
  * the windows advance in lock-step through ``masr_encode_chunk`` (n streams per call);
  * ``decoder: ctc_greedy`` -- only the per-frame (argmax, max prob) pairs leave the CTC head (never the [n, 16, V]
    probabilities); they are appended to a device-resident history [session, frame] and ONE ``masr_ctc_collapse`` launch per
    step turns the histories of all sessions that advanced into tokens + scores (the reference re-decodes its python lists
    per session, ctc_greedy_decoder.py:52-89);
  * ``decoder: ctc_beam_search`` -- the probabilities stay on the device and feed each session's own device-resident prefix
    beam search (``BeamSearchDecoder.decode_chunk``, beam_search_decoder.py:75-91).

Every session receives exactly the partial results its own reference ``predict_stream`` loop would produce.

``StreamPool(predictor, timestamps=True)`` -- token timestamps on streams: the pool keeps what the CTC head emitted for every
session on the device, one V-wide row per encoder frame in ONE row pool [n_rows, V] that all sessions share (posterior_rows.py
says which rows are whose: freed rows are reused, so a session's rows are neither contiguous nor increasing), and every step
aligns the current hypothesis of each session that advanced against ALL of its frames so far with one masr_ctc_align_rows launch
behind the decoding (csrc/ctc_align.hip reads the frames through the row table: a step packs and copies no history; only the
step in which the pool outgrows its allocation re-houses it, into twice the rows, every row keeping its number).  The result
gains ``'tokens'`` as offline (decoders/ctc_alignment.py), in seconds on the session's own clock.  Such a pool is a
``LockStepPool`` for ``ctc_greedy`` too; it costs V * 4 bytes of device memory per encoder frame and session (V = 4233: 17 KB per
frame, about 4 MB per 10 s of speech), bounded by the stream's own frame limit and given back on ``reset`` / ``close``.

``decoder: attention_rescoring`` with ``attention_rescoring_decoder_conf.on_streams: 'rescore_at_end'`` (without the key the
decoder is refused on streams, as it always was) -- a ``LockStepPool`` whose sessions search like ``ctc_beam_search`` sessions
without a language model (each its own fork of the rescoring block's search; the partial results are that first pass's best
prefix and score) while every lock-step call goes through ``masr_encode_chunk_enc`` and its encoder rows are appended to a second
row pool [n_rows, d_model] (a second ``RowAllocator``, the same slab growth, one indexed copy of the size of the call:
d_model * 4 bytes per encoder frame and session, 1 KB at 256).  In the step whose feed carried ``is_end=True`` the n-best of the
session's live search is read behind its last window and ONE masr_rescore_rows launch scores the hypotheses of all sessions
that end in that step against all of their kept frames through the row tables (one staged copy up, one back; more than
65535 // beam_size sessions ending together are split into that many per launch, the call's own limit); the result is the
winner with the combined score.  ``last_rescoring`` / ``encoder_rows`` show what happened; ``timestamps=True`` composes (the
winner is what is aligned); ``reset`` / ``close`` give the rows back.
"""
import ctypes as C
import os
import weakref

import numpy as np
import torch

from masr_amd import _lib
from masr_amd._lib import MasrError
from masr_amd.data_utils.audio import AudioSegment
from masr_amd.decoders import ctc_alignment
from masr_amd.engine import reference_gains

_PCM_SCALE = np.float32(1.0 / 32768.0)

# chunked decoding geometry of the reference facade (predict.py:283-290): 16 encoder frames per chunk, subsampling 4, context 7
DECODING_CHUNK, SUBSAMPLING, CONTEXT = 16, 4, 7
WINDOW = (DECODING_CHUNK - 1) * SUBSAMPLING + CONTEXT      # 67 feature frames per window
STRIDE = SUBSAMPLING * DECODING_CHUNK                      # 64
OVERLAP = CONTEXT - SUBSAMPLING                            # 3 frames carried over


def window_plan(n_frames, is_end):
    """the decoding windows of ``n_frames`` pending feature frames (predict.py:283-306) -> [(first, last)]: full windows only
    until the stream ends; at its end a short last window too, while it has the context's frames"""
    if (n_frames < WINDOW and not is_end) or n_frames < CONTEXT:
        return []
    left = CONTEXT if is_end else WINDOW
    return [(cur, min(cur + WINDOW, n_frames)) for cur in range(0, n_frames - left + 1, STRIDE)]


def device_resample_enabled():
    """MASR_DEVICE_RESAMPLE=0 (A/B): off-rate audio is resampled on the host, chunk by chunk, as before"""
    return os.environ.get('MASR_DEVICE_RESAMPLE', '1') != '0'


def route_feed(audio_data, channels, samp_width, sample_rate, target_rate, c_framing, device_resample):
    """where one ``StreamPool.feed`` goes -> ``('wire', int16 array)``: mono 16-bit PCM bytes at the model's rate, kept as they
    are; ``('raw', samples, format, n_out)``: OFF-RATE audio the C framing hands to the device resampler as fed -- mono 16-bit
    PCM bytes or an int16 vector (format 0), any other int / float array as the float32 mono samples ``AudioSegment`` makes of
    it (format 1) -- with ``n_out = resampled_length(n, sample_rate, target_rate)`` samples at the model's rate (raises the host
    resampler's ValueError for a chunk too short to give one); ``('host',)``: everything else -- multi-channel or non-16-bit
    bytes, audio at the model's rate that is not wire PCM, the python framing (beam search, MASR_POOL_PY=1) and
    MASR_DEVICE_RESAMPLE=0 -- through ``AudioSegment`` on the host, as before."""
    from masr_amd.data_utils.resample import resampled_length
    is_bytes = isinstance(audio_data, (bytes, bytearray, memoryview))
    pcm = is_bytes and samp_width == 2 and channels == 1
    if pcm and sample_rate == target_rate:
        return ('wire', np.frombuffer(bytes(audio_data) if isinstance(audio_data, bytearray) else audio_data, '<i2'))
    if not (c_framing and device_resample) or sample_rate == target_rate:
        return ('host',)
    if pcm:
        x, fmt = np.frombuffer(bytes(audio_data) if isinstance(audio_data, bytearray) else audio_data, '<i2'), 0
    elif isinstance(audio_data, np.ndarray):
        if audio_data.dtype == np.int16 and audio_data.ndim == 1:
            x, fmt = np.ascontiguousarray(audio_data), 0
        else:
            x, fmt = np.ascontiguousarray(AudioSegment._to_float(audio_data), np.float32), 1
        if x.ndim != 1:
            return ('host',)
    else:
        return ('host',)
    return ('raw', x, fmt, resampled_length(x.shape[0], sample_rate, target_rate))


def token_text(vocab, tokens):
    """token ids -> the transcript"""
    return ''.join([vocab[t] for t in tokens]).replace('<space>', ' ')


def greedy_result(vocab, tokens, score):
    """the partial result of a greedy session from its collapsed best path (token ids, float32 score); the score counts every
    non-blank frame (repeats included); with none the reference returns 0"""
    return {'text': token_text(vocab, tokens), 'score': float(score) * 100.0 if tokens else 0}


class StreamPool:
    """``pool = StreamPool(predictor)`` on a streaming MASRPredictor (conformer / squeezeformer / efficient_conformer /
    uni-directional deepspeech2; ``ctc_greedy`` or ``ctc_beam_search``).  ``open()`` -> handle; ``feed(handle, pcm_bytes,
    is_end)`` queues audio; ``step()`` processes everything queued since the last step and returns ``{handle: {'text',
    'score'} or None}`` for the sessions that were fed; ``close(handle)`` releases the stream.  The call returns a ``CStepPool``
    for greedy sessions and a ``LockStepPool`` for beam search, ``timestamps=True`` and MASR_POOL_PY=1 (``framing``: 'c' /
    'python'); this class is what the two share.

    ``timestamps=True``: every result gains ``'tokens'`` -- [{'token', 'start', 'end', 'score'}] as ``predict(timestamps=True)``
    gives offline, [] for an empty transcript, None when the CTC trellis holds no path for the hypothesis (or it is longer than
    MASR_ALIGN_MAX_TOKENS) -- in seconds since ``open()`` / ``reset()``; ``end`` never exceeds the audio fed so far.  The pool
    then keeps the CTC posteriors of every open session on the device, V * 4 bytes per encoder frame (V = 4233: 17 KB per frame,
    about 4 MB per 10 s of speech and session) until ``reset`` / ``close`` gives the rows back, bounded by the stream's frame
    limit (``max_frames_out`` / the positional table); each step re-aligns the whole history of the sessions that advanced in one
    launch, and ``ctc_greedy`` sessions run the python framing instead of the C step.  ``posterior_rows`` / ``posteriors`` show
    what is kept.  Without the flag nothing of this exists and the pool is what it was."""

    def __new__(cls, predictor, max_frames_out=0, timestamps=False, nbest=None):
        if cls is StreamPool:                                  # the one place the framing is chosen
            lock_step = (predictor.configs.decoder in ('ctc_beam_search', 'attention_rescoring') or timestamps
                         or os.environ.get('MASR_POOL_PY'))
            cls = LockStepPool if lock_step else CStepPool
        return super().__new__(cls)

    def __init__(self, predictor, max_frames_out=0, timestamps=False, nbest=None):
        cfg = predictor.configs
        if not cfg.streaming or not ('former' in cfg.use_model or cfg.use_model == 'deepspeech2'):
            raise Exception(f"不支持改该模型流式识别，当前模型：{cfg.use_model}，参数streaming为：{cfg.streaming}")
        if cfg.decoder == 'attention_rescoring':
            # opt-in (attention_rescoring_decoder_conf.on_streams: 'rescore_at_end'); without the key, or without the block, the
            # refusal streams always got -- before anything of a pool exists
            from masr_amd.decoders.attention_rescoring import STREAM_REFUSAL, on_streams
            if on_streams(cfg) != 'rescore_at_end':
                raise Exception(STREAM_REFUSAL)
            dec = predictor.rescoring_decoder
            if not dec._pruner.gpu_search_supported(1, len(predictor._text_featurizer.vocab_list)):
                raise MasrError(f"attention_rescoring_decoder_conf.on_streams='rescore_at_end' with beam_size={dec.beam_size}, "
                                f"cutoff_top_n={dec._pruner.cutoff_top_n}: a stream's first pass is the device-resident prefix search "
                                f"(beam_size 2 .. 512, cutoff_top_n <= 64, its tables within 160 KB of LDS), whose n-best is what "
                                f"is rescored")
        if cfg.decoder == 'attention':
            from masr_amd.decoders.attention_decoder import STREAM_REFUSAL
            raise Exception(STREAM_REFUSAL)
        if cfg.decoder == 'joint':
            from masr_amd.decoders.joint_decoder import STREAM_REFUSAL
            raise Exception(STREAM_REFUSAL)
        if cfg.decoder not in ('ctc_greedy', 'ctc_beam_search', 'attention_rescoring'):
            raise Exception(f'unknown decoder {cfg.decoder}')
        # nbest=N (ctc_beam_search sessions): every result gains 'nbest': [{'text', 'score'}], read from the session's
        # device-resident search behind each decoded chunk (masr_gbeam_nbest); the predictor refuses what has no such n-best
        self.nbest = predictor._nbest(nbest)
        self.predictor = predictor
        self.engine = predictor.predictor.engine
        self.vocab = predictor._text_featurizer.vocab_list
        pc = cfg.preprocess_conf
        self.method = pc.get('feature_method', 'fbank')
        self.n_mfcc = int(pc.get('n_mfcc', 40))
        self.sample_rate = int(pc.get('sample_rate', 16000))
        self.use_db, self.target_db = bool(pc.use_dB_normalization), pc.target_dB
        self.max_frames_out = max_frames_out
        self.timestamps = bool(timestamps)
        self.sessions = {}
        self.errors = {}              # handle -> message of a session the last step left out (full stream)
        self.device_resampled = 0     # off-rate feeds handed to the device resampler (masr_pool_step_rates) so far

    def shutdown(self):
        """release what the pool holds on its engine.  Idempotent; called by ``HipEngine.close()`` for every C-step pool still
        alive on it, so a pool never touches a destroyed engine."""
        self._closed = True
        self.sessions = {}

    def __del__(self):                                         # fallback only: owners call shutdown()
        try:
            self.shutdown()
        except Exception:                                      # noqa: BLE001  (interpreter shutdown)
            pass

    def _alive(self):
        if getattr(self, '_closed', False):
            raise MasrError('this StreamPool is shut down (its engine was closed): open a new pool on a live engine')

    def feed(self, handle, audio_data, is_end=False, channels=1, samp_width=2, sample_rate=16000):
        """queue raw PCM bytes (or a float / int numpy array) for a session (predict.py:260-272); processed by the next
        ``step()``.  Audio off the model's rate is queued as fed, with its rate: the step resamples it on the device
        (``route_feed``; MASR_DEVICE_RESAMPLE=0: on the host, here)."""
        self._alive()
        s = self.sessions[handle]
        route = route_feed(audio_data, channels, samp_width, sample_rate, self.sample_rate, self._C_FRAMING, device_resample_enabled())
        if route[0] == 'host':
            if isinstance(audio_data, np.ndarray):
                seg = AudioSegment.from_ndarray(audio_data, sample_rate)
            elif isinstance(audio_data, (bytes, bytearray, memoryview)):
                seg = AudioSegment.from_pcm_bytes(bytes(audio_data), channels=channels, samp_width=samp_width,
                                                  sample_rate=sample_rate)
            else:
                raise Exception(f'不支持该数据类型，当前数据类型为：{type(audio_data)}')
            if seg.sample_rate != self.sample_rate:
                seg.resample(self.sample_rate)
            route = ('host', seg.samples)
        self._queue(s, route, bool(is_end), sample_rate)

    def last_tokens(self, handle):
        """token ids behind the session's last partial result (what a multi-GPU front-end gathers instead of text)"""
        return self.sessions[handle].tokens

    def posterior_rows(self, handle):
        raise MasrError('this StreamPool keeps no posteriors: create it with timestamps=True')

    posteriors = posterior_rows

    def encoder_rows(self, handle):
        raise MasrError("this StreamPool keeps no encoder rows: decoder 'attention_rescoring' with "
                        "attention_rescoring_decoder_conf.on_streams 'rescore_at_end' does")

    last_rescoring = encoder_output = encoder_rows


class _CSession:
    __slots__ = ('sid', 'result', 'tokens')

    def __init__(self, sid):
        self.sid = sid
        self.result = None
        self.tokens = []              # token ids of the last partial result


class CStepPool(StreamPool):
    """greedy sessions: the whole step is ONE C-ABI call (masr_pool_step, csrc/pool.hip); this class keeps the handles, hands
    over the fed buffers and builds the text"""

    framing = property(lambda self: 'c')
    _C_FRAMING = True

    def __init__(self, predictor, max_frames_out=0, timestamps=False, nbest=None):
        super().__init__(predictor, max_frames_out, timestamps, nbest)
        self._feeds = []              # (handle, buffer, format, is_end, rate slot) since the last step
        self._packed = None           # the last step's rows as the C call left them: (device pointer, n, width, handles, host rows)
        self._rows = None             # ... and as ``last_packed`` hands them out, once asked for
        self._rate_slots = {}         # source rate -> slot of masr_pool_set_rate
        self._gain_error = None
        self._lib = _lib.lib()
        h = C.c_void_p()
        method = {'fbank': 0, 'mfcc': 1, 'linear': 2}[self.method]
        _lib.check(self._lib.masr_pool_create(self.engine.h, method, self.n_mfcc, 1 if self.use_db else 0, float(self.target_db),
                                              int(max_frames_out), C.byref(h)))
        self._c = h
        me = weakref.ref(self)                             # (no reference cycle through the callback: the pool dies with

        def gain_cb(ms_ptr, n, target_db, out_ptr, user):  #  its last reference, not at some later garbage collection)
            pool = me()
            return pool._gains(ms_ptr, n, target_db, out_ptr, user) if pool is not None else 1
        self._gain_cb = _lib.GAIN_FN(gain_cb)              # (kept alive with the pool)
        self.engine.__dict__.setdefault('_pools', weakref.WeakSet()).add(self)     # HipEngine.close() shuts its pools down first

    def shutdown(self):
        """destroy the C pool (closes its streams on the engine, synchronises the engine's device)"""
        c, self._c = getattr(self, '_c', None), None
        super().shutdown()
        if c and getattr(self.engine, 'h', None):
            with torch.cuda.device(self.engine.device):
                self._lib.masr_pool_destroy(c)
        self._feeds = []

    def _gains(self, ms_ptr, n, target_db, out_ptr, _user):
        """masr_gain_fn: the reference's scalar numpy expressions (audio.py:287-304,519-529) on the device's mean squares"""
        try:
            ms = np.ctypeslib.as_array(ms_ptr, (n,))
            np.ctypeslib.as_array(out_ptr, (n,))[:] = reference_gains(ms, self.target_db)
            return 0
        except Exception as exc:                               # noqa: BLE001  (re-raised by step() once the C call has returned)
            self._gain_error = exc
            return 1

    def open(self):
        self._alive()
        h = C.c_int32()
        _lib.check(self._lib.masr_pool_open(self._c, C.byref(h)))
        self.sessions[h.value] = _CSession(h.value)
        return h.value

    def close(self, handle):
        self._alive()
        _lib.check(self._lib.masr_pool_close(self._c, int(handle)))
        self.sessions.pop(handle)
        self._forget(handle)

    def reset(self, handle):
        """start a new utterance on an open session (MASRPredictor.reset_stream, predict.py:346-353)"""
        self._alive()
        _lib.check(self._lib.masr_pool_reset(self._c, int(handle)))
        self.sessions[handle] = _CSession(handle)
        self._forget(handle)

    def _forget(self, handle):
        self.errors.pop(handle, None)
        self._feeds = [f for f in self._feeds if f[0] != handle]

    def _rate_slot(self, sample_rate):
        """the pool's slot for a source rate: registered once (masr_pool_set_rate uploads the filter table)"""
        slot = self._rate_slots.get(sample_rate)
        if slot is None:
            from masr_amd.data_utils.resample import device_table
            pairs, num_table = device_table(sample_rate, self.sample_rate)
            out = C.c_int32()
            _lib.check(self._lib.masr_pool_set_rate(self._c, int(sample_rate), float(self.sample_rate) / sample_rate,
                                                    pairs.ctypes.data_as(C.c_void_p), pairs.shape[0], num_table, C.byref(out)))
            slot = self._rate_slots[sample_rate] = out.value
        return slot

    def _queue(self, s, route, is_end, sample_rate):
        if route[0] == 'wire':
            # (the buffer is handed to masr_pool_step as it is: the array keeps the caller's bytes alive until the step has run)
            self._feeds.append((s.sid, route[1], 0, is_end, -1))
        elif route[0] == 'raw':
            self._feeds.append((s.sid, route[1], route[2], is_end, self._rate_slot(sample_rate)))
        else:
            self._feeds.append((s.sid, np.ascontiguousarray(route[1], np.float32), 1, is_end, -1))

    @property
    def last_packed(self):
        """(device rows [n, tmax + 2] = tokens | count | score bits, tmax, handles) of the sessions that advanced in the last
        step -- what a multi-GPU front-end all-gathers (parallel.ShardedStreamPool) -- or None"""
        if self._rows is None and self._packed is not None:
            ptr, na, width, sids, host = self._packed
            try:            # zero-copy view of the pool's device rows (valid until the next step)
                view = type('_DevRows', (), {'__cuda_array_interface__': {'shape': (na, width), 'typestr': '<i4', 'data': (ptr, False),
                                                                         'version': 2, 'strides': None}})()
                rows = torch.as_tensor(view, device=self.engine.device)
            except Exception:                                  # noqa: BLE001
                rows = torch.from_numpy(host.copy()).to(self.engine.device)
            self._rows = (rows, width - 2, sids)
        return self._rows

    def step(self):
        """one masr_pool_step call over everything fed since the last step"""
        self._alive()
        feeds, self._feeds = self._feeds, []
        self._packed = self._rows = None
        if not feeds:
            return {}
        n = len(feeds)
        handles = np.fromiter((f[0] for f in feeds), np.int32, n)
        ptrs = np.fromiter((f[1].__array_interface__['data'][0] for f in feeds), np.uint64, n)
        counts = np.fromiter((f[1].shape[0] for f in feeds), np.int64, n)
        fmts = np.fromiter((f[2] for f in feeds), np.int32, n)
        ends = np.fromiter((f[3] for f in feeds), np.int32, n)
        ns, width = C.c_int32(), C.c_int32()
        h_out, st_out, rows_h, rows_d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._gain_error = None
        slots = np.fromiter((f[4] for f in feeds), np.int32, n)
        n_off = int((slots >= 0).sum())
        tail = (C.cast(self._gain_cb, C.c_void_p), None, C.byref(ns), C.byref(h_out), C.byref(st_out), C.byref(rows_h), C.byref(width),
                C.byref(rows_d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        head = (self._c, n, handles.ctypes.data, ptrs.ctypes.data, counts.ctypes.data, fmts.ctypes.data, ends.ctypes.data)
        if n_off:                                              # off-rate feeds: resampled on the device inside the step
            rc = self._lib.masr_pool_step_rates(*head, slots.ctypes.data, *tail)
        else:
            rc = self._lib.masr_pool_step(*head, *tail)
        if self._gain_error is not None:
            raise self._gain_error
        _lib.check(rc)
        self.device_resampled += n_off
        m, w = ns.value, width.value
        hs = np.ctypeslib.as_array(C.cast(h_out, C.POINTER(C.c_int32)), (m,))
        st = np.ctypeslib.as_array(C.cast(st_out, C.POINTER(C.c_int32)), (m,))
        na = int((st == 1).sum())
        rows = np.ctypeslib.as_array(C.cast(rows_h, C.POINTER(C.c_int32)), (na, w)) if na else None
        out, j, adv = {}, 0, []
        vocab = self.vocab
        for h, ok in zip(hs.tolist(), st.tolist()):
            s = self.sessions[h]
            if ok < 0:
                # left out of the step: its stream is full (max_frames_out / the positional table).  The reference asserts there
                # (embedding.py:48-50); here the OTHER sessions keep their results and this one carries the error until it is reset
                s.result = None
                out[h] = None
                self.errors[h] = 'stream exceeds max_frames_out / max_pos: reset_stream() or close it'
                continue
            if not ok:
                s.result = None
                out[h] = None
                continue
            r = rows[j]
            j += 1
            s.tokens = r[:int(r[w - 2])].tolist()
            s.result = out[h] = greedy_result(vocab, s.tokens, r[w - 1:w].view(np.float32)[0])
            adv.append(h)
        if na:
            self._packed = (rows_d.value, na, w, adv, rows)
        return out


class _HostStage:
    """Pinned host memory for the per-call uploads of a pool (pending samples, lengths, index arrays): a bump allocator whose
    copies to the device are asynchronous on the current stream, so the host never waits for the device between the launches
    of a step.  ``begin()`` opens a call: it waits for the previous call's copies (long done) before the area is reused."""

    def __init__(self, device, nbytes=1 << 20):
        self.device = device
        self._retired = []
        self._event = None
        self._alloc(nbytes)

    def _alloc(self, nbytes):
        self.buf = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.host = self.buf.numpy()
        self.used = 0

    def begin(self):
        if self._event is not None:
            self._event.synchronize()
            self._event = None
        elif self.used:                                      # a call that raised before end(): its copies may still be in flight
            torch.cuda.current_stream().synchronize()
        self._retired.clear()
        self.used = 0

    def take(self, shape, dtype):
        """-> (numpy view [shape] of dtype inside the pinned area, upload() -> device tensor of the same shape)"""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        at = (self.used + 63) & ~63
        if at + nbytes > self.host.size:                    # copies in flight keep the old area alive until the next begin()
            self._retired.append(self.buf)
            self._alloc(max(2 * self.host.size, 2 * nbytes))
            at = 0
        self.used = at + nbytes
        view = self.host[at:at + nbytes].view(dtype).reshape(shape)
        src = self.buf[at:at + nbytes].view({'float32': torch.float32, 'int32': torch.int32,
                                             'int64': torch.int64}[dtype.name]).view(*shape)
        return view, lambda: src.to(self.device, non_blocking=True)

    def fetch(self, dev):
        """device tensor (int32 / int64 / float32) -> numpy view of its copy in the pinned area; the copy is asynchronous on the
        current stream: the caller waits for that stream (or an event on it) before it reads the view"""
        view, _ = self.take(tuple(dev.shape), str(dev.dtype).replace('torch.', ''))
        at = self.used - view.nbytes
        self.buf[at:at + view.nbytes].view(dev.dtype).view(dev.shape).copy_(dev, non_blocking=True)
        return view

    def put(self, array, dtype=np.int64):
        view, upload = self.take(np.shape(array), dtype)
        view[...] = array
        return upload()

    def end(self):
        self._event = torch.cuda.Event()
        self._event.record()


class _Session:
    __slots__ = ('sid', 'remained', 'fresh', 'f0', 'nf', 'row', 'frames', 'result', 'decoder', 'tokens', 'beam_last', 'samples',
                 'rescored')

    def __init__(self, sid, row, decoder=None):
        self.sid = sid
        self.remained = None          # float32 samples not yet turned into frames (re-normalised on every call, like the reference)
        self.fresh = []               # audio fed since the last step: int16 PCM views (scaled when staged) / float32 arrays
        self.f0 = 0                   # feature frames not yet consumed by a window (the reference's cached_feat): frames
        self.nf = 0                   # f0 .. f0 + nf of this session's row of the device-resident feature pool
        self.row = row                # row of the pool's device-resident feature frames and (argmax, max prob) history
        self.frames = 0               # encoder frames decoded so far
        self.result = None
        self.decoder = decoder        # ctc_beam_search: this session's own search state
        self.tokens = []              # token ids of the last partial result
        self.beam_last = None         # beam search: the last decode_chunk result (what a step without a window returns)
        self.samples = 0              # samples fed so far at the model's rate (timestamps: the end of the session's clock)
        self.rescored = None          # rescore_at_end: the record of the session's last rescoring (``last_rescoring``)


class LockStepPool(StreamPool):
    """the python framing: ragged features into a device-resident frame pool, the windows of all sessions advanced in lock-step
    through ``masr_encode_chunk``, greedy histories collapsed in one launch or a prefix beam search per session; with
    ``timestamps=True`` the posterior rows and their alignment (the module docstring has the whole of it)"""

    framing = property(lambda self: 'python')
    _C_FRAMING = False
    ROW_SLAB = 4096                   # rows the posterior pool grows by (V = 4233: 69 MB)

    def __init__(self, predictor, max_frames_out=0, timestamps=False, nbest=None):
        super().__init__(predictor, max_frames_out, timestamps, nbest)
        self.min_samples = 320 if self.method == 'linear' else 400
        # rescore_at_end sessions search like beam sessions (their own LM-free search) and keep their encoder rows
        self.rescoring = predictor.configs.decoder == 'attention_rescoring'
        self.beam = predictor.configs.decoder == 'ctc_beam_search' or self.rescoring
        self._last_packed = None
        self._fed = {}                # handle -> is_end of the sessions fed since the last step
        self._free_rows = []
        self._hist_idx = torch.zeros(0, 0, dtype=torch.int32, device=self.engine.device)      # [rows, frames]
        self._hist_mp = torch.zeros(0, 0, dtype=torch.float32, device=self.engine.device)
        self.feat_dim = {'linear': 161, 'mfcc': self.n_mfcc}.get(self.method, 80)
        self._feat_cap = 512                                                                   # frames per session row
        self._feat = torch.zeros(0, self._feat_cap, self.feat_dim, dtype=torch.float32, device=self.engine.device)
        self._stage = _HostStage(self.engine.device)
        if self.timestamps:
            from masr_amd.posterior_rows import RowAllocator
            self._alloc = RowAllocator(self.ROW_SLAB)
            self._post = torch.empty(0, self.engine.vocab_size, dtype=torch.float32, device=self.engine.device)    # the row pool
            self._reduction = self.engine.frame_reduction()
        if self.rescoring:
            from masr_amd.posterior_rows import RowAllocator
            self._enc_alloc = RowAllocator(self.ROW_SLAB)      # (d_model = 256: 4 MB per slab)
            self._enc = torch.empty(0, self.engine.d_model, dtype=torch.float32, device=self.engine.device)       # the encoder row pool

    # ---- session life cycle ---------------------------------------------------------------------------------------------
    def _grow(self, rows, frames):
        """make the history tensors at least [rows, frames] (geometric growth, contents kept)"""
        r0, f0 = self._hist_idx.shape
        if rows <= r0 and frames <= f0:
            return
        r1 = r0 if rows <= r0 else max(rows, 2 * r0, 16)
        f1 = f0 if frames <= f0 else max(frames, 2 * f0, 256)
        for name, dt in (('_hist_idx', torch.int32), ('_hist_mp', torch.float32)):
            new = torch.zeros(r1, f1, dtype=dt, device=self.engine.device)
            new[:r0, :f0] = getattr(self, name)
            setattr(self, name, new)
        if max(r1, rows) > self._feat.shape[0]:
            new = torch.zeros(max(r1, rows), self._feat_cap, self.feat_dim, dtype=torch.float32, device=self.engine.device)
            new[:self._feat.shape[0]] = self._feat
            self._feat = new

    def _dev_index(self, idx):
        """host int64 index array -> device (staged through pinned memory, asynchronous)"""
        return self._stage.put(idx, np.int64)

    def _new_decoder(self):
        if self.rescoring:            # the first pass of the rescoring block: no language model, its beam_size and cutoffs
            return self.predictor.rescoring_decoder._pruner.fork()
        return self.predictor.beam_search_decoder.fork() if self.beam else None

    def open(self):
        self._alive()
        sid = self.engine.stream_open(self.max_frames_out)
        used = {s.row for s in self.sessions.values()}
        row = self._free_rows.pop() if self._free_rows else len(used)
        self._grow(row + 1, 256)
        self.sessions[sid] = _Session(sid, row, self._new_decoder())
        return sid

    def close(self, handle):
        self._alive()
        self.engine.stream_close(handle)
        s = self.sessions.pop(handle)
        if s.decoder is not None:
            s.decoder.close()
        self._free_rows.append(s.row)
        self._fed.pop(handle, None)
        if self.timestamps:
            self._alloc.release(handle)
        if self.rescoring:
            self._enc_alloc.release(handle)

    def reset(self, handle):
        """start a new utterance on an open session (MASRPredictor.reset_stream, predict.py:346-353)"""
        self._alive()
        self.engine.stream_reset(handle)
        old = self.sessions[handle]
        if old.decoder is not None:
            old.decoder.reset_decoder()
        self.sessions[handle] = _Session(handle, old.row, old.decoder)
        self._fed.pop(handle, None)
        if self.timestamps:
            self._alloc.release(handle)
        if self.rescoring:
            self._enc_alloc.release(handle)

    def _queue(self, s, route, is_end, sample_rate):
        # wire PCM, the common format, is kept as int16 (a view of the caller's bytes); x / 2^15 -- the float32 value
        # from_pcm_bytes produces -- happens when the step stages the samples for the device
        s.fresh.append(route[1])
        self._fed[s.sid] = is_end or self._fed.get(s.sid, False)

    # ---- timestamps: the posterior history and its alignment -----------------------------------------------------------------------
    def posterior_rows(self, handle):
        """timestamps pool: the rows of the pool's posterior matrix that hold the session's encoder frames, in frame order (int64)"""
        if not self.timestamps:
            return super().posterior_rows(handle)
        return np.asarray(self._alloc.rows_of(self.sessions[handle].sid), np.int64)

    def posteriors(self, handle):
        """timestamps pool: the CTC-head probabilities of all frames of the session so far, gathered -> [frames, V] device tensor"""
        rows = torch.from_numpy(self.posterior_rows(handle)).to(self.engine.device)
        return self._post[rows]

    def _keep_posteriors(self, items, probs):
        """append the rows ``probs`` [n, Tq, V] of one lock-step call to the sessions' histories: n * Tq rows of the pool, taken
        wherever it has room, filled with one copy of the size of this call (never of a history)"""
        self._post = self._append_rows(self._alloc, self._post, items, probs)

    def _append_rows(self, alloc, pool, items, block):
        """rows ``block`` [n, Tq, width] of one lock-step call into the row pool ``pool`` [n_rows, width] whose rows ``alloc`` hands
        out -> the pool (another tensor when it has grown)"""
        tq = block.shape[1]
        rows = np.concatenate([alloc.take(s.sid, tq) for s, _ in items])
        if alloc.capacity > pool.shape[0]:
            # more slabs: the rows keep their numbers.  (The matrix has to stay ONE allocation -- the kernel takes one base pointer --
            # so the step that outgrows it re-houses the pool, into at least twice the rows: the cost per row stays constant, and
            # no other step copies anything of the size of a history.)
            grown = torch.empty(max(alloc.capacity, 2 * pool.shape[0]), pool.shape[1], dtype=torch.float32, device=self.engine.device)
            grown[:pool.shape[0]] = pool
            pool = grown
        pool[self._dev_index(rows)] = block.reshape(-1, block.shape[2])
        return pool

    def _align(self, sess):
        """ONE masr_ctc_align_rows launch for the sessions ``sess`` (each with a result and at least one frame): their hypotheses,
        row tables and lengths go up in one staged copy, the packed alignment comes back in one, and that one is waited for ->
        the ``'tokens'`` value of each"""
        eng, st = self.engine, self._stage
        B = len(sess)
        tables = [self._alloc.rows_of(s.sid) for s in sess]
        tmax = max(len(t) for t in tables)
        flat, lmax, alignable = ctc_alignment.pack_hypotheses([s.tokens for s in sess], tmax)
        n32 = B + flat.size                                    # n_frames | tokens | n_tokens behind the int64 row table
        up, upload = st.take((B * tmax + (n32 + 1) // 2,), np.int64)
        table = up[:B * tmax].reshape(B, tmax)
        for b, t in enumerate(tables):
            table[b, :len(t)] = t
            table[b, len(t):] = -1
        small = up[B * tmax:].view(np.int32)
        small[:B] = [len(t) for t in tables]
        small[B:n32] = flat
        dev = upload()
        dsmall = dev[B * tmax:].view(torch.int32)
        packed = torch.empty(B * (3 * lmax + 2), dtype=torch.int32, device=eng.device)
        eng.ctc_align_rows(self._post, dev[:B * tmax].view(B, tmax), dsmall[:B], dsmall[B:B + B * lmax].view(B, lmax),
                           dsmall[B + B * lmax:n32], out=packed)
        host = st.fetch(packed)
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
        start, end, peak, score, status = ctc_alignment.unpack_alignment(host, B, lmax)
        return [ctc_alignment.utterance_tokens(s.tokens, start[b], end[b], peak[b], score[b], status[b] if alignable[b] else 1,
                                               self._reduction, self.sample_rate, s.samples / float(self.sample_rate), self.vocab)
                for b, s in enumerate(sess)]

    def _stamp(self, sess):
        """``'tokens'`` into the results of the sessions that decoded a window in this step"""
        todo = [s for s in sess if s.result is not None and s.frames > 0]
        for s, toks in zip(todo, self._align(todo) if todo else []):
            s.result['tokens'] = toks
        for s in sess:
            if s.result is not None and s.frames == 0:     # only windows too short for a frame so far: the empty transcript
                s.result['tokens'] = [] if not s.tokens else None

    # ---- rescore_at_end: the encoder rows and the second pass -----------------------------------------------------------------------
    def encoder_rows(self, handle):
        """rescore_at_end pool: the rows of the pool's encoder matrix that hold the session's encoder frames, in frame order (int64)"""
        if not self.rescoring:
            return super().encoder_rows(handle)
        return np.asarray(self._enc_alloc.rows_of(self.sessions[handle].sid), np.int64)

    def encoder_output(self, handle):
        """rescore_at_end pool: the encoder rows of all frames of the session so far, gathered -> [frames, d_model] device tensor"""
        rows = torch.from_numpy(self.encoder_rows(handle)).to(self.engine.device)
        return self._enc[rows]

    def last_rescoring(self, handle):
        """rescore_at_end pool: {'nbest': [token lists], 'ctc': [...], 'att': [...], 'r_att': [...], 'total': [...], 'winner': i} of
        the session's last rescoring (the first pass's prefixes best first, their CTC log-probabilities, both decoders' scores, the
        combined scores and the index of the result), or None before the first"""
        if not self.rescoring:
            return super().last_rescoring(handle)
        return self.sessions[handle].rescored

    def _rescore(self, sess):
        """ONE masr_rescore_rows launch for the sessions ``sess`` that end in this step (each with at least one encoder frame and
        the n-best of its search in its decoder): their row tables, frame counts and hypotheses go up in one staged copy, att /
        r_att come back in one, and that one is waited for -> their results become the winner and the combined score"""
        from masr_amd.decoders.attention_rescoring import build_table, combine, pick
        eng, st, dec = self.engine, self._stage, self.predictor.rescoring_decoder
        B = len(sess)
        nbest = [list(s.decoder.last_nbest_tokens) for s in sess]
        ctc = [np.array([sc for sc, _ in s.decoder.last_nbest], np.float32) for s in sess]
        hyps, lens, count = build_table(nbest, eng.max_pos)
        tables = [self._enc_alloc.rows_of(s.sid) for s in sess]
        tmax = max(len(t) for t in tables)
        n32 = B + hyps.size + lens.size                        # n_frames | hyps | hyp_lens behind the int64 row table
        up, upload = st.take((B * tmax + (n32 + 1) // 2,), np.int64)
        table = up[:B * tmax].reshape(B, tmax)
        for b, t in enumerate(tables):
            table[b, :len(t)] = t
            table[b, len(t):] = -1
        small = up[B * tmax:].view(np.int32)
        small[:B] = [len(t) for t in tables]
        small[B:B + hyps.size] = hyps.reshape(-1)
        small[B + hyps.size:n32] = lens.reshape(-1)
        dev = upload()
        dsmall = dev[B * tmax:].view(torch.int32)
        att, r_att = eng.rescore_rows(self._enc, dev[:B * tmax].view(B, tmax), dsmall[:B], dsmall[B:B + hyps.size].view(hyps.shape),
                                      dsmall[B + hyps.size:n32].view(lens.shape), with_right=dec.reverse_weight > 0)
        host = st.fetch(torch.stack([att, r_att]))
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
        for b, s in enumerate(sess):
            n = int(count[b])
            a, r = host[0, b, :n].copy(), host[1, b, :n].copy()
            total = combine(a, r, ctc[b], dec.ctc_weight, dec.reverse_weight)
            w = pick(total, n)
            s.rescored = {'nbest': nbest[b], 'ctc': ctc[b].tolist(), 'att': a.tolist(), 'r_att': r.tolist(), 'total': total.tolist(),
                          'winner': w}
            s.tokens = list(nbest[b][w])
            s.result = s.beam_last = {'text': token_text(self.vocab, s.tokens), 'score': float(total[w])}

    # ---- one batched step -------------------------------------------------------------------------------------------------
    def _featurize(self, sess):
        """features of all pending samples in one ragged launch (predict.py:274-281 per session), appended on the device to
        the sessions' rows of the feature pool; the carried-over samples are re-normalised in place on every call, exactly
        like the reference (audio.py:304).  The samples are assembled in pinned memory and copied asynchronously; nothing
        but the gains' mean squares travels back to the host."""
        eng, st = self.engine, self._stage
        n = len(sess)
        carried = [0 if s.remained is None else len(s.remained) for s in sess]
        lens = np.array([c + sum(len(a) for a in s.fresh) for c, s in zip(carried, sess)], np.int32)
        buf, upload_buf = st.take((n, max(int(lens.max()), self.min_samples)), np.float32)
        for i, s in enumerate(sess):
            s.samples += int(lens[i]) - carried[i]
            row, at = buf[i], carried[i]
            if at:
                row[:at] = s.remained
            for a in s.fresh:
                if a.dtype == np.float32:
                    row[at:at + len(a)] = a
                else:                                                  # int16 PCM: x / 2^15 in float32 (buf_to_float)
                    np.multiply(a, _PCM_SCALE, out=row[at:at + len(a)])
                at += len(a)
            row[at:] = 0
        xs, ns = upload_buf(), st.put(lens, np.int32)
        gain_h = gain = None
        if self.use_db:                                                # the reference's scalar expressions on this host
            gain_h = reference_gains(eng.mean_square(xs, ns).cpu().numpy(), self.target_db)
            gain = st.put(gain_h, np.float32)
        feats, _ = eng.features_batch(self.method, xs, ns, self.use_db, self.target_db, n_mfcc=self.n_mfcc, gain_in=gain)
        # frames per session: the front-end's own count (1 + (n - window) // 160), known without asking the device
        new = np.where(lens >= self.min_samples, (lens.astype(np.int64) - self.min_samples) // 160 + 1, 0)
        tmax = feats.shape[1]
        need = max(s.nf + int(new[i]) for i, s in enumerate(sess))
        if need > self._feat_cap:                                      # a whole utterance fed in one call: wider rows
            cap = max(need, 2 * self._feat_cap)
            wider = torch.zeros(self._feat.shape[0], cap, self.feat_dim, dtype=torch.float32, device=eng.device)
            wider[:, :self._feat_cap] = self._feat
            self._feat, self._feat_cap = wider, cap
        first = np.zeros(n, np.int64)                                  # flat pool index of each session's first new frame
        for i, s in enumerate(sess):
            nf, L = int(new[i]), int(lens[i])
            s.fresh = []
            rest = buf[i, 160 * nf:L]                                  # normalised in place, like AudioSegment.normalize
            s.remained = rest * np.float32(gain_h[i]) if self.use_db and L > 0 else rest.copy()
            if s.f0 + s.nf + nf > self._feat_cap:                      # make room: the live frames move to the front of the row
                self._feat[s.row, :s.nf] = self._feat[s.row, s.f0:s.f0 + s.nf].clone()
                s.f0 = 0
            first[i] = s.row * self._feat_cap + s.f0 + s.nf
            s.nf += nf
        total = int(new.sum())
        if total:
            offs = np.arange(total) - np.repeat(np.cumsum(new) - new, new)
            moves = self._dev_index(np.stack([np.repeat(np.arange(n, dtype=np.int64) * tmax, new) + offs,
                                              np.repeat(first, new) + offs]))
            self._feat.view(-1, self.feat_dim)[moves[1]] = feats.view(-1, self.feat_dim)[moves[0]]

    @property
    def last_packed(self):
        """(device rows [n, tmax + 2] = tokens | count | score bits, tmax, handles) of the greedy sessions that advanced in the
        last step -- what a multi-GPU front-end all-gathers (parallel.ShardedStreamPool) -- or None"""
        return self._last_packed

    def step(self):
        self._alive()
        self._last_packed = None
        fed, self._fed = self._fed, {}
        if not fed:
            return {}
        eng = self.engine
        sess = [self.sessions[h] for h in fed]
        self._stage.begin()
        self._featurize(sess)
        # windows of every session (predict.py:283-306), advanced in lock-step
        plans = [window_plan(s.nf, fed[s.sid]) for s in sess]
        for s in sess:
            s.result = None
        if self.rescoring:
            dec_beam = self.predictor.rescoring_decoder.beam_size
            n_windows = {s.sid: len(p) for s, p in zip(sess, plans)}
            read_nbest = set()            # sessions whose last decode_chunk of this step brought the n-best back
        for k in range(max((len(p) for p in plans), default=0)):
            groups = {}
            for s, p in zip(sess, plans):
                if k < len(p):
                    groups.setdefault(p[k][1] - p[k][0], []).append((s, p[k]))
            for length, items in groups.items():          # full windows together; a short last window on its own
                if eng.out_frames(length) <= 0:           # a last window below the front-end's minimum (conv2d6 / conv2d8): no frame
                    if self.beam:                         # nothing new to decode: the transcript so far (greedy re-collapses below)
                        for s, _ in items:
                            s.result = s.beam_last
                    continue
                # the windows are gathered from the device-resident feature pool: [items, length] flat frame indices
                base = np.array([s.row * self._feat_cap + s.f0 + a for s, (a, _) in items], np.int64)
                x = self._feat.view(-1, self.feat_dim)[self._dev_index(base[:, None] + np.arange(length)[None, :])]
                sids = [s.sid for s, _ in items]
                if self.beam:
                    if self.rescoring:
                        probs, _, _, enc = eng.encode_chunk(sids, x, want_probs=True, want_enc=True)
                        self._enc = self._append_rows(self._enc_alloc, self._enc, items, enc)
                    else:
                        probs, _, _ = eng.encode_chunk(sids, x, want_probs=True)
                    if self.timestamps:
                        self._keep_posteriors(items, probs)
                    for i, (s, _) in enumerate(items):
                        if self.rescoring:
                            # the last window of an utterance that ends here brings the search's n-best back with its result
                            last = fed[s.sid] and k == n_windows[s.sid] - 1
                            score, text = s.decoder.decode_chunk(probs=probs[i:i + 1], logits_lens=[probs.shape[1]],
                                                                 nbest=dec_beam if last else None)
                            if last:
                                read_nbest.add(s.sid)
                            res = {'text': text, 'score': score}
                        elif self.nbest is None:
                            score, text = s.decoder.decode_chunk(probs=probs[i:i + 1], logits_lens=[probs.shape[1]])
                            res = {'text': text, 'score': score}
                        else:
                            score, text = s.decoder.decode_chunk(probs=probs[i:i + 1], logits_lens=[probs.shape[1]], nbest=self.nbest)
                            res = {'text': text, 'score': score, 'nbest': [{'text': t, 'score': sc} for sc, t in s.decoder.last_nbest]}
                        s.frames += probs.shape[1]
                        s.result = s.beam_last = res
                        s.tokens = list(s.decoder.last_tokens)
                    continue
                probs, idx, mp = eng.encode_chunk(sids, x, want_probs=self.timestamps, want_argmax=True)
                if self.timestamps:
                    self._keep_posteriors(items, probs)
                tq = idx.shape[1]
                self._grow(0, max(s.frames for s, _ in items) + tq)
                at = self._dev_index(np.array([s.row * self._hist_idx.shape[1] + s.frames for s, _ in items],
                                              np.int64)[:, None] + np.arange(tq)[None, :])
                self._hist_idx.view(-1)[at] = idx                    # append this window's frames to the sessions' histories
                self._hist_mp.view(-1)[at] = mp
                for s, _ in items:
                    s.frames += tq
        # greedy: one collapse launch for every session that advanced -- full-history best path + score
        # (greedy_decoder_chunk semantics, ctc_greedy_decoder.py:52-89)
        adv = [s for s, p in zip(sess, plans) if p]
        if adv and not self.beam:
            rows = self._dev_index([s.row for s in adv])
            tmax = max(s.frames for s in adv)
            nfr = self._stage.put([s.frames for s in adv], np.int32)
            tok, ntok, score = eng.ctc_collapse(self._hist_idx[rows, :tmax].contiguous(), self._hist_mp[rows, :tmax].contiguous(), nfr)
            # one copy back: [tokens | count | score bits]
            packed_dev = torch.cat([tok, ntok[:, None], score.view(torch.int32)[:, None]], 1)
            self._last_packed = (packed_dev, tmax, [s.sid for s in adv])      # device copy: what a multi-GPU gather ships
            packed = packed_dev.cpu().numpy()
            tok, ntok, score = packed[:, :tmax], packed[:, tmax], packed[:, tmax + 1].copy().view(np.float32)
            for j, s in enumerate(adv):
                s.tokens = tok[j, :ntok[j]].tolist()
                s.result = greedy_result(self.vocab, s.tokens, score[j])
        if self.rescoring:
            # end of utterance: the second pass over all kept frames of every session that ends here and has any (a session that
            # never produced an encoder frame keeps what the CTC path gave it)
            ending = [s for s in sess if fed[s.sid] and s.frames > 0]
            for s in ending:
                if s.sid not in read_nbest:        # its last feed decoded no window: the live set as it stands
                    s.decoder.live_nbest(dec_beam)
            # one launch, or -- masr_rescore_rows takes B * N <= 65535 sequences per call -- one per 65535 // beam_size sessions
            per = max(1, 65535 // dec_beam)
            for at in range(0, len(ending), per):
                self._rescore(ending[at:at + per])
        if self.timestamps:
            self._stamp([s for s, p in zip(sess, plans) if p or (self.rescoring and fed[s.sid])])
        self._stage.end()
        out = {}
        for s, p in zip(sess, plans):
            if p:
                used = p[-1][1] - OVERLAP                                     # keep the overlap frames (predict.py:329)
                s.f0 += used
                s.nf -= used
            out[s.sid] = s.result
        return out
