"""One device pass of the offline path: the utterances of a pass are staged in pinned memory, uploaded and prepared on a side
stream (``begin``), then featurized, encoded and decoded by the configured decoder on the caller's stream and lane (``launch``).

A pass is always launched deferred: ``launch`` waits for nothing and returns a zero-argument function that waits for the pass
and returns its results; the non-deferred form is that function called at once.  Every decoder has one route (``_greedy_rows``,
``_greedy_calls``, ``_beam_search``, ``_rescoring``, ``_attention``, ``_joint``): it queues its work behind the encoder and returns a fetch
of [(token ids or text, score)] plus, with timestamps, the function that aligns those hypotheses.  What the routes share --
the frame counts, the aligner, the score rule, filling the results -- is written once below them.

``pass_plan.py`` decides how a list is cut into passes and pipelined; ``predict.py`` runs that plan over this class."""
import contextlib
import ctypes as C
import os
from collections import namedtuple

import numpy as np
import torch

from masr_amd._lib import check, debug_keys
from masr_amd.data_utils.resample import plan_rows
from masr_amd.decoders import ctc_alignment
from masr_amd.engine import reference_gains
from masr_amd.pinned import PinnedRing

# what the decoder routes of one pass work on: the engine, the rows that take part (``ok``: their indices in the pass, ``n``:
# their samples), the encoder output and its valid frames per row (None: every padded frame is decoded), and the call's flags
_Pass = namedtuple('_Pass', 'eng ok n min_samples enc nenc decode_all_frames want_ids defer timestamps nbest', defaults=(None,))


def device_resample():
    """MASR_DEVICE_RESAMPLE=0 (A/B): off-rate utterances are resampled on the host, one after the other, as before"""
    return os.environ.get('MASR_DEVICE_RESAMPLE', '1') != '0'


def greedy_score(score, ntok):
    """the greedy decoder's score in percent; an empty transcript that scored nothing counts 0"""
    return float(score) * 100.0 if ntok > 0 or score > 0 else 0


def empty_result(as_tokens, timestamps, nbest=None):
    """an utterance too short for one feature frame"""
    if as_tokens:
        return [], 0
    out = {'text': '', 'score': 0, 'tokens': []} if timestamps else {'text': '', 'score': 0}
    if nbest is not None:
        out['nbest'] = [{'text': '', 'score': 0}]
    return out


def first_of_nbest(fetch):
    """a fetch of per-utterance n-best lists -> (a fetch of every utterance's entry 0, what the other routes return; a box that
    holds the lists under 'many' once that fetch has run)"""
    box = {}

    def first():
        box['many'] = fetch()
        return [m[0] for m in box['many']]
    return first, box


class OfflinePasses:
    def __init__(self, engine, configs, vocab_list, beam=None, rescoring=None, attention=None, joint=None):
        self.eng, self.configs, self.vocab = engine, configs, vocab_list
        self.beam, self.rescoring, self.attention, self.joint = beam, rescoring, attention, joint
        # Pinned rings; the slot counts are the passes that may be in flight.  Staging: buffers take turns and each carries the
        # event of its last upload, so filling one never waits for the device unless that very buffer's previous copy (two
        # passes ago) is still in flight (a buffer's upload is complete long before the pass that staged it ends).
        self._stage = PinnedRing(2, headroom=True, events=True)            # per sample type
        self._stage_lens = PinnedRing(2, min_numel=64)                     # ... and its lengths, in step with it
        # native-rate rows: a pass takes one per distinct rate, and two passes are prepared ahead
        self._native = PinnedRing(4, headroom=True, events=True)
        self._mean_squares = PinnedRing(4, min_numel=64)
        self._rows = PinnedRing(4, min_numel=1 << 14)                      # packed result rows: at most two passes in flight
        self._named = PinnedRing(8, min_numel=1 << 12)                     # alignment read-backs: more slots than passes in flight
        self._sides, self._side_turn = None, 0
        self._frame_reduction = None

    def text(self, ids):
        return ''.join(self.vocab[j] for j in ids).replace('<space>', ' ')

    @property
    def rate(self):
        return int(self.configs.preprocess_conf.get('sample_rate', 16000))

    # ---- staging --------------------------------------------------------------------------------------------------------------
    def _stage_rows(self, ring, segs, n=None):
        """the rows of ``segs`` (their first ``n[i]`` samples; default: all) zero-padded into a slot of ``ring`` viewed [R, longest]
        -- int16 when every utterance still is the PCM it was loaded from: half the bytes over PCIe, x / 2^15 happens in the
        kernel -> (slot, pinned rows, lengths int32).  The caller records the slot once its upload is queued."""
        as_pcm = all(s._pcm16 is not None for s in segs)
        rows = [np.ascontiguousarray(s._pcm16 if as_pcm else s._samples, np.int16 if as_pcm else np.float32) for s in segs]
        n32 = np.array([r.shape[0] for r in rows], np.int32) if n is None else np.ascontiguousarray(n, np.int32)
        assert all(r.shape[0] >= int(m) for r, m in zip(rows, n32))
        width = int(n32.max())
        slot = ring.take(len(rows) * width, torch.int16 if as_pcm else torch.float32)
        stage = slot.buf.view(len(rows), width)
        # masr_stage_rows (csrc/stage.cpp): the rows of the pass into the pinned buffer, zero-padded, on four library threads --
        # 20 MB per pass of 32 x 20 s.  (Python threads over numpy row assignments: 0.45 ms per pass, one thread 0.66 ms; 2 / 8 / 12
        # python threads 17.0 / 17.4 / 18.5 ms per configs[2] greedy call against 16.9 with four; 16 row groups uploaded block by
        # block under the fill of the next block: 18.6 ms.)
        ptrs = (C.c_void_p * len(rows))(*[r.ctypes.data for r in rows])
        check(self.eng.lib.masr_stage_rows(C.c_void_p(stage.data_ptr()), width * stage.element_size(), ptrs,
                                           n32.ctypes.data_as(C.c_void_p), len(rows), stage.element_size(), 4))
        return slot, stage, n32

    def stage_batch(self, segs, n):
        """padded batch through a pinned staging buffer -> device samples [B, n_max] and lengths [B], on the CURRENT stream"""
        slot, stage, n32 = self._stage_rows(self._stage, segs, n)
        lens = self._stage_lens.take(len(segs), torch.int32, key=stage.dtype).buf
        lens.numpy()[:] = n32
        xs = stage.to(self.eng.device, non_blocking=True)
        ns = lens.to(self.eng.device, non_blocking=True)
        slot.record()
        return xs, ns

    def _upload_native(self, segs):
        """the rows of ONE source rate at that rate -> (device rows [R, longest], their lengths), on the current stream"""
        slot, stage, m32 = self._stage_rows(self._native, segs)
        src = stage.to(self.eng.device, non_blocking=True)
        slot.record()
        return src, m32

    def _stage_resampled(self, live, n, groups):
        """``stage_batch`` of a pass with rows off the model's rate, on the CURRENT stream: every distinct source rate's rows are
        staged and uploaded at that rate (PCM as int16) and ONE launch per rate resamples them into their rows of the pass's
        float32 input [B, n_max] -- the samples ``AudioSegment.resample`` makes, zeros behind each row's own length.  Rows at
        the model's rate are one more group, converted and copied by the same call."""
        eng = self.eng
        xs = torch.empty(len(live), int(n.max()), dtype=torch.float32, device=eng.device)
        for src_rate, rows in groups.items():
            src, m32 = self._upload_native([live[j] for j in rows])
            _, n_out = eng.resample_rows(src, m32, src_rate, self.rate, out=xs, dst_rows=rows)
            assert np.array_equal(n_out, n[rows])
        return xs, eng.to_device(np.ascontiguousarray(n, np.int32))

    def resample_long(self, seg, rate):
        """one recording -> its float32 samples at ``rate``, resampled on the device as a single row (``predict_long``)"""
        src, m32 = self._upload_native([seg])
        out, n_out = self.eng.resample_rows(src, m32, seg.sample_rate, rate)
        return self.eng.to_host(out[0, :int(n_out[0])])

    # ---- preparation ----------------------------------------------------------------------------------------------------------
    def prepare_begin(self, live, n, use_db, groups=None):
        """first half of a pass's preparation, nothing waited for: staging + upload + (bit-exact normalisation route) the mean
        squares on their way back to a pinned slot, all on the preparation stream (the host waits for THIS stream only, so
        preparing pass k + 1 never waits for the encoder of pass k on the main stream).  With two lanes it is issued for pass
        k + 1 BEFORE the encoder of pass k is launched: issued beside a running encoder pass, the upload and the mean squares start
        4 - 6 ms late (round 6; whichever side stream, 4 or 8 hardware queues).  ``groups`` (a pass with rows off the model's
        rate, ``begin``): the rows go up at their own rates and are resampled on the device, ``_stage_resampled``."""
        with torch.cuda.stream(self.eng.side_stream(2)):
            xs, ns = self.stage_batch(live, n) if groups is None else self._stage_resampled(live, n, groups)
            ms_host = None
            if use_db:
                ms_host = self._mean_squares.take(len(live), torch.float32).buf
                ms_host.copy_(self.eng.mean_square(xs, ns), non_blocking=True)
            ready = torch.cuda.Event()
            ready.record()
        return xs, ns, ms_host, ready

    def prepare_finish(self, began, target_db):
        """second half: the reference's gains -- the scalar float32 expressions of audio.py:287-304,519-529 in this host's numpy on
        the mean squares the device computed -- uploaded on the CURRENT stream (the pass's encoder stream), which then waits for
        the upload of the samples; the host has waited for the preparation stream's event only."""
        xs, ns, ms_host, ready = began
        main = torch.cuda.current_stream(self.eng.device)
        gain = None
        if ms_host is not None:
            ready.synchronize()
            gain = self.eng.to_device(reference_gains(ms_host.numpy().copy(), target_db))
        main.wait_event(ready)
        for t in (xs, ns):
            t.record_stream(main)
        return xs, ns, gain

    def begin(self, segs):
        """host side of a device pass + the asynchronous half of its preparation (``prepare_begin``); ``launch`` takes the result.
        Utterances too short for one feature frame are set aside here."""
        pc = self.configs.preprocess_conf
        rate = self.rate
        min_samples = 320 if pc.get('feature_method', 'fbank') == 'linear' else 400
        off_rate = any(s.sample_rate != rate for s in segs)
        if off_rate and not device_resample():
            for s in segs:
                if s.sample_rate != rate:
                    s.resample(rate)
            off_rate = False
        # lengths at the model's rate: what the host resampler would give, int(n * ratio), computed here -- the rows themselves
        # are resampled on the device behind their upload (``_stage_resampled``); a row too short for that raises as it did
        lengths = plan_rows([s.num_samples for s in segs], [s.sample_rate for s in segs], rate)[0] if off_rate else \
            [s.num_samples for s in segs]
        # 7 / 11 / 15 feature frames is the least Conv2dSubsampling4 / 6 / 8 accepts (subsampling.py:65-211)
        min_frames = getattr(self.eng, 'min_frames', 7)
        ok = [i for i, m in enumerate(lengths) if m >= min_samples + (min_frames - 1) * 160]
        live = [segs[i] for i in ok]
        n = np.array([lengths[i] for i in ok], np.int32)
        # one launch per distinct source rate among the rows that take part (row indices within ``live``)
        groups = plan_rows([s.num_samples for s in live], [s.sample_rate for s in live], rate)[1] if off_rate else None
        return {'count': len(segs), 'ok': ok, 'n': n, 'min_samples': min_samples,
                'prep': self.prepare_begin(live, n, pc.use_dB_normalization, groups) if ok else None}

    # ---- what the decoder routes share ----------------------------------------------------------------------------------------
    @staticmethod
    def _enc_lens(ps):
        """valid encoder frames per row on the device, int32 [B]"""
        if ps.nenc is not None:
            return ps.nenc
        return torch.full((len(ps.ok),), ps.enc.shape[1], dtype=torch.int32, device=ps.eng.device)

    @staticmethod
    def _n_host(ps):
        """the same on the host, from the sample counts: nothing is read back for it"""
        if ps.nenc is None:
            return [ps.enc.shape[1]] * len(ps.ok)
        return ps.eng.enc_frames((ps.n.astype(np.int64) - ps.min_samples) // 160 + 1).tolist()

    def search_stream(self):
        """the library's search streams of this device (masr_side_stream: queues of their own) take turns, so the searches of
        consecutive passes run next to each other, not one behind the other.  Two of them: with four side streams next to the
        main and the preparation stream the streams alias onto hardware queues (round 4: 50.1 vs 46.6 ms per configs[2] call)."""
        if self._sides is None:
            self._sides = [self.eng.side_stream(k) for k in range(max(1, min(2, int(os.environ.get('MASR_BEAM_SIDES', '2')))))]
        side = self._sides[self._side_turn]
        self._side_turn = (self._side_turn + 1) % len(self._sides)
        return side

    def search_streams(self):
        return self._sides or []

    def _align_queue(self, eng, probs, nenc, tok_dev, ntok_dev):
        """ONE masr_ctc_align call for a pass on the current stream and the active lane, and ONE copy of its packed results to
        pinned memory -> (pinned int32 buffer, what must stay alive until the copy is done)"""
        B, lmax = tok_dev.shape
        packed = torch.empty(B * (3 * lmax + 2), dtype=torch.int32, device=eng.device)
        eng.ctc_align(probs, nenc, tok_dev, ntok_dev, out=packed)
        host = self._named.take(packed.numel(), key='align').buf
        host.copy_(packed, non_blocking=True)
        return host, (probs, nenc, tok_dev, ntok_dev, packed)

    def _align_rows(self, eng, host, ids_list, lmax, n, alignable=None):
        """the packed alignment of a pass on the host -> the ``'tokens'`` value of every utterance of the pass"""
        rate = self.rate
        if self._frame_reduction is None:
            self._frame_reduction = eng.frame_reduction()
        start, end, peak, score, status = ctc_alignment.unpack_alignment(host.numpy(), len(ids_list), lmax)
        return [ctc_alignment.utterance_tokens(ids, start[j], end[j], peak[j], score[j],
                                               status[j] if alignable is None or alignable[j] else 1, self._frame_reduction, rate,
                                               float(n[j]) / rate, self.vocab) for j, ids in enumerate(ids_list)]

    def _aligner(self, ps, probs):
        """for the decoders whose hypotheses reach the host first (beam search, rescoring, attention, joint): the pass keeps its CTC
        posteriors ``probs`` on the device; the function returned takes the pass's [(token ids, score)] once they are known, sends
        the ids up in one small copy, aligns them with ONE masr_ctc_align call on the pass's own stream and lane, waits for the one
        copy back and returns the ``'tokens'`` values"""
        eng = ps.eng
        stream, lane, nenc = torch.cuda.current_stream(eng.device), eng.lane, self._enc_lens(ps)

        def align(res):
            ids_list = [[int(t) for t in r[0]] for r in res]
            flat, lmax, alignable = ctc_alignment.pack_hypotheses(ids_list, probs.shape[1])
            B = len(ids_list)
            with eng.on_lane(lane, stream):
                dev = eng.to_device(flat)
                host, keep = self._align_queue(eng, probs, nenc, dev[:B * lmax].view(B, lmax), dev[B * lmax:])
                ev = torch.cuda.Event()
                ev.record()
            ev.synchronize()
            del keep
            return self._align_rows(eng, host, ids_list, lmax, ps.n, alignable)
        return align

    # ---- the decoder routes: queue the decoding of ``ps`` -> (fetch of [(ids or text, score)], aligner or None) ---------------------
    def _greedy_rows(self, ps, xs, ns, gain):
        """ctc_greedy on fbank features: the whole pass is ONE C-ABI call and ONE copy back: rows [B, T' + 2] = tokens | count |
        score bits"""
        pc = self.configs.preprocess_conf
        rows = ps.eng.transcribe_rows(xs, ns, pc.use_dB_normalization, pc.target_dB, gain_in=gain,
                                      decode_all_frames=ps.decode_all_frames)
        host = self._rows.take(rows.numel()).buf.view(rows.shape)
        host.copy_(rows, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()

        def fetch():
            ev.synchronize()
            r = host.numpy()
            tp = r.shape[1] - 2
            ntok, score = r[:, tp], r[:, tp + 1].copy().view(np.float32)
            return [(r[j, :ntok[j]].tolist(), greedy_score(score[j], ntok[j])) for j in range(len(ps.ok))]
        return fetch, None

    def _greedy_calls(self, ps):
        """ctc_greedy in separate calls (other features; timestamps)"""
        eng = ps.eng
        idx, mp = eng.ctc_greedy_frames(ps.enc)
        tok, ntok, score = eng.ctc_collapse(idx, mp, ps.nenc)
        if not ps.timestamps:
            tok, ntok, score = eng.to_host(tok), eng.to_host(ntok), eng.to_host(score)
            return (lambda: [(tok[j, :ntok[j]].tolist(), greedy_score(score[j], ntok[j])) for j in range(len(ps.ok))]), None
        # the greedy tokens never leave the device before they are aligned: the CTC head's posteriors, ONE masr_ctc_align call
        # behind the collapse, and the hypotheses and the packed alignment come back behind one event
        B, Tp = tok.shape
        lmax = min(Tp, ctc_alignment.MAX_TOKENS)          # (a longer hypothesis comes back with status 2: 'tokens' is None)
        frames_dev = self._enc_lens(ps)
        tok_in = tok if lmax == Tp else tok[:, :lmax].contiguous()
        a_host, keep = self._align_queue(eng, eng.ctc_probs(ps.enc), frames_dev.contiguous(), tok_in, ntok)
        g_host = self._named.take(B * Tp + 2 * B, key='greedy').buf
        g_host[:B * Tp].view(B, Tp).copy_(tok, non_blocking=True)
        g_host[B * Tp:B * Tp + B].copy_(ntok, non_blocking=True)
        g_host[B * Tp + B:].view(torch.float32).copy_(score, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        keep = keep + (tok, ntok, score)

        def fetch(_keep=keep):
            ev.synchronize()
            g = g_host.numpy()
            tok_h, ntok_h, score_h = g[:B * Tp].reshape(B, Tp), g[B * Tp:B * Tp + B], g[B * Tp + B:].view(np.float32)
            return [(tok_h[j, :ntok_h[j]].tolist(), greedy_score(score_h[j], ntok_h[j])) for j in range(B)]
        return fetch, lambda res: self._align_rows(eng, a_host, [r[0] for r in res], lmax, ps.n)

    def _attention(self, ps):
        """the search is queued behind this pass's encoder on the SAME stream and lane (the caller selected them): no CTC head,
        no prefix search; the host waits at the search's end polls and fetches the hypotheses behind an event"""
        enc_lens = self._enc_lens(ps)
        # (timestamps: the CTC head runs for the alignment alone, in front of the search)
        align = self._aligner(ps, ps.eng.ctc_probs(ps.enc)) if ps.timestamps else None
        return self.attention.decode_pass(ps.eng, ps.enc, enc_lens.contiguous(), want_tokens=ps.want_ids), align

    def _joint(self, ps):
        """CTC head, then the joint search over this pass's encoder output and those posteriors, queued on the SAME stream and lane
        (the caller selected them); the aligner reuses the same posteriors; the host waits at the search's end polls and fetches
        the hypotheses behind an event"""
        probs = ps.eng.ctc_probs(ps.enc)
        enc_lens = self._enc_lens(ps)
        align = self._aligner(ps, probs) if ps.timestamps else None
        return self.joint.decode_pass(ps.eng, ps.enc, enc_lens.contiguous(), probs, want_tokens=ps.want_ids), align

    def _rescoring(self, ps):
        """first pass: CTC head, vocabulary pruning on the GPU, the n-best prefixes of the LM-free prefix search; second pass:
        both attention decoders over this pass's encoder output, queued behind it on the SAME stream and lane (the caller
        selected them), so two passes on two lanes never share a decoder workspace; the host waits for the first pass
        (pruned candidates, host-thread search), never for the second: its results are fetched behind an event"""
        probs = ps.eng.ctc_probs(ps.enc)
        n_host, enc_lens = self._n_host(ps), self._enc_lens(ps)
        align = self._aligner(ps, probs) if ps.timestamps else None
        return self.rescoring.decode_pass(ps.eng, ps.enc, enc_lens.contiguous(), probs, n_host, want_tokens=ps.want_ids), align

    def _beam_search(self, ps):
        """CTC prefix beam search: the probabilities stay on the GPU (vocabulary pruning, prefix search and LM scoring run there),
        searched in place: padded [B, T', V] + the valid frames per utterance"""
        eng, dec, want = ps.eng, self.beam, ps.want_ids
        probs = eng.ctc_probs(ps.enc)
        n_host = self._n_host(ps)
        align = self._aligner(ps, probs) if ps.timestamps else None
        if ps.nbest is not None:
            return self._beam_search_nbest(ps, probs, n_host, align)
        if ps.defer and dec.use_gpu_search and dec.gpu_search_supported(probs.shape[1], probs.shape[2]):
            # The prefix search of a pass (one workgroup per utterance, frames in sequence) runs on a side stream
            # (``search_stream``), launched at once: the call is bound by the longest utterance's ~30 us per frame x 494 frames, and
            # starting that search late costs more than sharing CUs with the next encoder pass (tools/studies/README.md, held
            # searches).
            main = torch.cuda.current_stream(eng.device)          # (explicit device: a server runs one worker thread per GPU)
            side = self.search_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                pending = dec._batch(probs, defer=True, frames=n_host)
            return (lambda: dec._batch_collect(pending, want_tokens=want)), align
        if ps.defer and os.environ.get('MASR_HOST_SEARCH_DEFER', '1') == '1':
            # host-thread search (word-based scorer, sizes beyond the GPU kernel): pruning queued now, candidates fetched and
            # searched when the results are collected -- under the encoders of the passes launched in between
            return dec.search_host_deferred(probs, n_host, want_tokens=want), align
        res = dec._batch(probs, want_tokens=want, frames=n_host)
        if align is not None:
            toks = align(res)
            return (lambda: res), lambda _res: toks
        return (lambda: res), None

    def _beam_search_nbest(self, ps, probs, n_host, align):
        """``_beam_search`` with ``nbest=N``: the same launches plus the n-best kernel behind the search, the rows in the search's
        one packed copy; entry 0 of every utterance takes the place of the single result (alignment included).  Beyond the GPU
        search the host-thread search gives them at once (LM-free; refused by name with a scorer bound)."""
        eng, dec, want = ps.eng, self.beam, ps.want_ids
        if ps.defer and dec.use_gpu_search and dec.gpu_search_supported(probs.shape[1], probs.shape[2]):
            main = torch.cuda.current_stream(eng.device)
            side = self.search_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                pending = dec._batch(probs, defer=True, frames=n_host, nbest=ps.nbest)
            fetch, self._nbest_box = first_of_nbest(lambda: dec._batch_collect(pending, want_tokens=want))
            return fetch, align
        many = dec._batch(probs, want_tokens=want, frames=n_host, nbest=ps.nbest)
        fetch, self._nbest_box = first_of_nbest(lambda: many)
        if align is not None:
            toks = align(fetch())
            return fetch, lambda _res: toks
        return fetch, None

    # ---- one pass ---------------------------------------------------------------------------------------------------------------
    def _decode(self, began, decode_all_frames, want_ids, defer, timestamps, nbest=None):
        """features, encoder and the configured decoder's route of the rows of ``began`` that take part, on the current stream"""
        eng, pc, decoder = self.eng, self.configs.preprocess_conf, self.configs.decoder
        method = pc.get('feature_method', 'fbank')
        xs, ns, gain = self.prepare_finish(began['prep'], pc.target_dB)
        ps = _Pass(eng, began['ok'], began['n'], began['min_samples'], None, None, decode_all_frames, want_ids, defer, timestamps, nbest)
        greedy = decoder not in ('ctc_beam_search', 'attention_rescoring', 'attention', 'joint')
        if greedy and method == 'fbank' and not timestamps:
            return self._greedy_rows(ps, xs, ns, gain)
        feats, frames = eng.features_batch(method, xs, ns, pc.use_dB_normalization, pc.target_dB, n_mfcc=pc.get('n_mfcc', 40),
                                           gain_in=gain)
        # the padded frames are decoded too: the engine must compute them (masr_debug_set key 38)
        with debug_keys(eng, skip_padding=0) if decode_all_frames else contextlib.nullcontext():
            enc = eng.encode_full(feats, frames, -1)
        ps = ps._replace(enc=enc, nenc=None if decode_all_frames else eng.enc_frames(frames).to(torch.int32))
        if greedy:
            return self._greedy_calls(ps)
        return {'attention': self._attention, 'joint': self._joint, 'attention_rescoring': self._rescoring,
                'ctc_beam_search': self._beam_search}[decoder](ps)

    def launch(self, began, decode_all_frames=False, as_tokens=False, defer=False, timestamps=False, nbest=None):
        """the pass ``began`` (``begin``) on the current stream and the active lane -> a zero-argument function that waits for it
        and returns [{'text', 'score'}] (``as_tokens``: [(token ids, score)]) in the order of the pass.  Utterances too short for
        one feature frame decode to the empty transcript (the reference's encoder cannot take them either); a digitally silent
        utterance (mean square 0) is normalised with gain = target_dB like the reference (audio.py:519-529), only a gain above
        max_gain_db raises (:300-303).  ``defer=True``: the caller collects later and launches the next pass underneath this one,
        so nothing may be waited for here (beam search on the GPU: the prefix search runs on a side stream); otherwise the caller
        calls the function at once.  ``timestamps=True``: every result gains ``'tokens'`` (decoders/ctc_alignment.py).  The pass
        keeps its CTC posteriors on the device until its hypotheses are known and aligns them with one masr_ctc_align call
        (``attention`` runs the CTC head for that alone); ``ctc_greedy`` takes the route of separate calls whatever the features.
        ``nbest=N`` (ctc_beam_search only; the caller has validated it): every result gains ``'nbest'``: [{'text', 'score'}]."""
        if timestamps and as_tokens:
            raise Exception(ctc_alignment.DISTRIBUTED_REFUSAL)
        if nbest is not None and (as_tokens or self.configs.decoder != 'ctc_beam_search'):
            raise ValueError("nbest needs decoder='ctc_beam_search' and is not available on the sharded path")
        ok = began['ok']
        out = [None] * began['count']
        for i in set(range(began['count'])) - set(ok):
            out[i] = empty_result(as_tokens, timestamps, nbest)
        if not ok:
            return lambda: out
        fetch, align = self._decode(began, decode_all_frames, as_tokens or timestamps, defer, timestamps, nbest)
        box = self._nbest_box if nbest is not None else None          # (this pass's: the next launch replaces the attribute)

        def entry(e):
            a, b = e
            if isinstance(b, str):                     # (score, text)
                a, b = b, a
            return {'text': a if isinstance(a, str) else self.text(a), 'score': b}

        def collect():
            res = fetch()
            toks = align(res) if align is not None else None
            for j, i in enumerate(ok):
                first, score = res[j]
                if isinstance(score, str):             # (the decoders' own (score, text) order)
                    first, score = score, first
                if as_tokens:
                    out[i] = (first, score)
                    continue
                out[i] = {'text': first if isinstance(first, str) else self.text(first), 'score': score}
                if toks is not None:
                    out[i]['tokens'] = toks[j]
                if box is not None:
                    out[i]['nbest'] = [entry(e) for e in box['many'][j]]
            return out
        return collect
