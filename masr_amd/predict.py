"""MASRPredictor -- the reference facade (masr/predict.py) on the MI355X engine.

Same constructor and ``predict`` / ``predict_long`` / ``predict_stream`` / ``reset_stream`` contract
(predict.py:20-26,167-171,195-199,237-244,346); everything between the audio and the text runs in libmasr_hip.so.
How the calls map onto the engine:

  * ``predict`` is ``predict_batch`` with a batch of one: padded PCM -> features -> encoder -> CTC decode in one device
    pass, no numpy round trips between the reference's stages;
  * ``predict_stream`` is a ``serving.StreamPool`` with a single session (the pool is the one implementation of the
    reference's stream framing; a server opens more sessions on the same pool);
  * ``predict_batch`` / ``evaluate`` shard their utterances over the ranks of an initialised ``torch.distributed`` process
    group (one process per GPU, ``parallel.py``) and all-gather the hypotheses.

The offline path is three files: ``pass_plan.py`` cuts a length-sorted list into device passes and decides how they are pipelined
(pure functions), ``offline_pass.py`` stages, prepares and decodes one pass (``OfflinePasses``; pinned buffers from ``pinned.py``),
and this class runs the plan: ``_run_sorted`` for ``predict_batch``, one pass for ``predict`` / ``predict_batch_deferred``.
"""
import json
import logging
import os
from io import BufferedReader

import numpy as np
import torch
import yaml

from masr_amd import SUPPORT_MODEL, parallel
from masr_amd.data_utils.audio import AudioSegment
from masr_amd.data_utils.featurizer.audio_featurizer import AudioFeaturizer
from masr_amd.data_utils.featurizer.text_featurizer import TextFeaturizer
from masr_amd.decoders.ctc_greedy_decoder import greedy_decoder
from masr_amd.infer_utils.inference_predictor import InferencePredictor
from masr_amd.offline_pass import OfflinePasses, device_resample
from masr_amd.pass_plan import balanced_cuts, pass_cuts, pass_policy, search_on_gpu      # noqa: F401 (balanced_cuts: public here)
from masr_amd.utils.utils import dict_to_object

logger = logging.getLogger(__name__)


class MASRPredictor:
    def __init__(self, configs=None, model_tag='conformer_streaming_fbank_aishell',
                 model_path='models/conformer_streaming_fbank/inference.pt', use_pun=False,
                 pun_model_dir='models/pun_models/', use_gpu=True, state_dict=None):
        if not configs:
            raise Exception('no network here: pass `configs` (YAML path or dict) and `model_path` explicitly')
        if isinstance(configs, str):
            with open(configs, 'r', encoding='utf-8') as f:
                configs = yaml.load(f.read(), Loader=yaml.FullLoader)
        self.configs = dict_to_object(configs)
        assert self.configs.use_model in SUPPORT_MODEL, f'没有该模型：{self.configs.use_model}'
        if use_pun:
            raise Exception('punctuation (PaddleNLP) is outside the hot path and not provided')
        self.running = False
        self.use_gpu = use_gpu
        self._text_featurizer = TextFeaturizer(vocab_filepath=self.configs.dataset_conf.dataset_vocab)
        self._audio_featurizer = AudioFeaturizer(**self.configs.preprocess_conf)
        self.beam_search_decoder = None
        self.vad_predictor = None
        self._pool = None             # predict_stream: a StreamPool with one session, opened on first use
        self._pool_timestamps = False    # ... created with timestamps=True?
        self._stream_running = False     # an utterance of predict_stream has begun (its first call fixed the flag)
        self._session = None
        if self.configs.decoder == 'ctc_beam_search':
            # predict.py:96-109; the search is masr_amd's own (vocabulary pruning, prefix search and LM scoring on the GPU)
            from masr_amd.decoders.beam_search_decoder import BeamSearchDecoder
            self.beam_search_decoder = BeamSearchDecoder(vocab_list=self._text_featurizer.vocab_list,
                                                         **self.configs.ctc_beam_search_decoder_conf)
        self.rescoring_decoder = None
        if self.configs.decoder == 'attention_rescoring':
            # second pass with the checkpoint's attention decoder over the CTC n-best (decoders/attention_rescoring.py); the
            # configuration is checked before anything is loaded
            from masr_amd.decoders.attention_rescoring import AttentionRescoringDecoder, validate_rescoring_conf
            if self.configs.use_model == 'deepspeech2':
                raise Exception("decoder='attention_rescoring' is not available for use_model deepspeech2: it has no attention "
                                "decoder (its decoder.* tensors are the CTC head)")
            dconf = dict(self.configs.get('decoder_conf', {}) or {})
            rconf = validate_rescoring_conf(self.configs.get('attention_rescoring_decoder_conf', None),
                                            self.configs.get('model_conf', None), dconf.get('r_num_blocks', 0))
            self.rescoring_decoder = AttentionRescoringDecoder(vocab_list=self._text_featurizer.vocab_list, **rconf)
        self.attention_decoder = None
        if self.configs.decoder == 'attention':
            # autoregressive beam search with the checkpoint's attention decoder, on the GPU (decoders/attention_decoder.py); the
            # configuration is checked before anything is loaded
            from masr_amd.decoders.attention_decoder import AttentionDecoder, DS2_REFUSAL, validate_attention_conf
            if self.configs.use_model == 'deepspeech2':
                raise Exception(DS2_REFUSAL)
            aconf = validate_attention_conf(self.configs.get('attention_decoder_conf', None), len(self._text_featurizer.vocab_list))
            self.attention_decoder = AttentionDecoder(vocab_list=self._text_featurizer.vocab_list, **aconf)
        self.joint_decoder = None
        if self.configs.decoder == 'joint':
            # the attention search ranked jointly with the CTC prefix score, on the GPU (decoders/joint_decoder.py); the
            # configuration is checked before anything is loaded
            from masr_amd.decoders.joint_decoder import JointDecoder, DS2_REFUSAL, load_language_model, validate_joint_conf
            if self.configs.use_model == 'deepspeech2':
                raise Exception(DS2_REFUSAL)
            jconf = validate_joint_conf(self.configs.get('joint_decoder_conf', None), self.configs.get('model_conf', None),
                                        len(self._text_featurizer.vocab_list))
            # shallow fusion: the ARPA model of language_model_path, loaded only where lm_weight > 0 uses it
            lm_path = jconf.pop('language_model_path', None)
            if lm_path is not None:
                jconf['language_model'] = load_language_model(lm_path, self._text_featurizer.vocab_list)
            self.joint_decoder = JointDecoder(vocab_list=self._text_featurizer.vocab_list, **jconf)
        if state_dict is None and not os.path.exists(model_path):
            raise Exception("模型文件不存在，请检查{}是否存在！".format(model_path))
        self.predictor = InferencePredictor(configs=self.configs, use_model=self.configs.use_model,
                                            streaming=self.configs.streaming, model_path=model_path,
                                            use_gpu=self.use_gpu, state_dict=state_dict)
        self._audio_featurizer.bind(self.predictor.engine)
        self._passes = OfflinePasses(self.predictor.engine, self.configs, self._text_featurizer.vocab_list,
                                     beam=self.beam_search_decoder, rescoring=self.rescoring_decoder, attention=self.attention_decoder,
                                     joint=self.joint_decoder)
        self._deferred_turn, self._lane1_ordered = 0, False
        # warm-up like the reference (predict.py:89-92)
        warmup_audio = np.random.uniform(low=-2.0, high=2.0, size=(134240,))
        self.predict(audio_data=warmup_audio, is_itn=False)
        self.reset_stream()

    # ---- helpers ----------------------------------------------------------------------------------------------------------
    def decode(self, output_data, use_pun, is_itn):
        """predict.py:118-144: probabilities [T', V] of one utterance -> (score, text)."""
        if self.configs.decoder == 'attention_rescoring':
            raise Exception("decoder='attention_rescoring' needs the encoder output of the utterance, not only its probabilities: "
                            "use predict / predict_batch")
        if self.configs.decoder == 'attention':
            from masr_amd.decoders.attention_decoder import DECODE_REFUSAL
            raise Exception(DECODE_REFUSAL)
        if self.configs.decoder == 'joint':
            from masr_amd.decoders.joint_decoder import DECODE_REFUSAL
            raise Exception(DECODE_REFUSAL)
        if self.configs.decoder == 'ctc_beam_search':
            score, text = self.beam_search_decoder.decode_beam_search_offline(probs_split=output_data)
        else:
            score, text = greedy_decoder(probs_seq=output_data, vocabulary=self._text_featurizer.vocab_list)
        self._no_itn(is_itn)
        return score, text

    @staticmethod
    def _no_itn(is_itn):
        if is_itn:
            raise Exception('inverse text normalisation (WeTextProcessing) is outside the hot path')

    @staticmethod
    def _load_audio(audio_data, sample_rate=16000):
        """predict.py:146-164: path / binary file object / ndarray / wav bytes -> AudioSegment."""
        loaders = ((str, AudioSegment.from_file), (BufferedReader, AudioSegment.from_file),
                   (np.ndarray, lambda a: AudioSegment.from_ndarray(a, sample_rate)), (bytes, AudioSegment.from_bytes))
        for kind, load in loaders:
            if isinstance(audio_data, kind):
                return load(audio_data)
        raise Exception(f'不支持该数据类型，当前数据类型为：{type(audio_data)}')

    def _text(self, ids):
        vocab = self._text_featurizer.vocab_list
        return ''.join(vocab[j] for j in ids).replace('<space>', ' ')

    def _nbest(self, nbest):
        """``nbest=N`` of the predict calls -> N, or None when it is not asked for; refused by name where there is no such n-best:
        a decoder other than ctc_beam_search, N outside 1 .. beam_size, a word-based scorer (its search runs on host threads,
        whose n-best is LM-free)"""
        if nbest is None:
            return None
        decoder = self.configs.decoder
        if decoder == 'joint':
            from masr_amd.decoders.joint_decoder import NBEST_REFUSAL
            raise ValueError(NBEST_REFUSAL.format(nbest=nbest))
        if decoder in ('attention_rescoring', 'attention'):
            raise ValueError(f"nbest={nbest!r} with decoder={decoder!r}: nbest returns the prefixes of the CTC prefix beam search "
                             f"(decoder='ctc_beam_search'); the n-best of {decoder} -- its rescored or autoregressive hypotheses -- "
                             f"is not this one and is not returned")
        if decoder != 'ctc_beam_search':
            raise ValueError(f"nbest={nbest!r} with decoder={decoder!r}: only decoder='ctc_beam_search' keeps more than one hypothesis")
        dec = self.beam_search_decoder
        nbest = dec.check_nbest(nbest)
        if dec._ext_scorer is not None and not dec._ext_scorer.is_character_based:
            raise ValueError('nbest with a word-based language model: that search runs on host threads, whose n-best '
                             '(masr_beam_search_batch_nbest) is LM-free; use a character-based model or language_model_path=None')
        return nbest

    # ---- offline ------------------------------------------------------------------------------------------------------------
    def predict(self, audio_data, use_pun=False, is_itn=False, sample_rate=16000, timestamps=False, nbest=None):
        """predict.py:167-192: one utterance -> {'text', 'score'} (a batch of one on the device path).  ``timestamps=True``: the
        result gains ``'tokens'``: [{'token', 'start', 'end', 'score'}] per token of the text, in seconds of the utterance (CTC
        forced alignment of the hypothesis on the GPU, decoders/ctc_alignment.py); [] for an empty transcript, None when the CTC
        trellis holds no path for the hypothesis.  ``nbest=N`` (decoder ctc_beam_search, 1 <= N <= beam_size): the result gains
        ``'nbest'``: [{'text', 'score'}] of the (at most) N best prefixes of the search, best first, entry 0 being the result's
        own text and score; without it the result is what it was, key for key."""
        nbest = self._nbest(nbest)
        self._no_itn(is_itn)
        return self._predict_local([self._load_audio(audio_data, sample_rate)], timestamps=timestamps, nbest=nbest)[0]

    def init_vad(self, vad_predictor=None):
        """predict.py:110-115: ``VADPredictor()`` -- the Silero network (on the GPU, weights from the reference's
        ``silero_vad.onnx``: infer_utils/silero_vad.py says where the file is looked for; without it this raises).
        ``vad_predictor``: any object with the reference VADPredictor's ``get_speech_timestamps`` instead, e.g. the built-in
        ``EnergyVAD`` stand-in for callers without the Silero file."""
        if vad_predictor is not None:
            self.vad_predictor = vad_predictor
        elif getattr(self, 'vad_predictor', None) is None:
            from masr_amd.infer_utils.vad_predictor import VADPredictor
            self.vad_predictor = VADPredictor()

    def predict_long(self, audio_data, use_pun=False, is_itn=False, sample_rate=16000, vad_predictor=None, batch_size=32,
                     timestamps=False, nbest=None):
        """predict.py:195-234: long audio -> VAD segments -> text.  The reference recognises the segments one after the
        other (``self.predict`` per segment, :220); here they go through ``predict_batch`` in length-sorted batches of
        ``batch_size`` (one device pass per batch); texts are joined in time order exactly like the reference (:222-227,233).
        A padded batch follows the reference's own batch > 1 semantics (its pad mask keeps one padding-contaminated key per
        shorter utterance, trainer.py:632); ``batch_size=1`` is the reference's per-segment ``predict`` to the bit.
        ``timestamps=True``: the result gains ``'tokens'`` (see ``predict``) over the WHOLE recording in time order: every
        token's times are shifted by the start of its VAD segment.  ``nbest=N``: the result gains ``'nbest'``: per VAD segment, in
        time order, that segment's [{'text', 'score'}] (see ``predict``) -- the segments' alternatives are not multiplied out."""
        nbest = self._nbest(nbest)
        if use_pun:
            raise Exception('punctuation (PaddleNLP) is outside the hot path and not provided')
        self._no_itn(is_itn)
        self.init_vad(vad_predictor)
        audio_segment = self._load_audio(audio_data=audio_data, sample_rate=sample_rate)
        if audio_segment.sample_rate != self.configs.preprocess_conf.sample_rate:
            if device_resample():
                # the recording as ONE long row through the resampling kernel (the samples AudioSegment.resample makes) and back
                # to the host, where the VAD and the segmentation read it
                rate = self.configs.preprocess_conf.sample_rate
                audio_segment = AudioSegment.from_ndarray(self._resample_long(audio_segment, rate), rate)
            else:
                audio_segment.resample(self.configs.preprocess_conf.sample_rate)
        samples = audio_segment.samples
        stamps = self.vad_predictor.get_speech_timestamps(samples, audio_segment.sample_rate)
        pieces = [samples[t['start']: t['end']] for t in stamps]
        order = sorted(range(len(pieces)), key=lambda i: len(pieces[i]))
        results = [None] * len(pieces)
        for lo in range(0, len(order), batch_size):
            idx = order[lo:lo + batch_size]
            for i, res in zip(idx, self._predict_local([AudioSegment.from_ndarray(pieces[i], audio_segment.sample_rate)
                                                        for i in idx], timestamps=timestamps, **({} if nbest is None else {'nbest': nbest}))):
                results[i] = res
        texts, scores = '', []
        for res in results:
            if res['text'] != '':
                texts = texts + '，' + res['text']
            scores.append(res['score'])
            logger.info(f'长语音识别片段结果：{res["text"]}')
        if texts[:1] == '，':
            texts = texts[1:]
        out = {'text': texts, 'score': round(sum(scores) / len(scores), 2) if scores else 0}
        if nbest is not None:
            out['nbest'] = [res['nbest'] for res in results]
        if timestamps:
            from masr_amd.decoders.ctc_alignment import join_segments
            out['tokens'] = join_segments([res['tokens'] for res in results],
                                          [t['start'] / float(audio_segment.sample_rate) for t in stamps])
        return out

    # ---- one device pass (offline_pass.py) under the names the tests and tools use as seams ------------------------------------------
    def _begin_pass(self, segs):
        return self._passes.begin(segs)

    def _prepare_finish(self, began, target_db):
        return self._passes.prepare_finish(began, target_db)

    def _resample_long(self, seg, rate):
        return self._passes.resample_long(seg, rate)

    def _predict_local(self, segs, decode_all_frames=False, as_tokens=False, timestamps=False, nbest=None):
        """AudioSegments -> [{'text','score'}] on THIS rank's engine: one pass on the current stream, waited for"""
        return self._passes.launch(self._begin_pass(segs), decode_all_frames, as_tokens, timestamps=timestamps, nbest=nbest)()

    def _gpu_search(self):
        """does the configured decoder's prefix search run on the GPU?"""
        return search_on_gpu(self.beam_search_decoder if self.configs.decoder == 'ctc_beam_search' else None,
                             len(self._text_featurizer.vocab_list))

    def _length_hint(self, audio_data, sample_rate):
        """number of samples an utterance will have at the model's rate, WITHOUT decoding it where that is possible (wav
        path / wav bytes: the header; ndarray: its length) -- what sorting into passes and sharding over ranks need"""
        rate = int(self.configs.preprocess_conf.get('sample_rate', 16000))
        try:
            if isinstance(audio_data, np.ndarray):
                return int(audio_data.shape[0] * rate // max(int(sample_rate), 1))
            if isinstance(audio_data, (str, bytes)):
                import io
                import wave
                with wave.open(audio_data if isinstance(audio_data, str) else io.BytesIO(audio_data), 'rb') as w:
                    return int(w.getnframes() * rate // max(w.getframerate(), 1))
        except Exception:
            pass
        return self._load_audio(audio_data, sample_rate).num_samples        # file objects and anything odd: decode

    def pass_size(self):
        """utterances of ~10 s per device pass that fill the chip for this model family: 32 are 248 row blocks of 32 for 256 CUs;
        the Efficient-Conformer runs at half the frame rate behind its stride layer, where it takes 64"""
        return 64 if self.configs.use_model == 'efficient_conformer' else 32

    def predict_batch(self, audio_list, sample_rate=16000, decode_all_frames=False, batch_size=0, distributed=None,
                      lengths=None, pass_padded=None, timestamps=False, nbest=None):
        """Batched offline path (an addition; the reference's only batched consumer is MASRTrainer.evaluate,
        trainer.py:592-651): a list of utterances -> [{'text','score'}] in input order.

        ``decode_all_frames=True`` reproduces the reference's batch evaluation quirk of decoding padded frames
        (trainer.py:340).  ``batch_size`` > 0 cuts the (length-sorted) work into device passes of that many utterances
        (``batch_size='auto'``: ``pass_size()`` -- 32, or 64 for the Efficient-Conformer; a LIST gives the pass sizes explicitly,
        counted from the longest utterance down, the last size repeating).  ``batch_size='balanced'``: passes of
        EQUAL PADDED SIZE instead of equal count -- a pass takes utterances (longest first) while count x its longest
        utterance stays within ``pass_padded`` (in the unit of the lengths; default: ``pass_size()`` utterances of 10 s, the row
        blocks that fill the chip once), so a pass of long utterances holds few of them, a pass of short ones many, every pass is
        one full round of workgroups and nobody is padded to the longest utterance of the whole list.  The
        audio of a pass is decoded when the pass is formed and dropped when its results are in, at most two passes are in
        flight (features + encoder of pass k under the prefix search of pass k - 1), so host memory and HBM hold two passes
        whatever the list's length.  ``lengths`` (samples or seconds, any common unit): known durations, e.g. a manifest's,
        used for sorting and sharding instead of reading every file's header.
        With an initialised ``torch.distributed`` group (``distributed=None``: automatically when world > 1) the utterances
        are dealt out length-balanced over the ranks -- every rank must call with the same list -- each rank decodes ONLY
        its shard on its own GPU and ONE all-gather of the token ids returns all hypotheses to every rank.
        ``timestamps=True``: every result gains ``'tokens'`` (see ``predict``); refused on the sharded path.
        ``nbest=N``: every result gains ``'nbest'`` (see ``predict``); refused on the sharded path."""
        nbest = self._nbest(nbest)
        hints = list(lengths) if lengths is not None else [self._length_hint(a, sample_rate) for a in audio_list]
        if batch_size == 'auto':
            batch_size = self.pass_size()
        if batch_size == 'balanced':
            rate = int(self.configs.preprocess_conf.get('sample_rate', 16000))
            if pass_padded is None:
                if lengths is not None:
                    raise ValueError("batch_size='balanced' with caller-supplied lengths needs pass_padded in the same unit "
                                     "(evaluate() passes manifest durations and derives it: pass_size() x 10 seconds)")
                pass_padded = self.pass_size() * 10 * rate
            batch_size = ('balanced', float(pass_padded))
        rank, world = parallel.world_info()
        if distributed is None:
            distributed = world > 1
        if timestamps and distributed:
            from masr_amd.decoders.ctc_alignment import DISTRIBUTED_REFUSAL
            raise Exception(DISTRIBUTED_REFUSAL)
        if nbest is not None and distributed:
            raise ValueError('nbest is not available on the sharded path (predict_batch under a process group): the all-gather '
                             'carries one hypothesis per utterance; call with distributed=False')
        if not distributed or not parallel.collectives_on():
            return self._run_sorted(audio_list, sample_rate, hints, list(range(len(audio_list))), decode_all_frames, batch_size,
                                    as_tokens=False, timestamps=timestamps, nbest=nbest)
        shards = parallel.length_balanced_shards(hints, world)
        mine = shards[rank]
        local = self._run_sorted(audio_list, sample_rate, hints, mine, decode_all_frames, batch_size, as_tokens=True)
        tmax = max([len(t) for t, _ in local], default=0)
        tok = torch.full((len(mine), max(tmax, 1)), -1, dtype=torch.int32)
        nt = torch.zeros(len(mine), dtype=torch.int32)
        sc = torch.zeros(len(mine), dtype=torch.float32)
        for j, (t, s) in enumerate(local):
            tok[j, :len(t)] = torch.tensor(t, dtype=torch.int32)
            nt[j], sc[j] = len(t), s
        tok, nt, sc = parallel.gather_sharded_results(tok, nt, sc, shards, len(audio_list))
        return [{'text': self._text(tok[i, :nt[i]]), 'score': float(sc[i])} for i in range(len(audio_list))]

    def predict_batch_deferred(self, audio_list, sample_rate=16000, timestamps=False, nbest=None):
        """ONE device pass over ``audio_list`` launched, nothing waited for: returns a function that -- when called -- waits for the
        pass and returns [{'text', 'score'}] in input order.  What a serving loop calls for the batch it has formed BEFORE it
        collects the previous one: staging, upload and launches of batch k + 1 then run under the device work of batch k, and
        consecutive calls alternate over the engine's two lanes (not with the prefix search on the GPU, whose launches already
        run beside the next pass).  The reference serves one request at a time (infer_server.py:48-71).
        ``timestamps=True``: every result gains ``'tokens'`` (see ``predict``); the pass stays deferred -- ``ctc_greedy`` aligns
        behind its collapse, the other decoders align when the function is called and their hypotheses are known.
        ``nbest=N``: every result gains ``'nbest'`` (see ``predict``); the n-best rows come back in the search's one packed copy."""
        nbest = self._nbest(nbest)
        eng = self.predictor.engine
        # (consecutive calls are the passes: the lane count of a call of several passes)
        lanes = pass_policy(self.configs.decoder, self._gpu_search(), 2, os.environ).lanes
        lane = self._deferred_turn % lanes
        self._deferred_turn += 1
        main = torch.cuda.current_stream(eng.device)
        stream = main
        if lane:
            stream = eng.side_stream(4)
            if not self._lane1_ordered:
                stream.wait_stream(main)             # (once: whatever the caller had queued before the first pass on lane 1)
                self._lane1_ordered = True
        began = self._begin_pass([self._load_audio(a, sample_rate) for a in audio_list])
        with eng.on_lane(lane, stream):
            return self._passes.launch(began, defer=True, timestamps=timestamps, nbest=nbest)

    def _run_sorted(self, audio_list, sample_rate, hints, which, decode_all_frames, batch_size, as_tokens, timestamps=False, nbest=None):
        """decode ``audio_list[i] for i in which`` in length-sorted device passes (cut shortest first, ties in input order -- the
        batches ``evaluate`` forms from a duration-sorted manifest); results in the order of ``which``.  ``pass_plan`` cuts the
        passes and says how they are pipelined: pass k is launched (its prefix search on a side stream), then pass k - depth + 1
        is collected and its audio dropped; consecutive passes alternate over the engine's lanes."""
        order = sorted(which, key=lambda i: hints[i]) if batch_size else list(which)      # (a list / tuple / number: sorted)
        cuts = pass_cuts(len(order), [hints[i] for i in order], batch_size)
        plan = pass_policy(self.configs.decoder, self._gpu_search(), len(cuts), os.environ)
        if plan.reverse:
            cuts.reverse()
        eng = self.predictor.engine
        main = torch.cuda.current_stream(eng.device)
        lane_streams = [main] + ([eng.side_stream(4)] if plan.lanes > 1 else [])
        for st in lane_streams[1:]:
            st.wait_stream(main)             # (once, before the first pass: whatever the caller queued comes first)
        got, pending, began = {}, [], {}

        def begin(k):
            lo, hi = cuts[k]
            began[k] = self._begin_pass([self._load_audio(audio_list[i], sample_rate) for i in order[lo:hi]])

        def collect(idx, fetch):
            for i, r in zip(idx, fetch()):
                got[i] = r
        for k, (lo, hi) in enumerate(cuts):
            if k not in began:
                begin(k)
            if plan.prep_ahead and k + 1 < len(cuts):
                # (the staging fills of the two passes started TOGETHER on eight threads, uploads behind them: measured slower --
                #  first encoder kernel at 1.4 instead of 1.15 ms, 17.5 vs 17.0 ms per call)
                begin(k + 1)
            lane = k % plan.lanes
            with eng.on_lane(lane, lane_streams[lane]):
                fetch = self._passes.launch(began.pop(k), decode_all_frames, as_tokens, defer=True, timestamps=timestamps,
                                           nbest=nbest)
            pending.append((order[lo:hi], fetch))
            if len(pending) >= plan.depth:
                collect(*pending.pop(0))
        if pending:
            for item in pending:
                collect(*item)
            for side in self._passes.search_streams() + lane_streams[1:]:
                main.wait_stream(side)
        return [got[i] for i in which]

    def evaluate(self, manifest, batch_size='auto', display_result=False, decode_all_frames=False, pass_padded=None):
        """Batched offline evaluation on the engine (the reference's batch > 1 consumer: MASRTrainer.evaluate,
        trainer.py:592-651): ``manifest`` is the reference's txt manifest (one JSON object per line with ``audio_filepath``
        and ``text``, data_utils/reader.py:32-40,55), utterances are sorted by duration, padded per batch and decoded with
        the configured decoder; returns (loss, error_rate) like the reference with loss = -1 (no CTC loss on this path) and
        error_rate = mean CER or WER over utterances (configs.metrics_type).  ``decode_all_frames=True`` reproduces the
        reference's decoding of the padded frames (trainer.py:340-344).  Under an initialised process group every rank reads
        the manifest, decodes its length-balanced shard and all ranks return the same error rate."""
        from masr_amd.utils.metrics import cer, wer
        items = []
        with open(manifest, 'r', encoding='utf-8') as f:
            for line in f:
                line = line.strip()
                if line:
                    d = json.loads(line)
                    items.append((d['audio_filepath'], d['text'], float(d.get('duration', 0.0))))
        items.sort(key=lambda it: it[2])
        metric = wer if self.configs.metrics_type == 'wer' else cer
        # manifest durations sort and shard the work: a rank opens only the files of its own shard, one pass at a time
        known = [it[2] for it in items] if all(it[2] > 0 for it in items) else None
        # batch_size='balanced': the pass budget in the unit of the lengths -- manifest durations are seconds
        if batch_size == 'balanced' and known is not None and pass_padded is None:
            pass_padded = self.pass_size() * 10.0
        results = self.predict_batch([it[0] for it in items], decode_all_frames=decode_all_frames, batch_size=batch_size,
                                     lengths=known, pass_padded=pass_padded)
        errors = []
        for (path, label, _), res in zip(items, results):
            err = metric(res['text'], label)
            errors.append(err)
            if display_result:
                logger.info(f'预测结果为：{res["text"]}')
                logger.info(f'实际标签为：{label}')
                logger.info(f'这条数据的{self.configs.metrics_type}：{round(err, 6)}，'
                            f'当前{self.configs.metrics_type}：{round(sum(errors) / len(errors), 6)}')
        return -1, (float(sum(errors) / len(errors)) if errors else -1)

    # ---- streaming ------------------------------------------------------------------------------------------------------------
    def predict_stream(self, audio_data, is_end=False, use_pun=False, is_itn=False, channels=1, samp_width=2,
                       sample_rate=16000, timestamps=False, nbest=None):
        """predict.py:237-343: feed raw PCM bytes / ndarray chunks, get the transcript so far ({'text','score'}), or None
        while fewer frames than one decoding window have arrived.  One session of a ``StreamPool``.
        ``timestamps=True``: the result gains ``'tokens'`` as in ``predict`` -- the transcript so far aligned against all frames of
        the utterance so far, in seconds since the utterance began (``StreamPool(timestamps=True)``: its cost is stated there).
        The flag of an utterance's first call decides for the utterance; change it after ``reset_stream()``.
        ``nbest=N`` (decoder ctc_beam_search): the result gains ``'nbest'`` as in ``predict``, read from the stream's
        device-resident search after every decoded chunk; the utterance's first call decides the value, as with ``timestamps``.
        ``decoder: attention_rescoring`` runs here only with ``attention_rescoring_decoder_conf.on_streams: 'rescore_at_end'``:
        the partial results are the CTC first pass's, and the call with ``is_end=True`` returns the rescored winner with the
        combined score (serving.py has the whole of it)."""
        nbest = self._nbest(nbest)
        if not self.configs.streaming:
            raise Exception(f"不支持改该模型流式识别，当前模型：{self.configs.use_model}，参数streaming为：{self.configs.streaming}")
        self._no_itn(is_itn)
        if self.configs.decoder == 'attention_rescoring':
            # (attention_rescoring_decoder_conf.on_streams: 'rescore_at_end' lifts it: the pool of one session rescores at is_end)
            from masr_amd.decoders.attention_rescoring import STREAM_REFUSAL, on_streams
            if on_streams(self.configs) != 'rescore_at_end':
                raise Exception(STREAM_REFUSAL)
        if self.configs.decoder == 'attention':
            from masr_amd.decoders.attention_decoder import STREAM_REFUSAL
            raise Exception(STREAM_REFUSAL)
        if self.configs.decoder == 'joint':
            from masr_amd.decoders.joint_decoder import STREAM_REFUSAL
            raise Exception(STREAM_REFUSAL)
        self._stream_pool_for(bool(timestamps), nbest)
        self._pool.feed(self._session, audio_data, is_end, channels=channels, samp_width=samp_width, sample_rate=sample_rate)
        return self._pool.step()[self._session]

    def _new_stream_pool(self, timestamps, nbest=None):
        from masr_amd.serving import StreamPool
        kw = dict(timestamps=True) if timestamps else {}
        if nbest is not None:
            kw['nbest'] = nbest
        return StreamPool(self, **kw)

    def _stream_pool_for(self, timestamps, nbest=None):
        """the single-session pool of ``predict_stream``: made on first use, and made anew at an utterance boundary when the new
        utterance's first call asks for the other kind; inside an utterance the flag cannot change"""
        if self._pool is not None and getattr(self, '_pool_nbest', None) != nbest and self._stream_running:
            from masr_amd._lib import MasrError
            raise MasrError(f'predict_stream: nbest={nbest} inside an utterance that began with nbest={self._pool_nbest}: the first '
                            f'call of an utterance decides; call reset_stream() first')
        if self._pool is not None and (self._pool_timestamps != timestamps or getattr(self, '_pool_nbest', None) != nbest):
            if self._stream_running:
                from masr_amd._lib import MasrError
                raise MasrError(f'predict_stream: timestamps={timestamps} inside an utterance that began with timestamps='
                                f'{self._pool_timestamps}: the first call of an utterance decides; call reset_stream() first')
            self._pool.close(self._session)
            self._pool.shutdown()
            self._pool = None
        if self._pool is None:
            self._pool = self._new_stream_pool(timestamps) if nbest is None else self._new_stream_pool(timestamps, nbest)
            self._pool_timestamps = timestamps
            self._pool_nbest = nbest
            self._session = self._pool.open()
        self._stream_running = True

    def reset_stream(self):
        """predict.py:346-353: forget the stream (caches, pending audio and frames, decoder history)."""
        self.predictor.reset_stream()
        self._stream_running = False
        if self._pool is not None:
            self._pool.reset(self._session)
