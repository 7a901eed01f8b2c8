"""Second-pass rescoring of the CTC n-best with the checkpoint's attention decoder (``decoder: 'attention_rescoring'``).

Every Conformer / Squeezeformer / Efficient-Conformer checkpoint is trained with two heads: the CTC head and a
BiTransformerDecoder (masr/model_utils/transformer/decoder.py; ``decoder_conf`` of the YAMLs).  The reference's predictor never
wired the second one up; its model holds the arithmetic, and the combination rule is WeNet's ``attention_rescoring``, which this
model family follows:

    sos = eos = vocab_size - 1
    att    = sum_i log_softmax(left_decoder([sos, h...]))_i [h..., eos]_i          (L + 1 positions)
    r_att  = the same from right_decoder on the reversed hypothesis
    score  = att * (1 - reverse_weight) + r_att * reverse_weight + ctc_weight * ctc_score

The n-best prefixes and their log-probabilities ``ctc_score`` come from the CTC prefix beam search without a language model:
``first_pass: 'host'`` (default) the host-thread search of libmasr_hip.so (masr_beam_search_batch_nbest) on the candidates the GPU
pruned; ``first_pass: 'gpu'`` masr_beam_search_gpu + masr_beam_nbest_gpu on the pass's stream over the device-resident
probabilities, only the n-best rows coming back (one pinned copy, one wait).  Both decoders run on the GPU
(masr_rescore), on the stream and the lane of the pass whose encoder output they read.  The winner is the highest score; an exact
tie goes to the hypothesis that ranked earlier in the search.

Streaming sessions (``predict_stream`` / ``serving.StreamPool``) are opt-in: ``attention_rescoring_decoder_conf.on_streams``.
``'refuse'`` (default, and what a configuration without the key gets): the decoder is refused on streams with ``STREAM_REFUSAL``.
``'rescore_at_end'``: the U2 serving mode.  Each session's first pass is the device-resident CTC prefix search of this block
(``_pruner.fork()``: no language model, the block's beam_size / cutoff_prob / cutoff_top_n) and its partial results are that
search's best prefix; every chunk step also hands out its encoder rows (masr_encode_chunk_enc), which the pool keeps in one
device row pool; in the step that ends an utterance the n-best of the live search is rescored against ALL kept frames of the
session through the row table (masr_rescore_rows: nothing is gathered into a dense block), and the result is the winner with the
combined score.  ``first_pass`` has no meaning there: a stream's first pass is always the device-resident search.

Left out: language-model fusion in the first pass."""
import ctypes as C

import numpy as np
import torch

from masr_amd import _lib
from masr_amd._lib import check

STREAM_REFUSAL = ("decoder='attention_rescoring' does not run on streaming sessions (predict_stream / StreamPool): rescoring at the "
                  "end of a stream would need the whole session's encoder output kept, which is left out; use predict / "
                  "predict_batch, or ctc_greedy / ctc_beam_search for streams.  "
                  "attention_rescoring_decoder_conf.on_streams: 'rescore_at_end' keeps it and rescores when the utterance ends")

BEAM_MIN, BEAM_MAX = 1, 64
FIRST_PASSES = ('host', 'gpu')      # where the first pass's prefix search runs
ON_STREAMS = ('refuse', 'rescore_at_end')      # attention_rescoring_decoder_conf.on_streams


def check_on_streams(value):
    """a value of ``attention_rescoring_decoder_conf.on_streams`` -> itself; one outside ``ON_STREAMS`` is refused by name"""
    if value not in ON_STREAMS:
        raise _lib.MasrError(f'attention_rescoring_decoder_conf.on_streams={value!r} is not supported: one of {ON_STREAMS}')
    return value


def on_streams(configs):
    """``attention_rescoring_decoder_conf.on_streams`` of a predictor's configuration: 'refuse' where the block or the key is
    absent"""
    conf = configs.get('attention_rescoring_decoder_conf', None) or {}
    return check_on_streams(dict(conf).get('on_streams', 'refuse'))


def validate_rescoring_conf(conf, model_conf=None, r_num_blocks=None):
    """``attention_rescoring_decoder_conf`` -> dict(beam_size, ctc_weight, reverse_weight, cutoff_prob, cutoff_top_n, num_processes).
    ``beam_size`` 1 .. 64 (default 10), ``ctc_weight`` (default 0.5), ``reverse_weight`` (default ``model_conf.reverse_weight``,
    0 without one), ``cutoff_prob`` / ``cutoff_top_n`` as in the CTC search block (0.99 / 40).  ``r_num_blocks`` given: a positive
    ``reverse_weight`` needs a right-to-left decoder.  ``on_streams`` ('refuse' / 'rescore_at_end') and ``first_pass`` are passed
    on only when named."""
    conf = dict(conf or {})
    known = ('beam_size', 'ctc_weight', 'reverse_weight', 'cutoff_prob', 'cutoff_top_n', 'num_processes', 'first_pass', 'on_streams')
    for k in conf:
        if k not in known:
            raise _lib.MasrError(f'attention_rescoring_decoder_conf.{k} is not a known key (known: {known})')
    beam = conf.get('beam_size', 10)
    if isinstance(beam, bool) or not isinstance(beam, int) or not BEAM_MIN <= beam <= BEAM_MAX:
        raise _lib.MasrError(f'attention_rescoring_decoder_conf.beam_size={beam!r} is not supported: an integer from {BEAM_MIN} to '
                             f'{BEAM_MAX}')

    def number(key, default):
        v = conf.get(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
            raise _lib.MasrError(f'attention_rescoring_decoder_conf.{key}={v!r} is not a number')
        return float(v)
    rw_default = 0.0 if model_conf is None else dict(model_conf).get('reverse_weight', 0.0)
    out = {'beam_size': beam, 'ctc_weight': number('ctc_weight', 0.5), 'reverse_weight': number('reverse_weight', rw_default),
           'cutoff_prob': number('cutoff_prob', 0.99), 'num_processes': int(conf.get('num_processes', 10))}
    if not 0.0 <= out['reverse_weight'] <= 1.0:
        raise _lib.MasrError(f'attention_rescoring_decoder_conf.reverse_weight={out["reverse_weight"]!r} is not in [0, 1]')
    top_n = conf.get('cutoff_top_n', 40)
    if isinstance(top_n, bool) or not isinstance(top_n, int) or top_n < 1:
        raise _lib.MasrError(f'attention_rescoring_decoder_conf.cutoff_top_n={top_n!r} is not supported: a positive integer')
    out['cutoff_top_n'] = top_n
    if 'first_pass' in conf:            # (not named: the decoder's own default, 'host' -- the path and the bits it was)
        if conf['first_pass'] not in FIRST_PASSES:
            raise _lib.MasrError(f'attention_rescoring_decoder_conf.first_pass={conf["first_pass"]!r} is not supported: one of '
                                 f'{FIRST_PASSES}')
        out['first_pass'] = conf['first_pass']
    if 'on_streams' in conf:            # (not named: 'refuse', what streams always got)
        out['on_streams'] = check_on_streams(conf['on_streams'])
    if r_num_blocks is not None and out['reverse_weight'] > 0 and r_num_blocks == 0:
        raise _lib.MasrError(f'attention_rescoring_decoder_conf.reverse_weight={out["reverse_weight"]} needs the right-to-left '
                             f'decoder, and this checkpoint has none (decoder_conf.r_num_blocks: 0)')
    return out


def combine(att, r_att, ctc_score, ctc_weight, reverse_weight):
    """the combined score of WeNet's attention_rescoring, evaluated in float64 on the float32 inputs"""
    att, r_att, ctc_score = (np.asarray(a, np.float64) for a in (att, r_att, ctc_score))
    return att * (1.0 - reverse_weight) + r_att * reverse_weight + ctc_weight * ctc_score


def pick(scores, count=None):
    """index of the winner among the first ``count`` hypotheses: the highest score, an exact tie to the earlier rank"""
    s = np.asarray(scores, np.float64)[:count]
    return int(np.argmax(s))         # (argmax returns the FIRST maximum)


def build_table(nbest, max_pos=None):
    """[[token lists of utterance b] ...] -> (hyps [B, N, Lmax] int32 zero-padded, lens [B, N] int32, count [B]); utterances with
    fewer than N hypotheses get empty ones (never selected).  ``max_pos``: hypotheses longer than ``max_pos - 1`` are refused."""
    B = len(nbest)
    N = max(1, max((len(h) for h in nbest), default=1))
    Lmax = max(1, max((len(t) for h in nbest for t in h), default=1))
    if max_pos is not None and Lmax > max_pos - 1:
        raise _lib.MasrError(f'attention_rescoring: a hypothesis of {Lmax} tokens is longer than max_pos - 1 = {max_pos - 1}: the '
                             f'decoder has no positional rows for it')
    hyps, lens = np.zeros((B, N, Lmax), np.int32), np.zeros((B, N), np.int32)
    for b, h in enumerate(nbest):
        for n, t in enumerate(h):
            hyps[b, n, :len(t)] = t
            lens[b, n] = len(t)
    return hyps, lens, np.array([len(h) for h in nbest], np.int32)


class AttentionRescoringDecoder:
    def __init__(self, vocab_list, beam_size=10, ctc_weight=0.5, reverse_weight=0.0, cutoff_prob=0.99, cutoff_top_n=40,
                 num_processes=10, blank_id=0, first_pass='host', on_streams='refuse'):
        from masr_amd.decoders.beam_search_decoder import BeamSearchDecoder
        self.vocab_list = vocab_list
        self.beam_size, self.ctc_weight, self.reverse_weight = int(beam_size), float(ctc_weight), float(reverse_weight)
        self.num_processes, self.blank_id = int(num_processes), int(blank_id)
        # the first pass's vocabulary pruning (masr_ctc_topk on the GPU) is the CTC search's own, without a language model
        self._pruner = BeamSearchDecoder(alpha=0, beta=0, beam_size=self.beam_size, cutoff_prob=cutoff_prob, cutoff_top_n=cutoff_top_n,
                                         vocab_list=vocab_list, num_processes=num_processes, blank_id=blank_id,
                                         language_model_path=None)
        self._lib = _lib.lib()
        if first_pass not in FIRST_PASSES:
            raise _lib.MasrError(f'attention_rescoring_decoder_conf.first_pass={first_pass!r} is not supported: one of {FIRST_PASSES}')
        if first_pass == 'gpu' and not self._pruner.gpu_search_supported(1, len(vocab_list)):
            raise _lib.MasrError(f"attention_rescoring_decoder_conf.first_pass='gpu' with beam_size={self.beam_size}, cutoff_top_n="
                                 f"{cutoff_top_n} is beyond the GPU prefix search (beam_size 2 .. 512, cutoff_top_n <= 64, its "
                                 f"tables within 160 KB of LDS); use first_pass='host'")
        self.first_pass = first_pass
        self.on_streams = check_on_streams(on_streams)

    def _text(self, toks):
        return ''.join(self.vocab_list[t] for t in toks).replace('<space>', ' ')

    def nbest(self, probs, frames):
        """first pass: probs [B, Ts, V] (device tensor or array), ``frames`` [B] valid rows -> per utterance the (up to)
        ``beam_size`` best prefixes [(token ids, log-probability)], best first"""
        B, Ts, V = probs.shape
        frames = np.ascontiguousarray(frames, np.int32)
        if self.first_pass == 'gpu':
            return self._nbest_gpu(probs, frames)
        idx, logp, cnt, _, K = self._pruner._candidates(probs.reshape(B * Ts, V))
        N, max_len = self.beam_size, max(Ts, 1)
        toks = np.zeros((B, N, max_len), np.int32)
        lens, scores, count = np.zeros((B, N), np.int32), np.zeros((B, N), np.float32), np.zeros(B, np.int32)
        as_p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = self._lib.masr_beam_search_batch_nbest(as_p(idx), as_p(logp), as_p(cnt), as_p(frames), B, Ts, K, self.beam_size,
                                                    self.blank_id, self.num_processes, N, as_p(toks), max_len, as_p(lens),
                                                    as_p(scores), as_p(count))
        if rc != 0:
            raise _lib.MasrError('masr_beam_search_batch_nbest failed')
        return [[(toks[b, n, :lens[b, n]].tolist(), float(scores[b, n])) for n in range(count[b])] for b in range(B)]

    def _nbest_gpu(self, probs, frames):
        """``first_pass: 'gpu'``: pruning, the LM-free masr_beam_search_gpu and masr_beam_nbest_gpu on the current stream; only the
        packed n-best rows [B, N, max_len + 2] + counts come back: one pinned copy behind them, one wait"""
        from masr_amd import runtime
        dec = self._pruner
        B, Ts, V = probs.shape
        if not torch.is_tensor(probs):
            probs = torch.as_tensor(np.asarray(probs), dtype=torch.float32)
        eng = runtime.aux_engine(probs.device if probs.is_cuda else None)
        cand = dec._candidates(probs.reshape(B * Ts, V), to_host=False)
        _, max_len, keep = dec._search_gpu(eng, cand, frames, B, Ts, pack=False)
        flat, keep_n = dec._nbest_gpu(eng, B, max_len, self.beam_size)
        host = dec._pinned_out(flat.numel())
        host[:flat.numel()].copy_(flat, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
        try:
            return dec._unpacked_nbest(host[:flat.numel()].numpy(), B, self.beam_size, max_len, True)
        finally:
            dec.__dict__.setdefault('_pin_free', []).append(host)

    def rescore_launch(self, eng, enc, enc_lens, nbest):
        """second pass QUEUED on ``eng``'s current stream and active lane, nothing waited for: the hypothesis table goes up through
        pinned memory, both decoders run (masr_rescore), att / r_att come back into a pinned buffer behind an event.  ``enc``
        [B, T', d] device, ``enc_lens`` [B] int32 device, ``nbest`` from ``nbest()`` -> a function that waits for that event only
        and returns, per utterance, (token ids, combined score, index of the winner, (att, r_att, combined) arrays)"""
        hyps, lens, count = build_table([[t for t, _ in h] for h in nbest], eng.max_pos)
        with_right = self.reverse_weight > 0
        att, r_att = eng.rescore(enc, enc_lens, eng.to_device(hyps).view(hyps.shape), eng.to_device(lens).view(lens.shape),
                                 with_right=with_right)
        host = torch.empty(2, *att.shape, dtype=torch.float32, pin_memory=True)
        host[0].copy_(att, non_blocking=True)
        host[1].copy_(r_att, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        collect_keeps = (enc, enc_lens, att, r_att)      # alive until the copies have run (the closure below holds them)

        def collect(_keep=collect_keeps):
            done.synchronize()
            both = host.numpy()
            out = []
            for b, h in enumerate(nbest):
                n = int(count[b])
                ctc = np.array([s for _, s in h], np.float32)
                total = combine(both[0, b, :n], both[1, b, :n], ctc, self.ctc_weight, self.reverse_weight)
                w = pick(total, n)
                out.append((h[w][0], float(total[w]), w, (both[0, b, :n].copy(), both[1, b, :n].copy(), total)))
            return out
        return collect

    def rescore(self, eng, enc, enc_lens, nbest):
        """``rescore_launch`` and its results at once"""
        return self.rescore_launch(eng, enc, enc_lens, nbest)()

    def decode_pass(self, eng, enc, enc_lens, probs, frames, want_tokens=False):
        """one device pass: the CTC n-best of ``probs`` (the host waits for the pruned candidates and searches them), then the
        second pass over ``enc`` queued -> a function that returns [(score, text)] (or [(token ids, score)]) when called"""
        collect = self.rescore_launch(eng, enc, enc_lens, self.nbest(probs, frames))

        def fetch():
            res = collect()
            if want_tokens:
                return [(toks, score) for toks, score, _, _ in res]
            return [(score, self._text(toks)) for toks, score, _, _ in res]
        return fetch
