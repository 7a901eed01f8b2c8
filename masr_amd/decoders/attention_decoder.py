"""Autoregressive beam search with the checkpoint's attention decoder (``decoder: 'attention'``).

The fourth decoding mode of this model family (WeNet's U2 recipe): left-to-right beam search driven by the LEFT half of the
BiTransformerDecoder alone, through what the reference's ``TransformerDecoder.forward_one_step`` computes
(masr/model_utils/transformer/decoder.py:233-270).  The whole search runs on the GPU (masr_attention_decode): one new decoder row
per hypothesis and step over a per-layer k | v cache, log-softmax + top-N and the beam merge in kernels of their own.  It never
passes through the CTC prefix search.

    sos = eos = vocab_size - 1;  N = beam_size
    start: N hypotheses [sos] with scores [0, -inf, ...]
    step : top N of every hypothesis' next-token log-probabilities (finished ones offer (0, eos), (-inf, eos), ...), then the top N
           of the utterance's N x N sums; ties go to the smaller token id, then to the smaller parent_rank * N + candidate_rank
    stop : after min(encoder frames of the utterance, max_len if positive, max_pos - 1) steps, or when all N end in eos
    text : the best hypothesis' tokens behind sos up to its first eos; score: its summed log-probability

Left out: the right-to-left decoder and streaming sessions.  Joint CTC scoring and a length bonus are ``decoder: 'joint'``
(decoders/joint_decoder.py)."""
import torch

from masr_amd import _lib

STREAM_REFUSAL = ("decoder='attention' does not run on streaming sessions (predict_stream / StreamPool): the attention decoder "
                  "searches over the whole utterance's encoder output, which a session does not keep; use predict / predict_batch, "
                  "or ctc_greedy / ctc_beam_search for streams")
DS2_REFUSAL = ("decoder='attention' is not available for use_model deepspeech2: it has no attention decoder (its decoder.* tensors "
               "are the CTC head)")
DECODE_REFUSAL = ("decoder='attention' needs the encoder output of the utterance, not only its probabilities: use predict / "
                  "predict_batch")

BEAM_MIN, BEAM_MAX = 1, 64


def validate_attention_conf(conf, vocab_size=None):
    """``attention_decoder_conf`` -> dict(beam_size, max_len): ``beam_size`` 1 .. 64 and at most the vocabulary (default 10),
    ``max_len`` >= 0 (default 0: no limit besides the utterance's encoder frames).  Unknown keys are refused by name."""
    conf = dict(conf or {})
    known = ('beam_size', 'max_len')
    for k in conf:
        if k not in known:
            raise _lib.MasrError(f'attention_decoder_conf.{k} is not a known key (known: {known})')
    beam = conf.get('beam_size', 10)
    if isinstance(beam, bool) or not isinstance(beam, int) or not BEAM_MIN <= beam <= BEAM_MAX:
        raise _lib.MasrError(f'attention_decoder_conf.beam_size={beam!r} is not supported: an integer from {BEAM_MIN} to {BEAM_MAX}')
    if vocab_size is not None and beam > vocab_size:
        raise _lib.MasrError(f'attention_decoder_conf.beam_size={beam} exceeds the vocabulary of {vocab_size}')
    max_len = conf.get('max_len', 0)
    if isinstance(max_len, bool) or not isinstance(max_len, int) or max_len < 0:
        raise _lib.MasrError(f'attention_decoder_conf.max_len={max_len!r} is not supported: an integer, 0 (no limit) or more')
    return {'beam_size': beam, 'max_len': max_len}


class AttentionDecoder:
    def __init__(self, vocab_list, beam_size=10, max_len=0):
        conf = validate_attention_conf({'beam_size': beam_size, 'max_len': max_len}, len(vocab_list))
        self.vocab_list = vocab_list
        self.beam_size, self.max_len = conf['beam_size'], conf['max_len']
        self.last_steps = 0             # steps the latest search launched (diagnostics)

    def _text(self, toks):
        return ''.join(self.vocab_list[t] for t in toks).replace('<space>', ' ')

    def search_launch(self, eng, enc, enc_lens):
        """the search QUEUED on ``eng``'s current stream and active lane (the host waits at the end polls only); the N hypotheses
        come back into pinned memory behind an event.  ``enc`` [B, T', d], ``enc_lens`` [B] int32 (device) -> a function that waits
        for that event and returns per utterance [(token ids, score)] of the N ranks, best first"""
        tokens, lens, scores, steps = eng.attention_decode(enc, enc_lens, self.beam_size, self.max_len)
        B, N, Lcap = tokens.shape
        host_t = torch.empty(B, N, Lcap, dtype=torch.int32, pin_memory=True)
        host_l = torch.empty(B, N, dtype=torch.int32, pin_memory=True)
        host_s = torch.empty(B, N, dtype=torch.float32, pin_memory=True)
        host_t.copy_(tokens, non_blocking=True)
        host_l.copy_(lens, non_blocking=True)
        host_s.copy_(scores, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        keeps = (enc, enc_lens, tokens, lens, scores)      # alive until the copies have run
        self.last_steps = steps

        def collect(_keep=keeps):
            done.synchronize()
            t, l, s = host_t.numpy(), host_l.numpy(), host_s.numpy()
            return [[(t[b, n, :l[b, n]].tolist(), float(s[b, n])) for n in range(N)] for b in range(B)]
        return collect

    def decode_pass(self, eng, enc, enc_lens, want_tokens=False):
        """one device pass: the search over ``enc`` queued -> a function that returns [(score, text)] (or [(token ids, score)]) of
        the best hypothesis of every utterance when called"""
        collect = self.search_launch(eng, enc, enc_lens)

        def fetch():
            best = [h[0] for h in collect()]
            if want_tokens:
                return best
            return [(score, self._text(toks)) for toks, score in best]
        return fetch

