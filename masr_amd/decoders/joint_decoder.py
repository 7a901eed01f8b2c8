"""Joint CTC / attention beam search (``decoder: 'joint'``).

The search of ``decoder: 'attention'`` (decoders/attention_decoder.py: the left decoder, one new row per hypothesis and step, its
tie rules, step limit and early stop) ranked by a key that ties every hypothesis to the audio: the CTC head's prefix probability
of its tokens over the utterance's frames, and a length bonus (Watanabe et al.'s joint CTC / attention decoding; ESPnet's default,
the ``ctc_weight`` of WeNet's attention mode).  The whole search runs on the GPU (masr_joint_decode; include/masr_hip.h holds
the rules).

    A   = the sum of the hypothesis' attention log-probabilities        psi = the log of its CTC prefix probability
    n   = its tokens other than eos                                      J   = ((1 - ctc_weight) A + ctc_weight psi) + length_bonus n
    step: the top ``ctc_candidates`` of every live hypothesis by attention log-probability, psi of each, then the top ``beam_size``
          of the utterance's keys J; ties go to the smaller token id, then to the smaller parent_rank * ctc_candidates + candidate_rank
    text: the best hypothesis' tokens; score: its J (``last_parts`` keeps A and psi of the latest pass beside it)

Shallow fusion with an n-gram language model (``language_model_path`` + ``lm_weight``; ESPnet's ``lm_weight``): a fourth part
Lm, the float32 running sum of ln P_LM(token | the hypothesis' last max_order - 1 tokens) -- ``LanguageModel.cond_log_prob`` bit
for bit, eos scored as the model's ``</s>`` -- and the key

    J = (((1 - ctc_weight) A + ctc_weight psi) + lm_weight Lm) + length_bonus n

over the same ``ctc_candidates`` attention candidates (masr_joint_decode_lm; ``last_lm`` keeps Lm of the latest pass).  With
``lm_weight`` 0 nothing of the model is loaded or launched and the search is the one above bit for bit.  Character-based ARPA
models only, as on the GPU CTC search.

Left out: the right-to-left decoder and streaming sessions."""
import math
import os

import torch

from masr_amd import _lib

STREAM_REFUSAL = ("decoder='joint' does not run on streaming sessions (predict_stream / StreamPool): the joint search runs over the "
                  "whole utterance's encoder output and CTC posteriors, which a session does not keep; use predict / "
                  "predict_batch, or ctc_greedy / ctc_beam_search for streams")
DS2_REFUSAL = ("decoder='joint' is not available for use_model deepspeech2: it has no attention decoder (its decoder.* tensors "
               "are the CTC head)")
DECODE_REFUSAL = ("decoder='joint' needs the encoder output of the utterance beside its probabilities: use predict / "
                  "predict_batch")
NBEST_REFUSAL = ("nbest={nbest!r} with decoder='joint': nbest returns the prefixes of the CTC prefix beam search "
                 "(decoder='ctc_beam_search'); the hypotheses of the joint search are not those and are not returned")

BEAM_MIN, BEAM_MAX = 1, 64
CANDIDATES_MAX = 64
DEFAULT_CTC_WEIGHT = 0.3
DEFAULT_LM_WEIGHT = 0.3         # with a language_model_path: ESPnet's usual AIShell value (a design choice, not a measurement)
WORD_LM_REFUSAL = ("joint_decoder_conf.language_model_path={path!r} is a word-based language model (an LM word longer than one "
                   "token): the joint search scores vocabulary tokens; word-based models run in decoder='ctc_beam_search' only")


def _real(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise _lib.MasrError(f'joint_decoder_conf.{name}={v!r} is not a number')
    return float(v)


def validate_joint_conf(conf, model_conf=None, vocab_size=None):
    """``joint_decoder_conf`` -> dict(beam_size, max_len, ctc_weight, length_bonus, ctc_candidates).  ``beam_size`` 1 .. 64 and at
    most the vocabulary (default 10); ``max_len`` >= 0 (default 0: no limit besides the utterance's encoder frames); ``ctc_weight``
    a real in [0, 1) (default: ``model_conf.ctc_weight`` when that lies in [0, 1), otherwise 0.3); ``length_bonus`` any finite real
    (default 0.0); ``ctc_candidates`` from beam_size to min(64, vocabulary) (default min(2 beam_size, 64, vocabulary)).  Unknown
    keys are refused by name.

    ``language_model_path`` (a string: an ARPA file, or None) and ``lm_weight`` (a finite real >= 0; default 0.3 with a path, 0.0
    without): a configuration that names either comes back with both beside the five keys above -- ``language_model_path`` None
    where ``lm_weight`` is 0, since nothing is loaded then.  ``lm_weight`` > 0 without a path is refused by name."""
    conf = dict(conf or {})
    known = ('beam_size', 'max_len', 'ctc_weight', 'length_bonus', 'ctc_candidates', 'language_model_path', 'lm_weight')
    for k in conf:
        if k not in known:
            raise _lib.MasrError(f'joint_decoder_conf.{k} is not a known key (known: {known})')
    beam = conf.get('beam_size', 10)
    if isinstance(beam, bool) or not isinstance(beam, int) or not BEAM_MIN <= beam <= BEAM_MAX:
        raise _lib.MasrError(f'joint_decoder_conf.beam_size={beam!r} is not supported: an integer from {BEAM_MIN} to {BEAM_MAX}')
    if vocab_size is not None and beam > vocab_size:
        raise _lib.MasrError(f'joint_decoder_conf.beam_size={beam} exceeds the vocabulary of {vocab_size}')
    max_len = conf.get('max_len', 0)
    if isinstance(max_len, bool) or not isinstance(max_len, int) or max_len < 0:
        raise _lib.MasrError(f'joint_decoder_conf.max_len={max_len!r} is not supported: an integer, 0 (no limit) or more')
    if 'ctc_weight' in conf:
        weight = _real('ctc_weight', conf['ctc_weight'])
        if not 0.0 <= weight < 1.0:
            raise _lib.MasrError(f'joint_decoder_conf.ctc_weight={conf["ctc_weight"]!r} is not in [0, 1)')
    else:
        weight = (model_conf or {}).get('ctc_weight', None)
        ok = not isinstance(weight, bool) and isinstance(weight, (int, float)) and 0.0 <= weight < 1.0
        weight = float(weight) if ok else DEFAULT_CTC_WEIGHT
    bonus = _real('length_bonus', conf.get('length_bonus', 0.0))
    if not math.isfinite(bonus):
        raise _lib.MasrError(f'joint_decoder_conf.length_bonus={conf["length_bonus"]!r} is not finite')
    top = CANDIDATES_MAX if vocab_size is None else min(CANDIDATES_MAX, vocab_size)
    cands = conf.get('ctc_candidates', min(2 * beam, top))
    if isinstance(cands, bool) or not isinstance(cands, int) or not beam <= cands <= top:
        raise _lib.MasrError(f'joint_decoder_conf.ctc_candidates={cands!r} is not supported: an integer from beam_size = {beam} to '
                             f'{top} (min(64, vocabulary))')
    out = {'beam_size': beam, 'max_len': max_len, 'ctc_weight': weight, 'length_bonus': bonus, 'ctc_candidates': cands}
    # (only then: a configuration without them returns the five keys it always did, which callers compare as a whole dict)
    if 'language_model_path' in conf or 'lm_weight' in conf:
        path = conf.get('language_model_path', None)
        if path is not None and (not isinstance(path, (str, os.PathLike)) or not str(path)):
            raise _lib.MasrError(f'joint_decoder_conf.language_model_path={path!r} is not a file path (a string, or None)')
        lm_weight = _real('lm_weight', conf.get('lm_weight', DEFAULT_LM_WEIGHT if path is not None else 0.0))
        if not math.isfinite(lm_weight) or lm_weight < 0.0:
            raise _lib.MasrError(f'joint_decoder_conf.lm_weight={conf["lm_weight"]!r} is not a finite number >= 0')
        if lm_weight > 0.0 and path is None:
            raise _lib.MasrError(f'joint_decoder_conf.lm_weight={lm_weight} needs joint_decoder_conf.language_model_path (an ARPA '
                                 f'n-gram model); without one lm_weight is 0')
        out.update(language_model_path=str(path) if path is not None and lm_weight > 0.0 else None, lm_weight=lm_weight)
    return out


def load_language_model(path, vocab_list):
    """the ARPA model of ``joint_decoder_conf.language_model_path`` with the loader and the missing-file behaviour of
    ``ctc_beam_search``'s ``language_model_path`` (decoders/beam_search_decoder.py); a word-based model is refused by name"""
    assert os.path.exists(path), f'语言模型不存在：{path}'
    from masr_amd.decoders.lm_scorer import LanguageModel
    lm = LanguageModel(path, vocab_list)
    if not lm.is_character_based:
        lm.close()
        raise _lib.MasrError(WORD_LM_REFUSAL.format(path=str(path)))
    return lm


class JointDecoder:
    def __init__(self, vocab_list, beam_size=10, max_len=0, ctc_weight=DEFAULT_CTC_WEIGHT, length_bonus=0.0, ctc_candidates=None,
                 language_model=None, lm_weight=0.0):
        """``language_model``: a ``LanguageModel`` loaded for ``vocab_list`` (``load_language_model``) or None; it is used when
        ``lm_weight`` > 0, which needs one"""
        lm_weight = _real('lm_weight', lm_weight)
        if not math.isfinite(lm_weight) or lm_weight < 0.0:
            raise _lib.MasrError(f'joint_decoder_conf.lm_weight={lm_weight!r} is not a finite number >= 0')
        if lm_weight > 0.0 and language_model is None:
            raise _lib.MasrError(f'joint_decoder_conf.lm_weight={lm_weight} needs a language model (language_model_path)')
        if language_model is not None and not language_model.is_character_based:
            raise _lib.MasrError(WORD_LM_REFUSAL.format(path=str(language_model.path)))
        if language_model is not None and language_model.vocab_size != len(vocab_list):
            raise _lib.MasrError(f'the language model was loaded for a vocabulary of {language_model.vocab_size} tokens, the '
                                 f'decoder has {len(vocab_list)}')
        self.language_model, self.lm_weight = language_model, lm_weight
        conf = {'beam_size': beam_size, 'max_len': max_len, 'ctc_weight': ctc_weight, 'length_bonus': length_bonus}
        if ctc_candidates is not None:
            conf['ctc_candidates'] = ctc_candidates
        conf = validate_joint_conf(conf, None, len(vocab_list))
        self.vocab_list = vocab_list
        self.beam_size, self.max_len = conf['beam_size'], conf['max_len']
        self.ctc_weight, self.length_bonus, self.ctc_candidates = conf['ctc_weight'], conf['length_bonus'], conf['ctc_candidates']
        self.last_steps = 0             # steps the latest search launched (diagnostics)
        self.last_parts = None          # per utterance [(A, psi)] of the N ranks of the latest COLLECTED pass
        self.last_lm = None             # per utterance [Lm] of the N ranks of that pass (zeros without a language model)

    def _text(self, toks):
        return ''.join(self.vocab_list[t] for t in toks).replace('<space>', ' ')

    def search_launch(self, eng, enc, enc_lens, probs):
        """the search QUEUED on ``eng``'s current stream and active lane (the host waits at the end polls only); the N hypotheses
        come back into pinned memory behind an event.  ``enc`` [B, T', d], ``enc_lens`` [B] int32, ``probs`` [B, T', V] the CTC
        head's posteriors of the same pass (device) -> a function that waits for that event and returns per utterance
        [(token ids, J)] of the N ranks, best first, and leaves their (A, psi) in ``last_parts`` and their Lm in ``last_lm``"""
        if self.lm_weight > 0.0:
            tokens, lens, scores, att, psi, lm, steps = eng.joint_decode_lm(
                enc, enc_lens, probs, self.language_model, self.lm_weight, self.beam_size, self.ctc_candidates, self.ctc_weight,
                self.length_bonus, self.max_len)
            parts = (scores, att, psi, lm)
        else:
            tokens, lens, scores, att, psi, steps = eng.joint_decode(enc, enc_lens, probs, self.beam_size, self.ctc_candidates,
                                                                     self.ctc_weight, self.length_bonus, self.max_len)
            parts = (scores, att, psi)
        B, N, Lcap = tokens.shape
        host_t = torch.empty(B, N, Lcap, dtype=torch.int32, pin_memory=True)
        host_l = torch.empty(B, N, dtype=torch.int32, pin_memory=True)
        host_s = torch.zeros(4, B, N, dtype=torch.float32, pin_memory=True)      # (row 3, Lm, stays 0 without a model)
        host_t.copy_(tokens, non_blocking=True)
        host_l.copy_(lens, non_blocking=True)
        for i, src in enumerate(parts):
            host_s[i].copy_(src, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        keeps = (enc, enc_lens, probs, tokens, lens) + parts      # alive until the copies have run
        self.last_steps = steps

        def collect(_keep=keeps):
            done.synchronize()
            t, l, s = host_t.numpy(), host_l.numpy(), host_s.numpy()
            self.last_parts = [[(float(s[1, b, n]), float(s[2, b, n])) for n in range(N)] for b in range(B)]
            self.last_lm = [[float(s[3, b, n]) for n in range(N)] for b in range(B)]
            return [[(t[b, n, :l[b, n]].tolist(), float(s[0, b, n])) for n in range(N)] for b in range(B)]
        return collect

    def decode_pass(self, eng, enc, enc_lens, probs, want_tokens=False):
        """one device pass: the search over ``enc`` and ``probs`` queued -> a function that returns [(score, text)] (or
        [(token ids, score)]) of the best hypothesis of every utterance when called"""
        collect = self.search_launch(eng, enc, enc_lens, probs)

        def fetch():
            best = [h[0] for h in collect()]
            if want_tokens:
                return best
            return [(score, self._text(toks)) for toks, score in best]
        return fetch
