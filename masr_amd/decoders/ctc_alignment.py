"""Token timestamps: host side of the CTC forced alignment (``timestamps=True`` of ``MASRPredictor.predict`` / ``predict_batch`` /
``predict_batch_deferred`` / ``predict_long`` / ``predict_stream`` and of ``serving.StreamPool``).

Every model family has a CTC head, so every hypothesis -- whichever decoder produced it, the attention decoders included -- can be
aligned against the CTC posteriors of its own utterance: masr_ctc_align (csrc/ctc_align.hip, include/masr_hip.h) finds the Viterbi
path through the trellis of the hypothesis on the GPU and returns, per token, the first and last encoder frame of its state and its
largest log-probability over those frames.  This module turns those frames into seconds; it needs neither the library nor a GPU.

Streaming sessions (``StreamPool(predictor, timestamps=True)``) keep the CTC head's rows of every session in one device-resident row
pool and align the hypothesis so far against all frames so far on every step: masr_ctc_align_rows, the same kernel reading its
frames through a row table.  The functions below serve both: a partial stream is an utterance whose ``duration_s`` is the audio fed
so far, and its times count from the session's ``open()`` / ``reset()``.

Tie rule of the path (part of the contract, restated by tests/ctc_align_ref.py): predecessors in the order stay, s - 1, s - 2, a
later one only if strictly greater; at the end the last blank wins a tie against the last token.  ``status`` 0 = aligned, 1 = the
trellis has no path (fewer frames than tokens + adjacent repeats), 2 = an argument out of range.

Left out: ``ShardedStreamPool`` and the websocket server (streaming timestamps exist on ``StreamPool`` / ``predict_stream`` only),
second passes on streams, the sharded (``distributed``) path, ``evaluate``, word grouping and punctuation."""
import math

import numpy as np

HOP_SAMPLES = 160           # feature frames are 10 ms apart at the model's 16 kHz (fbank, MFCC and linear alike)
SENTINEL = -1.0e30          # MASR_ALIGN_NEG of include/masr_hip.h: "unreachable" in the trellis
MAX_TOKENS = 1024           # MASR_ALIGN_MAX_TOKENS: the longest hypothesis the kernel's LDS rows hold

DISTRIBUTED_REFUSAL = ("timestamps=True does not run on the sharded path (distributed=True): the all-gather carries token ids and "
                       "scores only; call predict_batch with distributed=False on every rank's own utterances")


def frames_to_times(start, end, peak, reduction, hop_samples, sample_rate, duration_s, vocab):
    """per-token frames of ONE utterance -> [{'token', 'start', 'end', 'score'}] in time order.

    ``start`` / ``end`` [L]: first / last encoder frame (inclusive) of each token, ``peak`` [L]: its largest log-probability there,
    ``vocab`` [L]: the tokens' strings.  Encoder frame t begins at feature frame ``reduction`` * t, i.e. at sample
    ``reduction * hop_samples * t``:
        start = start_frame * reduction * hop / sample_rate
        end   = min((end_frame + 1) * reduction * hop / sample_rate, duration_s)
        score = exp(peak)
    in seconds of the utterance (``sample_rate`` is the model's, at which the frames were cut: audio given at another rate gets
    the same times)."""
    step = float(reduction) * float(hop_samples) / float(sample_rate)
    out = []
    for tok, s, e, p in zip(vocab, start, end, peak):
        out.append({'token': tok, 'start': int(s) * step, 'end': min((int(e) + 1) * step, float(duration_s)),
                    'score': math.exp(float(p))})
    return out


def shift_tokens(tokens, offset_s):
    """the tokens of a VAD segment moved to the recording's clock (``predict_long``): a copy with ``offset_s`` added to every
    start and end; None (no path) gives []"""
    return [dict(t, start=t['start'] + offset_s, end=t['end'] + offset_s) for t in (tokens or [])]


def join_segments(segment_tokens, segment_starts_s):
    """``predict_long``: the per-segment token lists (in time order of the segments) with every segment's start added -> one list
    that covers the whole recording in time order"""
    out = []
    for toks, t0 in zip(segment_tokens, segment_starts_s):
        out.extend(shift_tokens(toks, float(t0)))
    return out


def pack_hypotheses(ids_list, max_frames):
    """token id lists of one pass -> (flat int32 array = tokens [B, Lmax] | n_tokens [B], Lmax, alignable [B] bool).  A
    hypothesis longer than its pass has frames, or than the kernel's rows hold, cannot be aligned: it goes in as empty and comes
    out as None."""
    B = len(ids_list)
    cap = min(int(max_frames), MAX_TOKENS)
    alignable = np.array([len(ids) <= cap for ids in ids_list], bool)
    lmax = max([len(ids) for ids, ok in zip(ids_list, alignable) if ok] + [1])
    flat = np.zeros(B * lmax + B, np.int32)
    tok = flat[:B * lmax].reshape(B, lmax)
    for b, ids in enumerate(ids_list):
        if alignable[b]:
            tok[b, :len(ids)] = ids
            flat[B * lmax + b] = len(ids)
    return flat, lmax, alignable


def unpack_alignment(flat, B, lmax):
    """the packed int32 result of ``HipEngine.ctc_align(..., out=)`` on the host -> (start, end [B, Lmax] int32, peak [B, Lmax]
    float32, score [B] float32, status [B] int32)"""
    flat = np.ascontiguousarray(flat, np.int32).reshape(-1)
    n = B * lmax
    return (flat[:n].reshape(B, lmax), flat[n:2 * n].reshape(B, lmax), flat[2 * n:3 * n].view(np.float32).reshape(B, lmax),
            flat[3 * n:3 * n + B].view(np.float32), flat[3 * n + B:3 * n + 2 * B])


def utterance_tokens(ids, start, end, peak, score, status, reduction, sample_rate, duration_s, vocab_list, hop_samples=HOP_SAMPLES):
    """one utterance's row of the alignment -> its ``'tokens'`` value: [] for the empty transcript, None when the trellis holds no
    path for the hypothesis (status != 0 -- too few frames, or an attention decoder emitted the blank id -- or a path through a
    zero probability: score at the sentinel), else the list of
    ``frames_to_times``"""
    n = len(ids)
    if n == 0:
        return []
    if int(status) != 0 or not float(score) > SENTINEL / 2:
        return None
    names = [vocab_list[int(i)].replace('<space>', ' ') for i in ids]
    return frames_to_times(start[:n], end[:n], peak[:n], reduction, hop_samples, sample_rate, duration_s, names)
