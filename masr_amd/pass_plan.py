"""How ``predict_batch`` cuts a length-sorted list into device passes and how it pipelines them: pure functions of sizes, the
decoder and the environment (no device, no torch).  ``offline_pass.py`` runs one pass; ``predict.py`` runs the plan."""
from collections import namedtuple


def balanced_cuts(sorted_lengths, budget):
    """[lo, hi) index ranges over an ASCENDING list of utterance lengths such that every range holds as many utterances as fit
    count x (its longest utterance) <= budget, cut from the long end (at least one utterance per range); ranges in ascending
    order.  A range is one device pass: all passes then cost about the same padded work -- one full round of workgroups each --
    instead of a pass of long utterances costing twice a pass of short ones."""
    cuts, hi = [], len(sorted_lengths)
    while hi > 0:
        k = max(1, min(hi, int(float(budget) // max(float(sorted_lengths[hi - 1]), 1.0))))
        cuts.append((hi - k, hi))
        hi -= k
    cuts.reverse()
    return cuts


def pass_cuts(n, hints_sorted, batch_size):
    """[lo, hi) ranges, ascending, that cut ``n`` (length-sorted) utterances into device passes.  ``batch_size``: a number
    (passes of that many, 0: one pass), a LIST of pass sizes counted from the LONGEST utterance down (the last size repeats), or
    ``('balanced', budget)``: count x longest <= budget per pass over the ascending lengths ``hints_sorted``."""
    if isinstance(batch_size, tuple):
        return balanced_cuts(hints_sorted, batch_size[1])
    if isinstance(batch_size, list):
        if not batch_size:
            raise ValueError('batch_size: an empty list of pass sizes')
        cuts, hi, k = [], n, 0
        while hi > 0:
            step = max(1, int(batch_size[min(k, len(batch_size) - 1)]))
            cuts.append((max(0, hi - step), hi))
            hi -= step
            k += 1
        cuts.reverse()
        return cuts
    step = batch_size if batch_size else max(n, 1)
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


def search_on_gpu(beam_decoder, vocab_size):
    """does the CTC prefix search of ``beam_decoder`` (None: another decoder) run on the GPU?  (a word-based scorer, or beam x
    top-n beyond the kernel's LDS: the search runs on host threads whatever use_gpu_search says)"""
    return beam_decoder is not None and bool(getattr(beam_decoder, 'use_gpu_search', False)) and \
        bool(beam_decoder.gpu_search_supported(1, vocab_size))


PassPolicy = namedtuple('PassPolicy', 'reverse depth lanes prep_ahead')


def pass_policy(decoder, gpu_search, n_passes, env):
    """what ``predict_batch`` decides per call: ``decoder`` is configs.decoder, ``gpu_search`` is ``search_on_gpu``, ``env`` is
    os.environ.  -> (passes longest first?, passes in flight before the oldest is collected, lanes, next pass prepared ahead?)"""
    # Same passes either way; with the GPU prefix search the LONGEST pass goes first: its search (one workgroup per utterance,
    # the longest utterance is the critical path of the call) then starts right after the first encoder pass and the shorter
    # passes' encoders and searches run underneath it.  Depth 2: pass k is launched, then pass k - 1 is collected.
    reverse, depth = False, 2
    if decoder == 'ctc_beam_search' and not gpu_search and env.get('MASR_HOST_SEARCH_DEFER', '1') == '1':
        # host-thread search: pruning is queued behind each pass, the search itself runs when the pass is collected -- two
        # passes behind the launches, so the device always has a pass queued; the pass of the shortest utterances (the
        # quickest search) comes last: nothing runs under the last search
        reverse, depth = True, 3
    if gpu_search:
        # a prefix search is a long serial kernel on a few CUs (one workgroup per utterance, frames in sequence): the encoders
        # of up to three further passes are launched underneath it before its results are waited for
        reverse, depth = True, 4
    # Two LANES (masr_select_lane): consecutive passes run on two streams and two workspace sets of the one engine, so the
    # kernels of one pass fill the CUs the other leaves idle -- a fused Squeezeformer stage holds one 32-row block per CU,
    # the 429 / 179 valid row blocks of BASELINE configs[2]'s two passes are 2 + 1 rounds of 256 CUs one after the other
    # and 2.4 side by side (encoders alone: 17.0 -> 14.8 ms; the greedy call 18.5 -> 17.2 ms).  The preparation of pass
    # k + 1 (upload, mean squares) is queued BEFORE the encoder of pass k.  NOT with the prefix search on the GPU: a search
    # is a chain of dependent memory round trips and slows down with everything that runs beside it -- its pass's encoder
    # must finish EARLY, not share the chip (sharpened head 23.5 -> 24.7 ms, flat 28.0 -> 30.8 ms per call with two lanes;
    # passes of 16 or uneven passes on two lanes: 23.4 - 31 / 33 - 38 ms).  MASR_LANES=1 | 2 overrides (A/B).
    lanes = max(1, min(2, int(env.get('MASR_LANES', '1' if gpu_search else '2')))) if n_passes > 1 else 1
    # (MASR_PREP_AHEAD=0, A/B: the next pass prepared AFTER this pass's encoder is launched -- its upload and mean squares
    #  then wait 6 ms for CUs and the second lane starts late: 18.6 against 17.0 ms per configs[2] greedy call)
    return PassPolicy(reverse, depth, lanes, lanes > 1 and env.get('MASR_PREP_AHEAD', '1') == '1')
