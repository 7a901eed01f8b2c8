"""CPU: the numpy restatement of the CTC forced alignment (tests/ctc_align_ref.py) against brute-force enumeration, and the host
side of the token timestamps (masr_amd/decoders/ctc_alignment.py: frames -> seconds, the shift of predict_long)."""
import itertools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_align_ref as ar            # noqa: E402

from masr_amd.decoders import ctc_alignment as ca            # noqa: E402


def _log_softmax(x):
    x = np.asarray(x, np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=-1, keepdims=True))


HYPS = [list(h) for L in range(4) for h in itertools.product((1, 2), repeat=L)]


@pytest.mark.parametrize('T', [1, 2, 3, 4, 5, 6])
def test_restatement_against_enumeration_of_every_path(T):
    """all hypotheses with L <= 3 over V = 3: same best score as the enumeration of every labelling that collapses to the
    hypothesis, and the restatement's path is one of that score; the infeasible ones are reported as such"""
    rng = np.random.default_rng(100 + T)
    lp = _log_softmax(rng.standard_normal((T, 3)) * 2)
    for hyp in HYPS:
        best, arg = ar.brute_force(lp, hyp)
        got = ar.align(lp, hyp, np.float64)
        assert ar.feasible(hyp, T) == (best is not None), hyp
        if best is None:
            assert got['status'] == 1 and (got['start'] == -1).all() and (got['end'] == -1).all() and got['score'] == 0
            continue
        assert got['status'] == 0 and got['score'] == best, (hyp, got['score'], best)
        assert ar.path_is_valid(got['path'], hyp) and ar.labels_of(got['path'], hyp) in arg
        assert ar.path_score(lp, got['path'], hyp) == best
        # start / end / peak describe that path
        assert np.array_equal(ar.states_from_spans(got['start'], got['end'], T, len(hyp)), got['path'])
        for j, tok in enumerate(hyp):
            assert got['peak'][j] == lp[got['start'][j]:got['end'][j] + 1, tok].max()
        # float32 on float32 inputs: the same path unless two paths are closer than float32 resolves (not at these sizes)
        got32 = ar.align(lp.astype(np.float32), hyp, np.float32)
        assert got32['status'] == 0 and abs(float(got32['score']) - float(best)) <= 16 * T * 2.0 ** -24 * max(1.0, abs(float(best)))


def test_tie_rule_on_equal_log_probabilities():
    """every log-probability equal: every path ties, the rule decides -- stay first, the last blank wins the end"""
    lp = np.full((5, 3), -1.25, np.float32)
    got = ar.align(lp, [1, 2], np.float32)
    # the end takes state S - 1 (tie) and every state stays where it can, so the path reaches the last blank as early as the
    # trellis allows: token 1 on frame 0, the skip to token 2 on frame 1, the last blank from frame 2 on
    assert got['path'].tolist() == [1, 3, 4, 4, 4] and got['start'].tolist() == [0, 1] and got['end'].tolist() == [0, 1]
    best, arg = ar.brute_force(lp, [1, 2], np.float32)
    assert got['score'] == best and len(arg) > 1


def test_infeasible_and_edge_cases():
    lp = _log_softmax(np.zeros((2, 3)))
    assert ar.align(lp, [1, 1])['status'] == 1                  # needs 3 frames
    assert ar.align(lp[:1], [1, 2])['status'] == 1
    assert ar.align(lp[:0], [1])['status'] == 1
    r = ar.align(lp[:0], [])
    assert r['status'] == 0 and r['score'] == 0
    r = ar.align(_log_softmax(np.zeros((3, 3))), [1, 1])          # exactly feasible: token, blank, token
    assert r['status'] == 0 and r['path'].tolist() == [1, 2, 3]
    r = ar.align(lp, [])
    assert r['status'] == 0 and r['path'].tolist() == [0, 0] and r['score'] == np.float32(lp[0, 0]) + np.float32(lp[1, 0])
    # batch form: padding slots are -1 / 0
    s, e, p, sc, st = ar.align_batch(np.stack([_log_softmax(np.zeros((3, 3)))] * 2), [3, 2], [[1, 1], [2, 0]], [2, 1])
    assert st.tolist() == [0, 0] and s[1].tolist() == [0, -1] and e[1, 1] == -1 and p[1, 1] == 0


def test_frames_to_times_reduction_clipping_and_empty():
    start, end, peak = [0, 2, 5], [1, 2, 9], [math.log(0.5), 0.0, math.log(0.25)]
    got = ca.frames_to_times(start, end, peak, 4, 160, 16000, 10.0, ['a', 'b', 'c'])
    assert [t['token'] for t in got] == ['a', 'b', 'c']
    assert [t['start'] for t in got] == [0.0, 0.08, 0.2] and [t['end'] for t in got] == [0.08, 0.12, 0.4]
    assert [round(t['score'], 12) for t in got] == [0.5, 1.0, 0.25]
    got8 = ca.frames_to_times(start, end, peak, 8, 160, 16000, 0.75, ['a', 'b', 'c'])
    assert [t['start'] for t in got8] == [0.0, 0.16, 0.4]
    assert [t['end'] for t in got8] == [0.16, 0.24, 0.75]                       # (9 + 1) * 0.08 = 0.8 clipped to the duration
    # seconds of the utterance: the model's rate and hop decide, whatever rate the audio was given at
    assert ca.frames_to_times([3], [3], [0.0], 6, 160, 16000, 5.0, ['x'])[0]['start'] == pytest.approx(3 * 6 * 0.01)
    assert ca.frames_to_times([], [], [], 4, 160, 16000, 1.0, []) == []


def test_utterance_tokens_empty_none_and_text():
    vocab = ['<blank>', 'a', '<space>', 'b']
    assert ca.utterance_tokens([], [], [], [], 0.0, 0, 4, 16000, 1.0, vocab) == []
    assert ca.utterance_tokens([1], [-1], [-1], [0.0], 0.0, 1, 4, 16000, 1.0, vocab) is None
    assert ca.utterance_tokens([1], [0], [0], [0.0], ca.SENTINEL, 0, 4, 16000, 1.0, vocab) is None
    got = ca.utterance_tokens([1, 2, 3], [0, 1, 2, -1], [0, 1, 3, -1], [0.0, -1.0, -2.0, 0.0], -3.0, 0, 4, 16000, 1.0, vocab)
    assert ''.join(t['token'] for t in got) == 'a b' and got[2]['end'] == 0.16


def test_pack_and_unpack_round_trip():
    flat, lmax, ok = ca.pack_hypotheses([[3, 4, 5], [], [7] * 9], max_frames=8)
    assert lmax == 3 and ok.tolist() == [True, True, False]
    assert flat[:9].reshape(3, 3).tolist() == [[3, 4, 5], [0, 0, 0], [0, 0, 0]] and flat[9:].tolist() == [3, 0, 0]
    assert ca.pack_hypotheses([[], []], 5)[1] == 1                  # (Lmax is at least 1)
    B = 2
    packed = np.arange(B * (3 * lmax + 2), dtype=np.int32)
    s, e, p, sc, st = ca.unpack_alignment(packed, B, lmax)
    assert s.tolist() == [[0, 1, 2], [3, 4, 5]] and e[1].tolist() == [9, 10, 11] and st.tolist() == [20, 21]
    assert p.dtype == np.float32 and sc.dtype == np.float32 and p.view(np.int32)[0].tolist() == [12, 13, 14]


def test_join_segments_shifts_by_segment_start():
    a = [{'token': 'x', 'start': 0.0, 'end': 0.08, 'score': 1.0}]
    b = [{'token': 'y', 'start': 0.04, 'end': 0.12, 'score': 0.5}, {'token': 'z', 'start': 0.12, 'end': 0.2, 'score': 0.5}]
    got = ca.join_segments([a, None, [], b], [1.0, 2.0, 3.0, 4.5])
    assert [t['token'] for t in got] == ['x', 'y', 'z']
    assert [t['start'] for t in got] == [1.0, 4.54, 4.62] and got[2]['end'] == pytest.approx(4.7)
    assert a[0]['start'] == 0.0                                  # (copies: the segment's own list is as it was)


def test_predict_long_shifts_tokens_by_the_vad_segment_start():
    """predict_long itself, with the device pass and the VAD replaced: segments are recognised length-sorted, the tokens come back
    in time order on the recording's clock"""
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils.utils import dict_to_object

    class Vad:
        def get_speech_timestamps(self, samples, rate):
            return [{'start': 16000, 'end': 48000}, {'start': 64000, 'end': 72000}]

    p = MASRPredictor.__new__(MASRPredictor)
    p.configs = dict_to_object({'preprocess_conf': {'sample_rate': 16000}})
    p.vad_predictor = None
    seen = []

    def local(segs, timestamps=False):
        seen.append((len(segs), timestamps))
        out = []
        for s in segs:
            d = s.num_samples / 16000.0
            out.append({'text': 'ab', 'score': 50.0, 'tokens': [{'token': 'a', 'start': 0.0, 'end': d / 2, 'score': 0.9},
                                                                  {'token': 'b', 'start': d / 2, 'end': d, 'score': 0.8}]})
        return out
    p._predict_local = local
    res = p.predict_long(np.zeros(80000, np.float32), vad_predictor=Vad(), timestamps=True)
    assert seen == [(2, True)] and res['text'] == 'ab，ab'
    assert [(t['token'], t['start'], t['end']) for t in res['tokens']] == [('a', 1.0, 2.0), ('b', 2.0, 3.0), ('a', 4.0, 4.25),
                                                                          ('b', 4.25, 4.5)]
    seen.clear()
    plain = p.predict_long(np.zeros(80000, np.float32), vad_predictor=Vad())
    assert seen == [(2, False)] and 'tokens' not in plain
