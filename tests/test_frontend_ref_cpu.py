"""CPU: the inputs of tests/test_gpu_frontend_budget.py against the reference alone (tests/frontend_ref.py, oracle/fbank.py) -- the
conditions under which the GPU cases mean what they say, so that a later change of a generator cannot quietly turn a tight case
into a loose or an empty one."""
import numpy as np
import pytest

from oracle import fbank as ofb
from tests import budget
from tests import frontend_ref as fr


@pytest.fixture(scope='module')
def classes():
    out = {}
    for name in fr.CLASSES:
        pcm = fr.signal(name)
        assert pcm.dtype == np.int16 and pcm.shape[1] == fr.N_UTT
        out[name] = (pcm,) + tuple(fr.batch_truth_and_reference(pcm)[:2])
    return out


@pytest.mark.parametrize('name', fr.CLASSES)
def test_reference_error_is_finite_and_nonzero(classes, name):
    pcm, y64, y32 = classes[name]
    assert np.array_equal(pcm, fr.signal(name))                  # deterministic
    e = (y32 - y64).astype(np.float64)
    assert np.isfinite(y64).all() and np.isfinite(e).all() and np.abs(e).max() > 0 and budget.rms(e) > 0
    assert (y64 > fr.LOG_EPS).all()                              # no bin of a class sits on the floor: that is case b
    if name in fr.PEAKED:
        ep = fr.peak_relative(y32, y64) - fr.peak_relative(y64, y64)
        assert np.isfinite(ep).all() and np.abs(ep).max() > 0 and budget.rms(ep) > 0
        assert (fr.peak_relative(y64, y64).max(axis=-1) == 1.0).all()
        # tight where it matters: a float32 evaluation is within a few 1e-6 of a frame's peak in every bin
        assert np.abs(ep).max() < 1e-5


@pytest.mark.parametrize('name', fr.FLAT)
def test_flat_classes_are_tight_in_the_log_domain(classes, name):
    _, y64, y32 = classes[name]
    assert np.abs(y32 - y64).max() < 1e-4


def test_peak_relative_uses_the_truths_peak():
    y64 = np.log(np.array([[1.0, 4.0, 2.0], [8.0, 1.0, 1.0]]))
    assert np.allclose(fr.peak_relative(y64, y64), [[0.25, 1.0, 0.5], [1.0, 0.125, 0.125]])
    assert np.allclose(fr.peak_relative(y64 + np.log(2.0), y64), [[0.5, 2.0, 1.0], [2.0, 0.25, 0.25]])


def test_chirp_makes_every_filter_the_strongest_of_some_frame(classes):
    _, y64, _ = classes['chirp']
    strongest = set(np.argmax(y64, axis=-1).reshape(-1).tolist())
    assert strongest == set(range(80)), sorted(set(range(80)) - strongest)


def test_spike_signal_clips_at_both_ends():
    x = fr.spikes()[0]
    s = ofb.pcm16_to_float32(x)
    gain = 10. ** ((-20 - ofb.rms_db(s)) / 20.)
    assert gain > 2.0
    want = fr.oracle_norm(x)
    assert (want == 32767).sum() >= 8 and (want == -32768).sum() >= 8
    assert ((want != 0) == (x != 0)).all()


def test_filter_tones_have_a_safe_margin():
    assert set(range(64, 80)) <= set(fr.FILTERS) and {0, 63} <= set(fr.FILTERS)
    assert sum(0 < m < 63 for m in fr.FILTERS) >= 3
    pcm = fr.filter_tones()
    y64, y32, counts = fr.batch_truth_and_reference(pcm)
    assert set(counts) == {3}
    for i, m in enumerate(fr.FILTERS):
        t = fr.strongest_frame(y64[i])
        assert abs(int(np.argmax(y64[i, t])) - m) <= 1, m
        e_ref = float(np.abs(y32[i, t] - y64[i, t]).max())
        assert e_ref > 0 and bool(budget.argmax_margin(y64[i, t], e_ref)), m
        assert int(np.argmax(y32[i, t])) == int(np.argmax(y64[i, t]))


def test_ragged_lengths_and_frame_counts():
    assert tuple(ofb.num_frames(l) for l in fr.RAGGED_LENS) == fr.RAGGED_FRAMES == (0, 0, 0, 1, 1, 1, 2, 2, 3, 5)
    a, b = fr.ragged_batch(1100, garbage_seed=0), fr.ragged_batch(1100, garbage_seed=1)
    for r, l in enumerate(fr.RAGGED_LENS):
        assert np.array_equal(a[r, :l], b[r, :l]) and (a[r, l:] != b[r, l:]).mean() > 0.99


def test_sample_path_inputs_and_expected_values():
    x = fr.float_samples()[0]
    assert x.dtype == np.float32 and (np.signbit(x) & (x == 0)).any() and (x == 1).any() and (x == -1).any()
    assert (x > 1).any() and (x < -1).any()
    scaled = x.astype(np.float64) * 32768.0
    off_grid = (scaled != np.rint(scaled)) & (np.abs(scaled) < 32767)
    assert (off_grid & (x > 0)).sum() > 100 and (off_grid & (x < 0)).sum() > 100
    want = fr.expected_norm(x, 1.0)
    # truncation towards zero, not floor: a negative value off the grid goes UP to the next integer
    neg = off_grid & (x < 0)
    assert np.array_equal(want[neg], np.ceil(scaled[neg]).astype(np.int16))
    assert np.array_equal(want[off_grid & (x > 0)], np.floor(scaled[off_grid & (x > 0)]).astype(np.int16))
    assert want[x >= 1].tolist() == [32767] * int((x >= 1).sum()) and want[x <= -1].tolist() == [-32768] * int((x <= -1).sum())
    # the reference's own path: AudioSegment float32 -> gain -> int16
    i16 = fr.white()[0]
    for g in fr.GAINS:
        s = ofb.pcm16_to_float32(i16)
        s *= np.float32(g)
        assert np.array_equal(fr.expected_norm(i16, g), ofb.float32_to_int16(s))


def test_second_reference_differs_in_the_mel_logarithm_only(classes):
    pcm, y64, y32 = classes['dc_noise']
    assert np.array_equal(fr.fbank_f32_with_banks(pcm[0], ofb.mel_banks()), y32[0])          # the restatement is the oracle's
    a, b = ofb.mel_banks(), fr.mel_banks_rounded_log()
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (80, 257)
    # the same filters on the same bins; a weight moves by at most two ulp of a mel value over the filter spacing
    assert np.array_equal(a > 0, b > 0)
    assert np.abs(a.astype(np.float64) - b).max() <= 2 * np.spacing(np.float32(2840.0)) / fr.mel_edges()[1]
    t, ref = fr.peak_relative(y64, y64), fr.peak_relative(y32, y64)
    spread = fr.weights_spread(t, ref, fr.peak_relative(fr.reference_rounded_log(pcm), y64))
    assert 1.0 <= spread < 16.0, spread
    assert fr.weights_spread(t, ref, ref) == 1.0


def test_floor_inputs_sit_on_the_floor():
    for v in (0, 1234):
        y64, y32 = fr.truth_and_reference(np.full(fr.N_UTT, v, np.int16))
        assert (y64 == fr.LOG_EPS).all() and np.abs(y32 - y64).max() < 1e-6
