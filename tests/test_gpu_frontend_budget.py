"""GPU: the feature front end (masr_amd/csrc/fbank.hip: fbank_kernel, mfcc_kernel, norm_int16_kernel, the gain kernels) against
oracle/fbank.py in float64 under the rule of tests/budget.py, C = 8, on the int16 samples the kernel itself transformed; inputs,
truth and reference come from tests/frontend_ref.py (checked on the CPU by tests/test_frontend_ref_cpu.py).

a  signal classes, one budget case each (never pooled): log domain for all, peak-relative as well for tone / chirp / DC
b  the floor: zeros, a constant, one +-1 sample
c  one tone per mel filter: the strongest filter of the strongest frame
d  framing edges in a ragged batch; nothing behind a row's length is read
e  an utterance's frames do not depend on its batch
f  the sample path: supplied gains, float32 samples, clipping, silence
g  MFCC end to end

dB normalisation is off unless a case is about it, so the kernel sees exactly the samples the oracle gets."""
import functools

import numpy as np
import pytest
import torch

from oracle import fbank as ofb
from tests import budget
from tests import frontend_ref as fr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from masr_amd.engine import HipEngine
    e = HipEngine(None)
    yield e
    e.close()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def lens_of(pcm, lens=None):
    return np.full(pcm.shape[0], pcm.shape[1], np.int32) if lens is None else np.asarray(lens, np.int32)


def fbank(e, pcm, lens=None, use_db=False, **kw):
    """-> [feats [B, T, 80] float32 numpy, frames [B] numpy, ...]"""
    out = e.fbank_batch(dev(pcm), dev(lens_of(pcm, lens)), use_db, -20.0, **kw)
    return [t.cpu().numpy() for t in out]


def mfcc(e, pcm, n_ceps, lens=None):
    out = e.mfcc_batch(dev(pcm), dev(lens_of(pcm, lens)), n_ceps, False, -20.0)
    return [t.cpu().numpy() for t in out]


# ---- a. signal classes --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def class_batch():
    """all classes in one batch [rows, 4000] -> (pcm, {class: row slice}, y64, y32)"""
    parts, rows, at = [], {}, 0
    for name in fr.CLASSES:
        x = fr.signal(name)
        parts.append(x)
        rows[name] = slice(at, at + x.shape[0])
        at += x.shape[0]
    pcm = np.concatenate(parts, axis=0)
    y64, y32, counts = fr.batch_truth_and_reference(pcm)
    assert set(counts) == {ofb.num_frames(fr.N_UTT)}
    return pcm, rows, y64, y32


@pytest.fixture(scope='module')
def class_feats(eng):
    pcm = class_batch()[0]
    feats, frames = fbank(eng, pcm)
    assert feats.shape == (pcm.shape[0], 23, 80) and (frames == 23).all()
    return feats


@pytest.mark.parametrize('name', fr.CLASSES)
def test_signal_class_log_domain(class_feats, name):
    _, rows, y64, y32 = class_batch()
    r = rows[name]
    budget.check(f'fbank {name} log', y64[r], y32[r], class_feats[r])


# The one class with an allowance of its own on the max criterion (the rms criterion keeps C = 8).  Cause: the mel weights, not the
# kernel.  The engine's table (build_fbank_tables) takes mel(f) = 1127 * logf(1 + f / 700) from the C library, whose logf is
# correctly rounded here; the oracle's float32 weights -- which the float64 truth takes as given -- come from numpy's float32 log,
# which rounds the other way at some 30 of the 256 bin frequencies, and one ulp of a mel value moves a tap weight by up to
# 1.4e-5 (tests/frontend_ref.py).  Broadband noise on a DC has many strong bins in wide filters, each judged to a few 1e-7 of the
# frame's peak, so these taps show.  The allowance is the reference side's own spread: how much further from the truth the
# oracle's float32 evaluation is with a correctly rounded logarithm in its weights than with numpy's (about 7 on this input).
WEIGHTS_SPREAD_CLASSES = ('dc_noise',)


@pytest.mark.parametrize('name', fr.PEAKED)
def test_signal_class_peak_relative(class_feats, name):
    pcm, rows, y64, y32 = class_batch()
    r = rows[name]
    t, ref = fr.peak_relative(y64[r], y64[r]), fr.peak_relative(y32[r], y64[r])
    c_max = None
    if name in WEIGHTS_SPREAD_CLASSES:
        spread = fr.weights_spread(t, ref, fr.peak_relative(fr.reference_rounded_log(pcm[r]), y64[r]))
        print(f'{name}: spread of the reference under the rounding of the mel logarithm x{spread:.2f}')
        c_max = budget.C * spread
    budget.check(f'fbank {name} peak-relative', t, ref, fr.peak_relative(class_feats[r], y64[r]), c_max=c_max)


# ---- b. the floor -------------------------------------------------------------------------------------------------------------------
def frames_holding(i):
    """the frames whose 400 samples include sample i"""
    return [t for t in range(ofb.num_frames(fr.N_UTT)) if 160 * t <= i < 160 * t + 400]


def test_floor(eng):
    n = fr.N_UTT
    singles = ((1000, 1), (2000, -1))
    assert frames_holding(1000) == [4, 5, 6] and frames_holding(2000) == [11, 12]
    pcm = np.zeros((2 + len(singles), n), np.int16)
    pcm[1] = 1234
    for b, (i, v) in enumerate(singles):
        pcm[2 + b, i] = v
    y64, y32, _ = fr.batch_truth_and_reference(pcm)
    assert (y64[:2] == fr.LOG_EPS).all()
    feats, frames = fbank(eng, pcm)
    assert np.isfinite(feats).all() and (frames == 23).all()
    budget.check('fbank floor zeros', y64[0], y32[0], feats[0])
    budget.check('fbank floor constant 1234', y64[1], y32[1], feats[1])
    for b, (i, v) in enumerate(singles):
        b += 2
        budget.check(f'fbank floor single sample {v:+d} at {i}', y64[b], y32[b], feats[b])
        on_floor = np.ones(23, bool)
        on_floor[frames_holding(i)] = False
        assert (y64[b][on_floor] == fr.LOG_EPS).all() and (y64[b][~on_floor].max(axis=-1) > fr.LOG_EPS + 10.0).all()
        assert np.abs(feats[b][on_floor] - fr.LOG_EPS).max() <= budget.C * budget.ULP32 * abs(fr.LOG_EPS)
        assert (feats[b][~on_floor].max(axis=-1) > fr.LOG_EPS + 10.0).all()


# ---- c. each mel filter alone -------------------------------------------------------------------------------------------------------
def test_each_filter_alone(eng):
    pcm = fr.filter_tones()
    y64, y32, _ = fr.batch_truth_and_reference(pcm)
    feats, _ = fbank(eng, pcm)
    judged = 0
    for i, m in enumerate(fr.FILTERS):
        t = fr.strongest_frame(y64[i])
        want = int(np.argmax(y64[i, t]))
        assert abs(want - m) <= 1, (m, want)
        e_ref = float(np.abs(y32[i, t] - y64[i, t]).max())
        if budget.argmax_margin(y64[i, t], e_ref):
            judged += 1
            got = int(np.argmax(feats[i, t]))
            assert got == want, f'tone at the centre bin {fr.filter_bin(m)} of filter {m}: strongest filter {got}, float64 {want}'
    assert judged == len(fr.FILTERS)            # (every listed filter has a safe margin: tests/test_frontend_ref_cpu.py)


# ---- d. framing edges ---------------------------------------------------------------------------------------------------------------
N_MAX_OF_T = {1: 450, 2: 600, 3: 800, 4: 1000, 5: 1100}          # T_max -> an n_max that is none of the lengths


def ragged_case(n_max, lens=None, garbage_seed=0):
    lens = [l for l in fr.RAGGED_LENS if l <= n_max] if lens is None else list(lens)
    assert n_max not in lens
    return fr.ragged_batch(n_max, lens, garbage_seed=garbage_seed), lens


def check_ragged(eng, name, n_max, lens=None):
    pcm, lens = ragged_case(n_max, lens, 0)
    pcm2, _ = ragged_case(n_max, lens, 1)
    valid = np.arange(n_max)[None, :] < np.asarray(lens)[:, None]
    assert (pcm[valid] == pcm2[valid]).all() and (pcm[~valid] != pcm2[~valid]).mean() > 0.99
    feats, frames = fbank(eng, pcm, lens)
    feats2, frames2 = fbank(eng, pcm2, lens)
    T_max = ofb.num_frames(n_max)
    assert feats.shape == (len(lens), T_max, 80)
    assert np.array_equal(feats.view(np.uint32), feats2.view(np.uint32)), 'samples behind a row\'s length were read'
    want = [ofb.num_frames(l) for l in lens]
    assert frames.tolist() == want and frames2.tolist() == want
    trimmed = pcm.copy()
    trimmed[~valid] = 0
    y64, y32, counts = fr.batch_truth_and_reference(trimmed, lens)
    assert counts == want
    for b, T in enumerate(want):
        assert (feats[b, T:] == 0.0).all(), (b, T)
    if any(want):
        budget.check(name, y64, y32, feats, budget.valid_mask(feats.shape, None, counts=want))
    return feats, lens


@pytest.mark.parametrize('T_max', sorted(N_MAX_OF_T))
def test_framing_edges(eng, T_max):
    n_max = N_MAX_OF_T[T_max]
    assert ofb.num_frames(n_max) == T_max
    check_ragged(eng, f'fbank ragged T_max {T_max}', n_max)


def test_framing_batch_shorter_than_a_frame(eng):
    lens = [0, 1, 398]
    pcm = fr.ragged_batch(399, lens)
    feats, frames = fbank(eng, pcm, lens)
    assert feats.shape == (3, 0, 80) and frames.tolist() == [0, 0, 0]
    mf, frames = mfcc(eng, pcm, 13, lens)
    assert mf.shape == (3, 0, 13) and frames.tolist() == [0, 0, 0]


@pytest.mark.parametrize('B', [1, 33])
def test_framing_batch_sizes(eng, B):
    lens = [1041] if B == 1 else [fr.RAGGED_LENS[(7 * b + 3) % len(fr.RAGGED_LENS)] for b in range(B)]
    check_ragged(eng, f'fbank ragged B {B}', 1100, lens)


# ---- e. frames do not depend on the batch -------------------------------------------------------------------------------------------
def test_frames_do_not_depend_on_the_batch(eng):
    n_max = 1100
    pcm, lens = ragged_case(n_max)
    in_batch, _ = fbank(eng, pcm, lens)
    longer = np.random.default_rng(5).integers(-32768, 32768, (len(lens), 2000)).astype(np.int16)
    for b, l in enumerate(lens):
        longer[b, :l] = pcm[b, :l]
    in_longer, _ = fbank(eng, longer, lens)
    seen = 0
    for b, l in enumerate(lens):
        T = ofb.num_frames(l)
        if not T:
            continue
        alone, frames = fbank(eng, pcm[b:b + 1, :l])
        assert int(frames[0]) == T and alone.shape == (1, T, 80)
        for other, what in ((in_batch, 'in the ragged batch'), (in_longer, 'with n_max raised')):
            assert np.array_equal(alone[0].view(np.uint32), other[b, :T].view(np.uint32)), (b, l, what)
        seen += T
    assert seen == sum(fr.RAGGED_FRAMES)


# ---- f. the sample path -------------------------------------------------------------------------------------------------------------
def int16_samples():
    x = fr.white()
    x[0, :8] = [32767, -32768, 32766, -32767, 1, -1, 0, 16384]
    return x


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('gain', fr.GAINS)
@pytest.mark.parametrize('fmt', ['int16', 'float32'])
def test_supplied_gain_sample_path(eng, fmt, gain):
    x = int16_samples() if fmt == 'int16' else fr.float_samples()
    if fmt == 'float32':
        assert (np.signbit(x) & (x == 0)).any() and (np.abs(x) > 1).any() and (x == 1).any() and (x == -1).any()
    g = torch.tensor([gain], dtype=torch.float32)
    feats, frames, norm = fbank(eng, x, use_db=True, return_norm=True, gain_in=g)
    want = fr.expected_norm(x[0], np.float32(gain))
    assert norm.dtype == np.int16 and np.array_equal(norm[0], want), \
        f'{fmt} gain {gain}: {(norm[0] != want).sum()} samples differ, first at {np.flatnonzero(norm[0] != want)[:4]}'
    if gain > (0.5 if fmt == 'float32' else 1):
        assert (want == 32767).any() and (want == -32768).any()
    # norm_sample_fast: the features are those of the returned int16 samples with the normalisation off
    plain, _ = fbank(eng, norm)
    assert np.array_equal(bits(feats), bits(plain))
    y64, y32 = fr.truth_and_reference(norm[0])
    budget.check(f'fbank {fmt} gain {gain:g}', y64, y32, feats[0])


def test_float_input_on_the_int16_grid(eng):
    x = int16_samples()
    xf = ofb.pcm16_to_float32(x[0])[None, :]
    a, _ = fbank(eng, x)
    b, _ = fbank(eng, xf)
    assert np.array_equal(bits(a), bits(b))
    for gain in fr.GAINS:
        g = torch.tensor([gain], dtype=torch.float32)
        a, _, na = fbank(eng, x, use_db=True, return_norm=True, gain_in=g)
        b, _, nb = fbank(eng, xf, use_db=True, return_norm=True, gain_in=g)
        assert np.array_equal(na, nb), gain
        assert np.array_equal(bits(a), bits(b)), gain


def test_clipping_under_the_device_gain(eng):
    x = fr.spikes()
    want = fr.oracle_norm(x[0])
    feats, frames, norm, gain = fbank(eng, x, use_db=True, return_norm=True, return_gain=True)
    assert float(gain[0]) > 2.0
    diff = norm[0].astype(np.int32) - want.astype(np.int32)
    # the +-1 LSB allowance of test_fbank_testwav_against_reference_fixture (the gain is reproducible to a few ulp only)
    assert np.abs(diff).max() <= 1 and (diff != 0).mean() < 5e-3, (np.abs(diff).max(), (diff != 0).mean())
    clipped = (want == 32767) | (want == -32768)
    assert (want == 32767).sum() >= 8 and (want == -32768).sum() >= 8
    assert np.array_equal(norm[0][clipped], want[clipped])
    y64, y32 = fr.truth_and_reference(norm[0])
    budget.check('fbank clipped spikes', y64, y32, feats[0])


def test_silence_under_the_device_gain(eng):
    n = fr.N_UTT
    pcm = fr.ragged_batch(n, [0, n])
    pcm[1] = 0
    lens = [0, n]
    feats, frames, norm, gain = fbank(eng, pcm, lens, use_db=True, return_norm=True, return_gain=True)
    # digital silence: the reference's rms_db counts a zero mean square as 1, so the gain is target_dB itself, 10 ** (-20 / 20);
    # a zero-length utterance has no samples to weigh and gets the same gain
    silent = np.float32(10. ** ((-20 - ofb.rms_db(np.zeros(n, np.float32))) / 20.))
    assert silent == np.float32(0.1)
    assert gain.tolist() == [silent, silent]
    assert np.isfinite(feats).all() and frames.tolist() == [0, 23] and (norm == 0).all()
    assert (feats[0] == 0.0).all()
    y64, y32 = fr.truth_and_reference(pcm[1])
    assert (y64 == fr.LOG_EPS).all()
    budget.check('fbank silence, device gain', y64, y32, feats[1])


# ---- g. MFCC ------------------------------------------------------------------------------------------------------------------------
MFCC_CLASSES = ('synthetic', 'white', 'chirp')
N_CEPS = (13, 40, 1, 80)              # two usual values and the bounds masr_mfcc_batch accepts: 1 <= n_ceps <= 80


@functools.lru_cache(maxsize=None)
def mfcc_batch_pcm():
    parts, rows, at = [], {}, 0
    for name in MFCC_CLASSES:
        x = fr.signal(name)
        parts.append(x)
        rows[name] = slice(at, at + x.shape[0])
        at += x.shape[0]
    return np.concatenate(parts, axis=0), rows


@pytest.mark.parametrize('n_ceps', N_CEPS)
def test_mfcc_budget(eng, n_ceps):
    pcm, rows = mfcc_batch_pcm()
    y64, y32, _ = fr.batch_truth_and_reference(pcm, None, 'mfcc', n_ceps)
    out, frames = mfcc(eng, pcm, n_ceps)
    assert out.shape == (pcm.shape[0], 23, n_ceps) and (frames == 23).all()
    failed = []
    for name in MFCC_CLASSES:
        r = rows[name]
        f = budget.evaluate(y64[r], y32[r], out[r])
        print(budget.line(f'mfcc n_ceps {n_ceps} {name}', f), flush=True)
        if not f['ok']:
            failed.append(budget.line(f'mfcc n_ceps {n_ceps} {name}', f))
    assert not failed, 'over budget -- ' + ' | '.join(failed)


@pytest.mark.parametrize('n_ceps', [0, 81])
def test_mfcc_refuses_n_ceps_out_of_range(eng, n_ceps):
    from masr_amd._lib import MasrError
    pcm = fr.synthetic(800)
    with pytest.raises(MasrError, match='n_ceps'):
        eng.mfcc_batch(dev(pcm), dev(lens_of(pcm)), n_ceps, False, -20.0)
