"""Inputs and references of the feature front-end tests (a plain helper module: tests import it).

The kernels under test are ``fbank_kernel`` / ``mfcc_kernel`` / ``norm_int16_kernel`` of masr_amd/csrc/fbank.hip.  Truth is
``oracle.fbank.kaldi_fbank`` / ``kaldi_mfcc`` in float64, the reference the same in float32, both on the int16 samples the kernel
itself transformed (the +-1 LSB gain effect documented in tests/test_gpu_parity.py never enters), and the rule is that of
tests/budget.py, C = 8 unchanged.

Signal classes.  Each generator is deterministic from its seed and returns int16 PCM.  The *flat* classes have no bin far below
their frame's peak: the reference's log-domain error is a few 1e-5 and the log-domain rule is tight.  The *peaked* classes
(tone, chirp, DC + noise) have bins tens of nats below the peak of their frame; the float32 FFT's error there is set by the peak,
not by the bin, so the log-domain ``e_ref`` is large and says nothing about the strong bins.  ``peak_relative`` maps log-mel rows
to mel energies divided by the truth's largest energy of the same frame; in that domain the same rule is tight for the bins that
matter, and the peaked classes are judged in both domains."""
import math

import numpy as np

from masr_amd.utils.synthetic import synthetic_pcm
from oracle import fbank as ofb

N_UTT = 4000                       # 23 frames
LOG_EPS = float(np.log(np.float64(ofb.EPS_F32)))       # the floor of the log-mel features
FS, NFFT, BIN_HZ = 16000.0, 512, 16000.0 / 512
FLAT = ('synthetic', 'white', 'lsb3', 'impulses')
PEAKED = ('tone_bin', 'tone_between', 'chirp', 'dc_noise')
CLASSES = FLAT + PEAKED


def _i16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


# ---- generators: [rows, n] int16 -------------------------------------------------------------------------------------------------
def synthetic(n=N_UTT, seed=11, rows=1):
    return synthetic_pcm(rows, n, seed=seed)


def white(n=N_UTT, seed=21, rows=1, amp=20000):
    return np.random.default_rng(seed).integers(-amp, amp + 1, (rows, n)).astype(np.int16)


def lsb3(n=N_UTT, seed=27, rows=1):
    return white(n, seed, rows, amp=3)


def impulses(n=N_UTT, seed=23, rows=1, every=25):
    """full-scale samples of either sign at one position in ``every`` on average, zeros elsewhere (every 400-sample frame holds a
    few, so no frame sits on the floor)"""
    rng = np.random.default_rng(seed)
    hit = rng.random((rows, n)) < 1.0 / every
    sign = rng.integers(0, 2, (rows, n)) * 2 - 1
    return np.where(hit, np.where(sign > 0, 32767, -32768), 0).astype(np.int16)


def tone(freq, n=N_UTT, amp=20000.0, phase=0.3):
    t = np.arange(n, dtype=np.float64)
    return _i16(amp * np.sin(2.0 * math.pi * freq * t / FS + phase))[None, :]


def tone_bin(n=N_UTT):
    """1000 Hz = FFT bin 32 exactly"""
    return tone(1000.0, n)


def tone_between(n=N_UTT):
    """1015.625 Hz = bin 32.5"""
    return tone(1015.625, n)


def mel_to_hz(m):
    return 700.0 * (np.exp(np.asarray(m, np.float64) / 1127.0) - 1.0)


def mel_edges(n_mels=80, low=20.0, high=8000.0):
    """(mel_low, delta): filter m spans mel_low + m * delta .. mel_low + (m + 2) * delta, centre at (m + 1) * delta"""
    lo, hi = ofb.mel_scale(low), ofb.mel_scale(high)
    return float(lo), float((hi - lo) / (n_mels + 1))


CHIRP_ROWS, CHIRP_OVERLAP, CHIRP_TURN = 5, 640, 0.95


def chirp(n=N_UTT, amp=20000.0, rows=CHIRP_ROWS, overlap=CHIRP_OVERLAP, turn=CHIRP_TURN):
    """one sweep, linear on the mel scale, from one filter spacing below 20 Hz (held at 5 Hz until it gets there) up to 8 kHz and, in
    the last 5 %, back down to the centre of filter 79; cut into ``rows`` utterances of ``n`` samples, each starting ``overlap``
    samples before the one before it ends.  80 filters over 5 x 23 frames is less than one filter per hop, so every mel filter
    -- filters 64..79 and the last one next to Nyquist included -- is the strongest of some frame (asserted in
    tests/test_frontend_ref_cpu.py)."""
    total = rows * n - (rows - 1) * overlap
    mlo, delta = mel_edges()
    u = np.arange(total, dtype=np.float64) / (total - 1)
    mel = np.where(u < turn, (mlo - delta) + (u / turn) * 82.0 * delta, mlo + 81.0 * delta - (u - turn) / (1.0 - turn) * delta)
    f = np.clip(mel_to_hz(mel), 5.0, 8000.0)
    x = _i16(amp * np.sin(2.0 * math.pi * np.cumsum(f) / FS))
    return np.stack([x[r * (n - overlap): r * (n - overlap) + n] for r in range(rows)])


def dc_noise(n=N_UTT, seed=24, rows=1, dc=30000, amp=2000):
    return (dc + np.random.default_rng(seed).integers(-amp, amp + 1, (rows, n))).astype(np.int16)


def signal(name, n=N_UTT):
    return {'synthetic': synthetic, 'white': white, 'lsb3': lsb3, 'impulses': impulses, 'tone_bin': tone_bin,
            'tone_between': tone_between, 'chirp': chirp, 'dc_noise': dc_noise}[name](n)


def spikes(n=2 * N_UTT, every=400, amp=30000):
    """silent except one sample of +-``amp`` every ``every`` samples, signs alternating: the reference's dB gain is above 2 and the
    spikes saturate at both ends of int16"""
    x = np.zeros(n, np.int16)
    pos = np.arange(every // 2, n, every)
    x[pos] = np.where(np.arange(len(pos)) % 2 == 0, amp, -amp)
    return x[None, :]


# ---- the float32 sample path ---------------------------------------------------------------------------------------------------------
GAINS = (1.0, 0.1, 0.9759301, 2.18, 7.3)


def float_samples(n=N_UTT, seed=31):
    """float32 samples for ``norm_sample``: values off the int16 grid of both signs (.25 / .5 / .75 LSB and random fractions),
    exactly +-1.0, values beyond +-1, -0.0 and +0.0, and the grid values next to the clip points"""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(-0.9, 0.9, n)).astype(np.float32)
    k = rng.integers(-30000, 30000, n)
    frac = np.array([0.25, 0.5, 0.75, 0.999, 0.001])[rng.integers(0, 5, n)]
    grid = ((k + np.sign(k) * frac) / 32768.0).astype(np.float32)
    x[::3] = grid[::3]
    special = np.array([1.0, -1.0, 1.5, -1.5, 7.0, -7.0, -0.0, 0.0, 32767.0 / 32768.0, -32767.0 / 32768.0, 32767.5 / 32768.0,
                        -32767.5 / 32768.0, 0.5 / 32768.0, -0.5 / 32768.0, 0.99 / 32768.0, -0.99 / 32768.0, 1.0 / 32768.0,
                        -1.0 / 32768.0], np.float32)
    at = 7 + 37 * np.arange(len(special) * 3)
    x[at] = np.tile(special, 3)
    return x[None, :]


def expected_norm(samples, gain):
    """the int16 samples the reference makes of ``samples`` (int16 PCM or float32) under the linear ``gain``, in its own order of
    operations: /32768 (int16 only), float32 multiply by the gain, x 32768, clip to [-32768, 32767], truncation towards zero"""
    s = ofb.pcm16_to_float32(samples) if samples.dtype == np.int16 else np.array(samples, np.float32)
    if gain is not None:
        s = s * np.float32(gain)
    return ofb.float32_to_int16(s.astype(np.float32))


def oracle_norm(i16, target_db=-20):
    """the reference's dB-normalised int16 samples of one int16 utterance"""
    return ofb.float32_to_int16(ofb.db_normalize(ofb.pcm16_to_float32(i16), target_db))


# ---- truth, reference, domains -------------------------------------------------------------------------------------------------
def truth_and_reference(i16, kind='fbank', n_ceps=None):
    """(float64 truth, float32 reference) [T, 80] or [T, n_ceps] of ONE utterance of int16 samples"""
    i16 = np.asarray(i16)
    assert i16.dtype == np.int16 and i16.ndim == 1
    if kind == 'fbank':
        return ofb.kaldi_fbank(i16, 80, np.float64), ofb.kaldi_fbank(i16, 80, np.float32)
    assert kind == 'mfcc' and n_ceps is not None
    return ofb.kaldi_mfcc(i16, 80, n_ceps, np.float64), ofb.kaldi_mfcc(i16, 80, n_ceps, np.float32)


def batch_truth_and_reference(pcm, lens=None, kind='fbank', n_ceps=None):
    """the same for a padded batch [B, n_max] -> ([B, T_max, D] float64, float32, frame counts); zeros behind an utterance's frames"""
    B, n_max = pcm.shape
    lens = [n_max] * B if lens is None else [int(l) for l in lens]
    T, D = ofb.num_frames(n_max), 80 if kind == 'fbank' else n_ceps
    y64, y32 = np.zeros((B, T, D), np.float64), np.zeros((B, T, D), np.float32)
    counts = []
    for b in range(B):
        t, r = truth_and_reference(pcm[b, :lens[b]], kind, n_ceps)
        y64[b, :t.shape[0]], y32[b, :t.shape[0]] = t, r
        counts.append(t.shape[0])
    return y64, y32, counts


def peak_relative(y, y64):
    """log-mel rows -> mel energies over the TRUTH's largest energy of the same frame (truth, reference and candidate alike)"""
    y, y64 = np.asarray(y, np.float64), np.asarray(y64, np.float64)
    return np.exp(y - y64.max(axis=-1, keepdims=True))


# ---- a second float32 reference: the mel weights with a correctly rounded logarithm ----------------------------------------------------
# torchaudio's get_mel_banks evaluates mel(f) = 1127 * log(1 + f / 700) on float32 tensors.  No float32 ``log`` of a vector library
# is correctly rounded, and the libraries disagree in the last bit: numpy's (the oracle's) differs from the correctly rounded
# value at some 30 of the 256 bin frequencies.  One ulp of a mel value near 2000 - 2840 is 1.2e-4 - 2.4e-4; divided by the filter
# spacing of 34.7 mel it moves a tap weight by up to 1.4e-5, far more than the 6e-8 a weight's own rounding costs.  The float64
# truth takes the oracle's float32 weights as given, so a featurizer whose (equally legitimate) logarithm rounds the other way is
# 1e-5 of a weight "off" in some 60 of the 501 taps: in the peak-relative domain, where the strong bins are judged to a few
# 1e-7, that shows.  ``reference_rounded_log`` is the oracle's float32 evaluation with exactly that one change, and
# ``weights_spread`` how much further from the truth it is than the oracle's own float32 evaluation -- a figure of the
# reference side alone, the allowance of the one class that needs it (tests/test_gpu_frontend_budget.py).
def mel_banks_rounded_log(num_bins=80, padded=512, sample_freq=16000.0, low_freq=20.0):
    """``oracle.fbank.mel_banks`` in float32 with the logarithm of the bin frequencies correctly rounded (float64 log, rounded once)"""
    f32 = np.float32
    nyquist = 0.5 * sample_freq
    mel_low, mel_high = 1127.0 * math.log(1.0 + low_freq / 700.0), 1127.0 * math.log(1.0 + nyquist / 700.0)
    delta = (mel_high - mel_low) / (num_bins + 1)
    b = np.arange(num_bins, dtype=f32)[:, None]
    left, center, right = f32(mel_low) + b * f32(delta), f32(mel_low) + (b + f32(1.0)) * f32(delta), f32(mel_low) + (b + f32(2.0)) * f32(delta)
    freqs = f32(sample_freq / padded) * np.arange(padded // 2, dtype=f32)
    mel = (f32(1127.0) * np.log((f32(1.0) + freqs / f32(700.0)).astype(np.float64)).astype(f32))[None, :]
    bins = np.maximum(f32(0.0), np.minimum((mel - left) / (center - left), (right - mel) / (right - center))).astype(f32)
    return np.concatenate([bins, np.zeros((num_bins, 1), f32)], axis=1)


def fbank_f32_with_banks(i16, banks):
    """``oracle.fbank.kaldi_fbank(i16, 80, np.float32)`` restated with the mel weights as an argument (bit-identical to it with
    ``oracle.fbank.mel_banks()``: tests/test_frontend_ref_cpu.py)"""
    f32 = np.float32
    x = np.asarray(i16).astype(f32)
    m = ofb.num_frames(x.shape[0])
    if m == 0:
        return np.zeros((0, banks.shape[0]), f32)
    fr = x[np.arange(400)[None, :] + 160 * np.arange(m)[:, None]]
    fr = fr - fr.mean(axis=1, keepdims=True, dtype=f32)
    fr = fr - f32(0.97) * np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = np.concatenate([fr * ofb.povey_window(400, f32)[None, :], np.zeros((m, 112), f32)], axis=1)
    power = (np.abs(np.fft.rfft(fr, axis=1).astype(np.complex64)) ** 2).astype(f32)
    return np.log(np.maximum(power @ banks.astype(f32).T, ofb.EPS_F32)).astype(f32)


def reference_rounded_log(pcm):
    """[B, T, 80] float32: the second reference for a batch of full-length rows"""
    banks = mel_banks_rounded_log()
    return np.stack([fbank_f32_with_banks(row, banks) for row in pcm])


def weights_spread(t, r, r2):
    """max|r2 - t| / max(max|r - t|, ulp floor), at least 1: how much further from the truth ``t`` the second reference ``r2`` is
    than the first (all three in the domain of the case)"""
    t, r, r2 = (np.asarray(a, np.float64) for a in (t, r, r2))
    floor = 2.0 ** -23 * float(np.abs(t).max())
    return max(1.0, float(np.abs(r2 - t).max()) / max(float(np.abs(r - t).max()), floor))


# ---- one tone per mel filter -----------------------------------------------------------------------------------------------------
FILTERS = (0, 1, 17, 40, 57, 63) + tuple(range(64, 80))


def filter_bin(m):
    """the FFT bin nearest the centre of mel filter m"""
    mlo, delta = mel_edges()
    return int(np.clip(np.rint(mel_to_hz(mlo + (m + 1) * delta) / BIN_HZ), 1, 255))


def filter_tones(filters=FILTERS, n=720):
    """[len(filters), n] int16: row i is a tone at the centre bin of filter ``filters[i]`` (3 frames)"""
    return np.concatenate([tone(filter_bin(m) * BIN_HZ, n) for m in filters], axis=0)


def strongest_frame(y64):
    """index of the frame holding the largest float64 output of an utterance [T, 80]"""
    return int(np.argmax(y64.max(axis=-1)))


# ---- framing ---------------------------------------------------------------------------------------------------------------------
RAGGED_LENS = (0, 1, 399, 400, 401, 559, 560, 561, 720, 1041)
RAGGED_FRAMES = (0, 0, 0, 1, 1, 1, 2, 2, 3, 5)


def ragged_batch(n_max, lens=RAGGED_LENS, seed=41, garbage_seed=0):
    """[len(lens), n_max] int16: row b = ``synthetic_pcm`` up to lens[b]; behind it random int16 garbage drawn from
    ``garbage_seed`` (the valid samples do not depend on it)"""
    assert n_max >= max(lens)
    pcm = synthetic_pcm(len(lens), n_max, seed=seed)
    junk = np.random.default_rng(1000 + garbage_seed).integers(-32768, 32768, pcm.shape).astype(np.int16)
    for b, l in enumerate(lens):
        pcm[b, l:] = junk[b, l:]
    return pcm
