"""Band-limited sinc interpolation with a Kaiser-windowed filter table (J. O. Smith's algorithm) -- the resampler behind the
reference's ``AudioSegment.resample`` (masr/data_utils/audio.py:306-317 -> ``resampy.resample(samples, sr, target, filter=
'kaiser_best')``; resampy is third-party, un-vendored (``requirements.txt:8``: ``resampy>=0.2.2``) and absent from this image).

Restated from resampy's PUBLISHED algorithm and filter parameters (resampy/core.py ``resample``, resampy/interpn.py
``_resample_loop``, resampy/filters.py ``sinc_window``; the shipped ``kaiser_best`` / ``kaiser_fast`` tables are
``sinc_window(num_zeros=64 | 16, precision=9, window=kaiser(beta=14.769656459379492 | 8.555504641634386),
rolloff=0.9475937167399596 | 0.85)``), regenerated here instead of loaded from resampy's data files.  **Parity unpinned**:
there is no resampy to compare with; the vectorised form below is pinned bit-for-bit against a loop-form restatement of the
same published algorithm (oracle/resample.py) and checked on band-limited tones.  Same output length as the reference:
``int(n * sr_new / sr_orig)``.  Host code: an input-format step in front of the hot path, not part of it.
"""
import functools

import numpy as np

FILTERS = {'kaiser_best': (64, 14.769656459379492, 0.9475937167399596),
           'kaiser_fast': (16, 8.555504641634386, 0.85)}
PRECISION = 9


@functools.lru_cache(maxsize=None)
def filter_table(name):
    """right wing of the windowed sinc, ``2**precision`` samples per zero crossing (resampy/filters.py sinc_window)"""
    if name not in FILTERS:
        raise NotImplementedError(f'unknown resampling filter {name!r} (kaiser_best | kaiser_fast)')
    num_zeros, beta, rolloff = FILTERS[name]
    num_bits = 2 ** PRECISION
    n = num_bits * num_zeros
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
    taper = np.kaiser(2 * n + 1, beta)[n:]            # == scipy.signal.windows.kaiser(2n + 1, beta), symmetric
    return taper * sinc_win, num_bits


def resample(x, sr_orig, sr_new, filter='kaiser_best'):
    """1-D float samples at ``sr_orig`` -> ``int(len(x) * sr_new / sr_orig)`` samples at ``sr_new``; every output is the sum,
    left wing then right wing, nearest tap first, of ``(win[j] + eta * dwin[j]) * x[.]`` accumulated in the dtype of ``x`` --
    the order of resampy's loop, one numpy pass per tap over all outputs."""
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError('resample: 1-D samples expected')
    if sr_orig <= 0 or sr_new <= 0:
        raise ValueError('Invalid sample rate')
    dtype = x.dtype if x.dtype.kind == 'f' else np.dtype(np.float32)
    ratio = float(sr_new) / sr_orig
    n_out = int(x.shape[0] * ratio)
    if n_out < 1:
        raise ValueError(f'Input signal length={x.shape[0]} is too small to resample from {sr_orig}->{sr_new}')
    win, num_table = filter_table(filter)
    if ratio < 1:
        win = ratio * win
    dwin = np.diff(win, append=win[-1])
    scale = min(1.0, ratio)
    index_step = int(scale * num_table)
    nwin, n_orig = win.shape[0], x.shape[0]
    t_reg = np.arange(n_out) * (1.0 / ratio)
    n = t_reg.astype(np.int64)
    xd = x.astype(np.float64)
    y = np.zeros(n_out, dtype)

    def wing(frac, first, step, count):
        # taps j = 0 .. count-1 of every output: weight from the table at offset + j * index_step, sample x[first + step * j]
        nonlocal y
        index_frac = frac * num_table
        offset = index_frac.astype(np.int64)
        eta = index_frac - offset
        for j in range(int(count.max(initial=0))):
            live = np.nonzero(j < count)[0]
            k = offset[live] + j * index_step
            w = win[k] + eta[live] * dwin[k]
            y[live] = (y[live].astype(np.float64) + w * xd[first[live] + step * j]).astype(dtype)

    frac = scale * (t_reg - n)
    offs = (frac * num_table).astype(np.int64)
    wing(frac, n, -1, np.minimum(n + 1, (nwin - offs) // index_step))
    frac = scale - frac
    offs = (frac * num_table).astype(np.int64)
    wing(frac, n + 1, 1, np.minimum(n_orig - n - 1, (nwin - offs) // index_step))
    return y


def resampled_length(n, sr_orig, sr_new):
    """samples that ``n`` samples at ``sr_orig`` give at ``sr_new``: ``int(n * ratio)`` with ``ratio = float(sr_new) / sr_orig``
    exactly as :func:`resample` evaluates it (NOT ``n * sr_new // sr_orig``: the float product may round across an integer);
    raises like :func:`resample` for bad rates and for a row too short to give one output sample"""
    if sr_orig <= 0 or sr_new <= 0:
        raise ValueError('Invalid sample rate')
    n_out = int(int(n) * (float(sr_new) / sr_orig))
    if n_out < 1:
        raise ValueError(f'Input signal length={int(n)} is too small to resample from {sr_orig}->{sr_new}')
    return n_out


def plan_rows(lengths, rates, target_rate):
    """host-side plan of a device pass whose rows come at their own sample rates: ``(n_out, groups)`` -- ``n_out[i]`` samples of
    row i at ``target_rate`` (its own length when it is there already, :func:`resampled_length` otherwise, raising like the host
    resampler), ``groups`` = {source rate: [row indices, ascending]} in order of first appearance: one device launch each"""
    if len(lengths) != len(rates):
        raise ValueError('plan_rows: one rate per row expected')
    n_out, groups = [], {}
    for i, (n, sr) in enumerate(zip(lengths, rates)):
        n_out.append(int(n) if sr == target_rate else resampled_length(n, sr, target_rate))
        groups.setdefault(sr, []).append(i)
    return n_out, groups


def device_table(sr_orig, sr_new, filter='kaiser_best'):
    """the filter as the device kernel reads it: ``(pairs [nwin, 2] float64 = (win[k], dwin[k]), num_table)``, prepared exactly
    as :func:`resample_native` prepares win / dwin (float64, scaled by the ratio when it is below 1, dwin = diff(win))"""
    ratio = float(sr_new) / sr_orig
    win, num_table = filter_table(filter)
    if ratio < 1:
        win = ratio * win
    win = np.ascontiguousarray(win, dtype=np.float64)
    dwin = np.diff(win, append=win[-1])
    return np.ascontiguousarray(np.stack([win, dwin], axis=1)), num_table


def resample_native(x, sr_orig, sr_new, filter='kaiser_best'):
    """the same algorithm through ``masr_resample_f32`` of libmasr_hip.so (host C++, operation for operation the arithmetic of
    :func:`resample`: bit-identical output, ~40x faster than the numpy tap loop); float32 in, float32 out"""
    import ctypes as C
    from .. import _lib
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 1:
        raise ValueError('resample: 1-D samples expected')
    if sr_orig <= 0 or sr_new <= 0:
        raise ValueError('Invalid sample rate')
    ratio = float(sr_new) / sr_orig
    n_out = int(x.shape[0] * ratio)
    if n_out < 1:
        raise ValueError(f'Input signal length={x.shape[0]} is too small to resample from {sr_orig}->{sr_new}')
    win, num_table = filter_table(filter)
    if ratio < 1:
        win = ratio * win
    win = np.ascontiguousarray(win, dtype=np.float64)
    dwin = np.ascontiguousarray(np.diff(win, append=win[-1]), dtype=np.float64)
    y = np.empty(n_out, np.float32)
    rc = _lib.lib().masr_resample_f32(x.ctypes.data_as(C.c_void_p), x.shape[0], ratio, win.ctypes.data_as(C.c_void_p),
                                      dwin.ctypes.data_as(C.c_void_p), win.shape[0], num_table, y.ctypes.data_as(C.c_void_p), n_out)
    if rc != 0:
        raise ValueError('masr_resample_f32 rejected its arguments')
    return y
