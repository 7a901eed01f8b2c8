"""CPU: the host-side plan of a device pass whose rows come at their own sample rates (masr_amd/data_utils/resample.py
``resampled_length`` / ``plan_rows`` / ``device_table``) -- the lengths the device resampler is told to produce must be the
lengths the host resampler produces, its errors the host's errors, and the grouping by rate must keep the rows in order."""
import numpy as np
import pytest

RATES = [(8000, 16000), (11025, 16000), (22050, 16000), (24000, 16000), (32000, 16000), (44100, 16000), (48000, 16000),
         (16000, 8000)]


@pytest.mark.parametrize('sr_in,sr_out', RATES)
def test_output_length_is_the_host_resamplers(sr_in, sr_out):
    from masr_amd.data_utils import resample as rs
    # (the length does not depend on the filter: the short one keeps 2 000 runs of the numpy form quick)
    for n in range(1, 2001):
        x = np.zeros(n, np.float32)
        if int(n * (float(sr_out) / sr_in)) < 1:
            with pytest.raises(ValueError):
                rs.resample(x, sr_in, sr_out, 'kaiser_fast')
            with pytest.raises(ValueError):
                rs.resampled_length(n, sr_in, sr_out)
        else:
            assert rs.resampled_length(n, sr_in, sr_out) == len(rs.resample(x, sr_in, sr_out, 'kaiser_fast')), n
    for n in (159999, 160000, 441000, 480001, 1234567):
        assert rs.resampled_length(n, sr_in, sr_out) == len(rs.resample(np.zeros(n, np.float32), sr_in, sr_out, 'kaiser_fast')), n


def test_too_short_row_raises_the_host_text():
    from masr_amd.data_utils import resample as rs
    for n, a, b in ((1, 48000, 16000), (2, 44100, 16000), (1, 16000, 8000)):
        with pytest.raises(ValueError) as host:
            rs.resample(np.zeros(n, np.float32), a, b)
        with pytest.raises(ValueError) as plan:
            rs.resampled_length(n, a, b)
        assert str(plan.value) == str(host.value) == f'Input signal length={n} is too small to resample from {a}->{b}'
        with pytest.raises(ValueError) as rows:
            rs.plan_rows([16000, n], [16000, a], b)
        assert str(rows.value) == str(host.value)
    with pytest.raises(ValueError, match='Invalid sample rate'):
        rs.resampled_length(10, 0, 16000)


def test_mixed_rate_grouping_preserves_row_order():
    from masr_amd.data_utils import resample as rs
    lengths = [8000, 44100, 16000, 8001, 48000, 16001, 44101, 8002]
    rates = [8000, 44100, 16000, 8000, 48000, 16000, 44100, 8000]
    n_out, groups = rs.plan_rows(lengths, rates, 16000)
    assert n_out == [len(rs.resample(np.zeros(n, np.float32), r, 16000, 'kaiser_fast')) if r != 16000 else n for n, r in zip(lengths, rates)]
    assert list(groups) == [8000, 44100, 16000, 48000]                   # one launch per distinct rate, in order of appearance
    assert groups == {8000: [0, 3, 7], 44100: [1, 6], 16000: [2, 5], 48000: [4]}
    assert sorted(i for rows in groups.values() for i in rows) == list(range(len(lengths)))
    assert rs.plan_rows([], [], 16000) == ([], {})
    with pytest.raises(ValueError):
        rs.plan_rows([1, 2], [8000], 16000)


@pytest.mark.parametrize('name', ['kaiser_best', 'kaiser_fast'])
def test_device_table_is_what_resample_native_prepares(name):
    from masr_amd.data_utils import resample as rs
    for sr_in, sr_out in ((48000, 16000), (8000, 16000)):
        pairs, num_table = rs.device_table(sr_in, sr_out, name)
        win, nt = rs.filter_table(name)
        ratio = float(sr_out) / sr_in
        if ratio < 1:
            win = ratio * win
        assert num_table == nt and pairs.dtype == np.float64 and pairs.shape == (win.shape[0], 2) and pairs.flags.c_contiguous
        assert np.array_equal(pairs[:, 0], win) and np.array_equal(pairs[:, 1], np.diff(win, append=win[-1]))
