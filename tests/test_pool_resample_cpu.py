"""CPU: the host side of the streaming device resampler -- the new C-ABI symbols, ``masr_resample_plan`` (validation + tile list, no
GPU needed), the routing of ``StreamPool.feed`` (``serving.route_feed``) and the ``sample_rate`` of the server's feed calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'masr_resample_rate_fill': 5, 'masr_resample_tile_span': 1, 'masr_resample_plan': 12, 'masr_resample_feeds': 16,
       'masr_pool_set_rate': 7, 'masr_pool_step_rates': 17}


def test_new_symbols_are_declared_bound_and_exported(built_lib):
    from masr_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'masr_hip.h')).read(), flags=re.S)
    h = C.CDLL(built_lib)
    for name, n_args in NEW.items():
        m = re.search(r'\b%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S)
        assert m, f'{name} is not declared in include/masr_hip.h'
        assert len(m.group(1).split(',')) == n_args == len(_lib.SIGNATURES[name]), name
        assert hasattr(h, name), f'{name} is not exported'
    # masr_pool_step_rates is masr_pool_step with one more array in front of the gain evaluator
    old, new = _lib.SIGNATURES['masr_pool_step'], _lib.SIGNATURES['masr_pool_step_rates']
    assert new[:7] == old[:7] and new[8:] == old[7:]
    # the record layouts of the binding are the header's structs
    assert _lib.RESAMPLE_FEED.itemsize == 32 and _lib.RESAMPLE_RATE.itemsize == 48
    assert '#define MASR_RESAMPLE_TILE %d' % _lib.RESAMPLE_TILE in src and '#define MASR_RESAMPLE_LDS_FLOATS %d' % _lib.RESAMPLE_LDS_FLOATS in src


def _rate(lib, sr_in, sr_out, table):
    from masr_amd import _lib
    rec = np.zeros(1, _lib.RESAMPLE_RATE)
    rc = lib.masr_resample_rate_fill(float(sr_out) / sr_in, table.ctypes.data_as(C.c_void_p), 32769, 512, rec.ctypes.data_as(C.c_void_p))
    return rc, rec[0]


def _plan(lib, feeds, rates, src_bytes, rows, stride):
    n, bad, why = C.c_int64(), C.c_int32(), C.c_char_p()
    args = (feeds.ctypes.data_as(C.c_void_p), len(feeds), rates.ctypes.data_as(C.c_void_p), len(rates), src_bytes, rows, stride)
    rc = lib.masr_resample_plan(*args, None, 0, C.byref(n), C.byref(bad), C.byref(why))
    if rc:
        return rc, bad.value, (why.value or b'').decode(), None
    tiles = np.full((n.value, 2), -7, np.int32)
    assert lib.masr_resample_plan(*args, tiles.ctypes.data_as(C.c_void_p), n.value, C.byref(n), None, None) == 0
    return 0, -1, '', tiles


def test_plan_derives_what_the_host_loop_derives_and_tiles_every_output(built_lib):
    from masr_amd import _lib
    from masr_amd.data_utils import resample as rs
    lib = _lib.lib()
    table = np.zeros(4)                                                   # (only its address is recorded)
    rates = []
    for sr in (8000, 44100, 48000):
        rc, r = _rate(lib, sr, 16000, table)
        ratio = 16000.0 / sr
        assert rc == 0 and r['ratio'] == ratio and r['time_increment'] == 1.0 / ratio and r['scale'] == min(ratio, 1.0)
        assert r['index_step'] == int(min(ratio, 1.0) * 512) and r['nwin'] == 32769 and r['num_table'] == 512
        assert r['table_dev'] == table.ctypes.data
        span = lib.masr_resample_tile_span(C.c_void_p(np.array([r]).ctypes.data))
        assert span == int(255 * (1.0 / ratio)) + 2 * (32769 // int(r['index_step'])) + 4
        rates.append(r)
    rates = np.array(rates, _lib.RESAMPLE_RATE)
    assert _rate(lib, 16000, 0, table)[0] != 0 and _rate(lib, 16000 * 1024, 16000, table)[0] != 0     # ratio 0; index_step 0
    lens = [(0, 1, 0), (2, 3, 1), (1, 3, 0), (0, 128, 0), (0, 129, 1), (2, 765, 0), (1, 28224, 0), (0, 5120, 1)]
    feeds, at, off = [], 0, 0
    for slot, n_in, fmt in lens:
        n_out = rs.resampled_length(n_in, (8000, 44100, 48000)[slot], 16000)
        at = (at + 3) & ~3 if fmt else at
        feeds.append((at, fmt, n_in, n_out, 0, off, slot))
        at += n_in * (4 if fmt else 2)
        off += n_out
    feeds = np.array(feeds, _lib.RESAMPLE_FEED)
    assert feeds['n_out'].tolist() == [2, 1, 1, 256, 258, 255, 10240, 10240]
    rc, bad, why, tiles = _plan(lib, feeds, rates, at, 1, off)
    assert rc == 0 and bad == -1
    want = [(k, t0) for k, f in enumerate(feeds) for t0 in range(0, int(f['n_out']), 256)]
    assert tiles.tolist() == [list(t) for t in want] and len(want) == 1 + 1 + 1 + 1 + 2 + 1 + 40 + 40

    def refused(k, stride=off, src_bytes=at, n_rates=3, **kw):
        f = feeds.copy()
        for name, v in kw.items():
            f[name][k] = v
        rc, bad, why, _ = _plan(lib, f, rates[:n_rates], src_bytes, 1, stride)
        assert rc != 0 and bad == k, (kw, rc, bad, why)
        return why
    assert 'n_out' in refused(3, n_out=257) and 'n_out' in refused(3, n_out=255) and 'n_out' in refused(3, n_in=127)
    assert 'unknown rate slot' in refused(2, rate_slot=3) and 'unknown rate slot' in refused(2, rate_slot=-1)
    assert 'unknown rate slot' in refused(1, n_rates=2)                 # the first feed of the slot that is gone
    assert 'destination range' in refused(7, stride=off - 1) and 'destination range' in refused(0, dst_row=1)
    assert 'destination range' in refused(0, dst_offset=-1)
    assert 'source range' in refused(7, src_bytes=at - 1) and 'source range' in refused(4, src_offset=int(feeds['src_offset'][4]) + 2)
    assert 'source range' in refused(2, src_offset=int(feeds['src_offset'][2]) + 1) and 'format' in refused(1, format=2)
    bad_rates = rates.copy()
    bad_rates['time_increment'][1] *= 1.0 + 2.0 ** -50
    rc, bad, why, _ = _plan(lib, feeds, bad_rates, at, 1, off)
    assert rc != 0 and bad == -1 and 'bad rate' in why


def test_feed_routing_and_lengths():
    from masr_amd import serving
    from masr_amd.data_utils import resample as rs
    from masr_amd.data_utils.audio import AudioSegment
    pcm = (np.arange(1000) * 37 % 2000 - 1000).astype(np.int16)
    route = lambda a, ch=1, w=2, sr=8000, c=True, dev=True: serving.route_feed(a, ch, w, sr, 16000, c, dev)
    # wire PCM at the model's rate stays wire PCM on every framing
    for c in (True, False):
        for dev in (True, False):
            r = route(pcm.tobytes(), sr=16000, c=c, dev=dev)
            assert r[0] == 'wire' and np.array_equal(r[1], pcm)
    # off-rate: raw to the device, with the host resampler's own length, for every rate and chunk size
    for sr in (8000, 11025, 22050, 44100, 48000):
        for n in (1, 2, 3, 7, 160, 999, 1000):
            try:
                want = rs.resampled_length(n, sr, 16000)
            except ValueError as exc:
                with pytest.raises(ValueError) as got:
                    route(pcm[:n].tobytes(), sr=sr)
                assert str(got.value) == str(exc) == f'Input signal length={n} is too small to resample from {sr}->16000'
                continue
            kind, x, fmt, n_out = route(pcm[:n].tobytes(), sr=sr)
            assert (kind, fmt, n_out) == ('raw', 0, want) and x.dtype == np.int16 and np.array_equal(x, pcm[:n])
            assert n_out == len(rs.resample(np.zeros(n, np.float32), sr, 16000, 'kaiser_fast'))
    with pytest.raises(ValueError, match='Input signal length=0 is too small to resample from 8000->16000'):
        route(b'')
    with pytest.raises(ValueError, match='Invalid sample rate'):
        route(pcm.tobytes(), sr=0)
    assert route(bytearray(pcm.tobytes()))[0] == 'raw' and route(memoryview(pcm.tobytes()))[0] == 'raw'
    # arrays: int16 vectors as they are, everything else as the float32 mono samples AudioSegment makes of it
    kind, x, fmt, n_out = route(pcm)
    assert (kind, fmt, n_out) == ('raw', 0, 2000) and x.dtype == np.int16
    for arr in (pcm.astype(np.float32) / 32768, pcm.astype(np.float64) / 32768, pcm.astype(np.int32) << 16, np.stack([pcm, pcm[::-1]], 1)):
        kind, x, fmt, n_out = route(arr)
        assert (kind, fmt, n_out) == ('raw', 1, 2000) and x.dtype == np.float32 and x.flags.c_contiguous
        assert np.array_equal(x, AudioSegment.from_ndarray(arr, 8000).samples)
    with pytest.raises(TypeError):
        route(pcm.astype(np.uint8))
    # the host path keeps: multi-channel or non-16-bit bytes, arrays at the model's rate, the python framing, the switch at 0
    assert route(np.repeat(pcm, 2).tobytes(), ch=2) == ('host',) and route(pcm.astype('<i4').tobytes(), w=4) == ('host',)
    assert route(pcm, sr=16000) == ('host',) and route(pcm.astype(np.float32), sr=16000) == ('host',)
    assert route(pcm.tobytes(), c=False) == ('host',) and route(pcm.tobytes(), dev=False) == ('host',)
    assert route(pcm.astype(np.float32), c=False) == ('host',) and route('a string') == ('host',)


def test_device_resample_switch(monkeypatch):
    from masr_amd import serving
    monkeypatch.delenv('MASR_DEVICE_RESAMPLE', raising=False)
    assert serving.device_resample_enabled()
    monkeypatch.setenv('MASR_DEVICE_RESAMPLE', '0')
    assert not serving.device_resample_enabled()
    monkeypatch.setenv('MASR_DEVICE_RESAMPLE', '1')
    assert serving.device_resample_enabled()


class _Pool:
    """StreamPool interface: records what every feed was declared as"""

    def __init__(self):
        self.fed, self.errors, self._n = [], {}, 0

    def open(self):
        self._n += 1
        return self._n

    def close(self, handle):
        pass

    def feed(self, handle, data, is_end=False, **kw):
        self.fed.append((handle, len(data), is_end, kw))
        self._last = handle

    def step(self):
        return {self._last: {'text': str(len(self.fed)), 'score': 0.0}}


def test_worker_and_router_pass_the_sample_rate():
    from masr_amd.server import EngineWorker, WorkerRouter
    pools = [_Pool(), _Pool()]
    workers = [EngineWorker(None, p, max_batch=4, max_wait_ms=1.0) for p in pools]
    router = WorkerRouter(workers)
    try:
        a, b = router.stream_open().result(timeout=10), router.stream_open().result(timeout=10)
        assert router.stream_feed(a, b'1234').result(timeout=10)['text'] == '1'
        assert router.stream_feed(b, b'12', sample_rate=8000).result(timeout=10)['text'] == '1'
        assert router.stream_feed(a, b'123456', True, 8000).result(timeout=10)['text'] == '2'
    finally:
        router.shutdown()
    # a pool of another model rate: chunks AT that rate carry no keyword, and an empty final chunk (a client's b'end' alone) is
    # fed as it always was, whatever the wire rate -- no resampler takes zero samples
    pool8 = _Pool()
    pool8.sample_rate = 8000
    w = EngineWorker(None, pool8, max_batch=4, max_wait_ms=1.0)
    try:
        h = w.stream_open().result(timeout=10)
        w.stream_feed(h, b'12', False, 8000).result(timeout=10)
        w.stream_feed(h, b'1234').result(timeout=10)
        w.stream_feed(h, b'', True, 44100).result(timeout=10)
    finally:
        w.shutdown()
    assert pool8.fed == [(1, 2, False, {}), (1, 4, False, {'sample_rate': 16000}), (1, 0, True, {})]
    fed = sorted(p.fed for p in pools)
    assert sorted([fed[0], fed[1]], key=len) == [[(1, 2, False, {'sample_rate': 8000})],
                                                 [(1, 4, False, {}), (1, 6, True, {'sample_rate': 8000})]]
