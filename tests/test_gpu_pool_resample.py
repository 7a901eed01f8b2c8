"""GPU: off-rate streaming sessions resampled on the device inside the pool step (csrc/resample.hip resample_feeds_kernel,
masr_resample_feeds, masr_pool_set_rate / masr_pool_step_rates, StreamPool.feed) against the HOST resampler of libmasr_hip.so
(``masr_resample_f32`` through ``data_utils.resample.resample_native``).  The bar is ``np.array_equal`` on float32 bit patterns:
the kernel repeats the host arithmetic operation for operation, so there is no tolerance to grant."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
SENTINEL = np.int32(0x7fc12345)                      # a NaN payload no resampler writes


@pytest.fixture(scope='module')
def engine():
    from masr_amd.engine import HipEngine
    return HipEngine(None)


def _n_in_for(sr_in, sr_out, n_out):
    """the fewest input samples that give exactly ``n_out`` output samples"""
    n = 1
    while int(n * (float(sr_out) / sr_in)) < n_out:
        n += 1
    assert int(n * (float(sr_out) / sr_in)) == n_out, (sr_in, n_out)
    return n


def _launch_set(engine, spec, sr_out, seed, stride=None, gaps=None):
    """``spec``: rows of [(source rate, n_in, format)], placed from offset 3 of their row; ``gaps[r]``: samples left free behind
    every feed of row r (default 0: the feeds of a row land back to back) -> everything a launch needs and the host's answer per
    feed"""
    from masr_amd import _lib
    from masr_amd.data_utils import resample as rs
    rng = np.random.default_rng(seed)
    srs = sorted({f[0] for row in spec for f in row})
    rates = np.array([engine.resample_rate(sr, sr_out) for sr in srs], _lib.RESAMPLE_RATE)
    feeds, want, blob, at = [], [], bytearray(), 0
    for r, row in enumerate(spec):
        off = 3
        for j, (sr, n_in, fmt) in enumerate(row):
            pcm = rng.integers(-20000, 20000, n_in).astype(np.int16)
            flt = pcm.astype(np.float32) * np.float32(1.0 / 32768.0)
            raw = flt.tobytes() if fmt else pcm.tobytes()
            at = (at + 3) & ~3 if fmt else at                          # float32 feeds 4-byte aligned, int16 feeds wherever they land
            blob.extend(b'\0' * (at - len(blob)))
            y = rs.resample_native(flt, sr, sr_out)
            feeds.append((at, fmt, n_in, len(y), r, off, srs.index(sr)))
            want.append(y)
            blob.extend(raw)
            at += len(raw)
            off += len(y) + (gaps[r] if gaps else 0)
    feeds = np.array(feeds, _lib.RESAMPLE_FEED)
    stride = stride or int(max(f['dst_offset'] + f['n_out'] for f in feeds)) + 9
    src = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).to(engine.device)
    out = torch.from_numpy(np.full((len(spec) + 1, stride), SENTINEL, np.int32)).to(engine.device).view(torch.float32)
    return src, feeds, rates, out, want


def _check(out, feeds, want):
    host = out.cpu().numpy()
    bits = host.view(np.int32).copy()
    for f, w in zip(feeds, want):
        got = host[f['dst_row'], f['dst_offset']:f['dst_offset'] + f['n_out']]
        assert np.array_equal(got.view(np.int32), w.view(np.int32)), (tuple(f), int(np.sum(got.view(np.int32) != w.view(np.int32))))
        bits[f['dst_row'], f['dst_offset']:f['dst_offset'] + f['n_out']] = SENTINEL
    assert np.all(bits == SENTINEL), int(np.sum(bits != SENTINEL))      # nothing outside the feeds' own ranges was written


def test_feeds_kernel_one_launch_of_mixed_rates_equals_the_host_entry(engine):
    """8 / 11.025 / 44.1 / 48 kHz -> 16 kHz, int16 and float32, in ONE launch: the shortest feeds that give an output, a feed
    shorter than the filter wing, 255 / 256 / 257 outputs (the tile edge), 0.64 s feeds, two and three feeds back to back in a
    row, destination offsets that are no multiple of 4, int16 sources at 2-byte-aligned offsets"""
    spec = [[(48000, 3, 1), (8000, 1, 0), (11025, 1, 0)],                                        # 1, 2, 1 outputs, back to back
            [(44100, 3, 1), (8000, 20, 0)],                                                       # 1 output; shorter than a wing
            [(48000, _n_in_for(48000, 16000, 255), 0), (8000, _n_in_for(8000, 16000, 256), 1), (44100, _n_in_for(44100, 16000, 257), 0)],
            [(8000, 5120, 0), (48000, 30720, 1)],                                                 # 0.64 s
            [(44100, 28224, 0), (11025, 7057, 1), (8000, 333, 0)]]
    # rows 0 and 2: three feeds with no gap at all; row 1: two feeds back to back; rows 3 and 4: gaps that are no multiple of 4
    src, feeds, rates, out, want = _launch_set(engine, spec, 16000, 5, gaps=[0, 0, 0, 5, 7])
    ends = {(int(f['dst_row']), int(f['dst_offset'] + f['n_out'])) for f in feeds}
    starts = {(int(f['dst_row']), int(f['dst_offset'])) for f in feeds}
    both = [f for f in feeds if (int(f['dst_row']), int(f['dst_offset'])) in ends and (int(f['dst_row']), int(f['dst_offset'] + f['n_out'])) in starts]
    assert len(both) == 2 and {int(f['dst_row']) for f in both} == {0, 2}          # a neighbour abutting on BOTH sides
    assert sum((int(f['dst_row']), int(f['dst_offset'])) in ends for f in feeds) == 5   # rows 0, 2: two each; row 1: one
    assert [len(w) for w in want[:4]] == [1, 2, 1, 1] and [len(w) for w in want[5:8]] == [255, 256, 257]
    assert any(f['format'] == 0 and f['src_offset'] % 4 == 2 for f in feeds) and any(f['dst_offset'] % 4 for f in feeds)
    tiles = engine.resample_plan(feeds, rates, src.numel(), out.shape[0], out.shape[1])
    assert len(tiles) == sum(-(-int(f['n_out']) // 256) for f in feeds) and len(tiles) > len(feeds)
    lib = engine.lib
    assert all(0 < lib.masr_resample_tile_span(C.c_void_p(rates[j:j + 1].ctypes.data)) <= 16000 for j in range(len(rates)))
    engine.resample_feeds(src, feeds, rates, tiles, out)
    _check(out, feeds, want)


def test_feeds_kernel_reads_global_memory_beyond_the_lds_span(engine):
    """a downsampling ratio so small that a tile's inputs exceed the launcher's LDS budget (its own span computation says so):
    the kernel reads its inputs from global memory, same samples; a staged rate rides in the same launch"""
    from masr_amd import _lib
    spec = [[(16000, 40000, 0), (16000, 26000, 1)], [(8000, 700, 0)]]
    src, feeds, rates, out, want = _launch_set(engine, spec, 320, 6)
    spans = [engine.lib.masr_resample_tile_span(C.c_void_p(rates[j:j + 1].ctypes.data)) for j in range(len(rates))]
    assert spans[1] > _lib.RESAMPLE_LDS_FLOATS and 0 < spans[0] <= _lib.RESAMPLE_LDS_FLOATS, spans   # (8000, 16000) in slot order
    assert [len(w) for w in want] == [800, 520, 28]
    tiles = engine.resample_plan(feeds, rates, src.numel(), out.shape[0], out.shape[1])
    engine.resample_feeds(src, feeds, rates, tiles, out)
    _check(out, feeds, want)


def test_feeds_entry_refuses_before_it_launches(engine):
    from masr_amd._lib import MasrError
    spec = [[(8000, 600, 0), (48000, 900, 1)]]
    src, feeds, rates, out, _ = _launch_set(engine, spec, 16000, 7, stride=1600)
    tiles = engine.resample_plan(feeds, rates, src.numel(), out.shape[0], out.shape[1])

    def broken(k, **kw):
        f = feeds.copy()
        for name, v in kw.items():
            f[name][k] = v
        return f
    cases = [(broken(0, n_out=1201), 'n_out'), (broken(0, n_out=1199), 'n_out'),
             (broken(0, n_in=599), 'n_out'),                                                    # its last outputs would read past its input
             (broken(1, src_offset=int(feeds['src_offset'][1]) + 8), 'source range'),          # would read past the source buffer
             (broken(1, dst_offset=1301), 'destination range'), (broken(1, dst_row=2), 'destination range'),
             (broken(0, rate_slot=2), 'unknown rate slot'), (broken(0, rate_slot=-1), 'unknown rate slot'),
             (broken(0, src_offset=1), 'source range')]
    for f, what in cases:
        with pytest.raises(MasrError, match=what):
            engine.resample_feeds(src, f, rates, tiles, out)
    r2 = rates.copy()
    r2['ratio'][0] = 2.0 + 2.0 ** -40                                      # not what masr_resample_rate_fill derives
    with pytest.raises(MasrError, match='bad rate'):
        engine.resample_feeds(src, feeds, r2, tiles, out)
    with pytest.raises(MasrError, match='tile list'):
        engine.resample_feeds(src, feeds, rates, tiles[::-1].copy(), out)
    with pytest.raises(MasrError, match='tile list'):
        engine.resample_feeds(src, feeds, rates, tiles[:-1].copy(), out)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy().view(np.int32) == SENTINEL)            # nothing was launched
    engine.resample_feeds(src, feeds, rates, tiles, out)                    # and the unbroken call goes through
    torch.cuda.synchronize()
    assert np.any(out.cpu().numpy().view(np.int32) != SENTINEL)


# ---- the pool, end to end: device path against MASR_DEVICE_RESAMPLE=0 on a fresh pool -------------------------------------------
CONFIG = """
encoder_conf: {output_size: 256, attention_heads: 4, linear_units: 2048, num_blocks: 2, input_layer: conv2d,
  normalize_before: True, cnn_module_kernel: 15, use_cnn_module: True, activation_type: swish, pos_enc_layer_type: rel_pos}
preprocess_conf: {feature_method: fbank, n_mels: 80, n_mfcc: 40, sample_rate: 16000, use_dB_normalization: USE_DB, target_dB: -20}
dataset_conf: {dataset_vocab: VOCAB}
use_model: conformer
streaming: True
decoder: ctc_greedy
metrics_type: cer
"""
VOCAB = 96


@pytest.fixture(scope='module', params=[True, False], ids=['db_norm', 'no_db_norm'])
def predictor(request, tmp_path_factory):
    """a small random-weight streaming Conformer (2 blocks, 96 tokens); without dB normalisation a step has no wait before its
    windows, so the carried-over samples of an off-rate session return on another path"""
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    d = tmp_path_factory.mktemp('pool_resample')
    vpath = os.path.join(d, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(VOCAB):
            f.write(f'{t}\t1\n')
    cfg = yaml.safe_load(CONFIG.replace('VOCAB', vpath).replace('USE_DB', str(request.param)))
    return MASRPredictor(configs=cfg, use_gpu=True, state_dict=synthetic.conformer_state_dict(0, VOCAB, num_blocks=2))


@pytest.fixture(scope='module')
def audio():
    """the test recording at 16 kHz (int16), "recorded" at 8 kHz (int16) and at 48 kHz (float32) -- made once, on the host"""
    from masr_amd.data_utils import resample as rs
    pcm16 = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm'][:56000]
    x = pcm16.astype(np.float32) / np.float32(32768.0)
    as_pcm = lambda y: np.clip(np.rint(y * 32768.0), -32768, 32767).astype(np.int16)
    return {16000: pcm16, 8000: as_pcm(rs.resample_native(x, 16000, 8000)), 48000: rs.resample_native(x, 16000, 48000)}


def _cuts(total, sizes):
    """uneven chunk boundaries: the given sizes in turn, the rest in the last chunk"""
    at, out = 0, []
    for s in sizes:
        out.append((at, min(at + s, total)))
        at = min(at + s, total)
    out.append((at, total))
    return [c for c in out if c[1] > c[0]]


def _run(predictor, audio, lib_proxy=None):
    """four sessions in one pool over several steps -- 8 kHz int16 bytes, a 48 kHz float ndarray, 16 kHz wire PCM, and one that
    mixes 16 kHz and 8 kHz feeds inside a step -- then ``reset`` / ``close`` and a second utterance -> (per step: texts, packed
    host rows, handles that advanced), device-resampled feeds"""
    from masr_amd.serving import StreamPool
    pool = StreamPool(predictor)
    if lib_proxy is not None:
        pool._lib = lib_proxy(pool._lib)
    log = []

    def step(hs):
        out = pool.step()
        pk = pool._packed
        log.append(([out.get(h) for h in hs], None if pk is None else pk[4].copy(), None if pk is None else [hs.index(h) for h in pk[3]]))
    try:
        hs = [pool.open() for _ in range(4)]
        a8, a48, a16 = audio[8000], audio[48000], audio[16000]
        c8 = _cuts(len(a8), [1000, 2400, 5120, 777, 3001, 5120, 1])
        c48 = _cuts(len(a48), [30720, 4801, 15000, 30720, 3, 21000, 30720])
        c16 = _cuts(len(a16), [10240, 1600, 3333, 10240, 10240, 7, 10240])
        n = max(len(c8), len(c48), len(c16))
        for k in range(n):
            if k < len(c8):
                pool.feed(hs[0], a8[c8[k][0]:c8[k][1]].tobytes(), is_end=k == len(c8) - 1, sample_rate=8000)
            if k < len(c48):
                pool.feed(hs[1], a48[c48[k][0]:c48[k][1]].copy(), is_end=k == len(c48) - 1, sample_rate=48000)
            if k < len(c16):
                pool.feed(hs[2], a16[c16[k][0]:c16[k][1]].tobytes(), is_end=k == len(c16) - 1)
                # session 3: the same stretch of time, its first half at the model's rate and its second half from 8 kHz
                lo, hi = c16[k]
                mid = (lo + hi) // 2 & ~1
                pool.feed(hs[3], a16[lo:mid].tobytes()) if mid > lo else None
                if hi // 2 > mid // 2:
                    pool.feed(hs[3], a8[mid // 2:hi // 2].tobytes(), is_end=k == len(c16) - 1, sample_rate=8000)
            step(hs)
        # between utterances: one session reset, one closed and reopened; then 8 kHz again on both, 1 s + the rest
        pool.reset(hs[0])
        pool.close(hs[1])
        hs[1] = pool.open()
        for k, (lo, hi) in enumerate(_cuts(20000, [8000, 5120])):
            pool.feed(hs[0], a8[lo:hi].tobytes(), is_end=k == 2, sample_rate=8000)
            pool.feed(hs[1], a8[4000 + lo:4000 + hi].copy(), is_end=k == 2, sample_rate=8000)       # an int16 ndarray
            step(hs)
        return log, pool.device_resampled
    finally:
        pool.shutdown()


def _same(a, b):
    assert len(a) == len(b)
    for k, ((ta, ra, ha), (tb, rb, hb)) in enumerate(zip(a, b)):
        assert ta == tb and ha == hb, (k, ta, tb)
        assert (ra is None) == (rb is None) and (ra is None or (ra.shape == rb.shape and np.array_equal(ra, rb))), k


def test_pool_off_rate_sessions_equal_the_host_path(monkeypatch, predictor, audio):
    monkeypatch.delenv('MASR_DEVICE_RESAMPLE', raising=False)
    monkeypatch.delenv('MASR_POOL_PY', raising=False)
    dev, n_dev = _run(predictor, audio)
    monkeypatch.setenv('MASR_DEVICE_RESAMPLE', '0')
    host, n_host = _run(predictor, audio)                                   # a fresh pool on the same engine
    assert n_dev > 0 and n_host == 0
    _same(dev, host)
    texts = [t for step in dev for t in step[0] if t is not None]
    assert any(t['text'] for t in texts) and any(step[1] is not None for step in dev)
    # every session got partial results, off-rate ones included
    assert all(any(step[0][i] is not None for step in dev) for i in range(4))


def test_pool_python_framing_keeps_the_host_path(monkeypatch, predictor, audio):
    monkeypatch.delenv('MASR_DEVICE_RESAMPLE', raising=False)
    monkeypatch.setenv('MASR_POOL_PY', '1')
    from masr_amd.serving import StreamPool
    pool = StreamPool(predictor)
    try:
        h = pool.open()
        pool.feed(h, audio[8000][:12000].tobytes(), is_end=True, sample_rate=8000)
        py = pool.step()[h]
        assert pool.framing == 'python' and pool.device_resampled == 0
    finally:
        pool.shutdown()
    monkeypatch.delenv('MASR_POOL_PY')
    pool = StreamPool(predictor)
    try:
        h = pool.open()
        pool.feed(h, audio[8000][:12000].tobytes(), is_end=True, sample_rate=8000)
        c = pool.step()[h]
        assert pool.device_resampled == 1
        with pytest.raises(ValueError, match='Input signal length=2 is too small to resample from 48000->16000'):
            pool.feed(h, np.zeros(2, np.float32), sample_rate=48000)
        # stereo and 32-bit bytes go through the host resampler
        pool.reset(h)
        pool.feed(h, np.repeat(audio[8000][:12000], 2).tobytes(), is_end=True, channels=2, sample_rate=8000)
        stereo = pool.step()[h]
        assert pool.device_resampled == 1
    finally:
        pool.shutdown()
    assert py == c and py is not None and py['text']
    assert stereo is not None


def test_pool_at_the_models_rate_is_the_old_entry(monkeypatch, predictor, audio):
    """16 kHz only: ``masr_pool_step`` (what a pool without off-rate feeds still calls) and ``masr_pool_step_rates`` with every
    slot -1 return the same rows"""
    monkeypatch.delenv('MASR_DEVICE_RESAMPLE', raising=False)
    monkeypatch.delenv('MASR_POOL_PY', raising=False)
    calls = []

    class Proxy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            return getattr(self._lib, name)

        def masr_pool_step(self, *a):
            slots = np.full(a[1], -1, np.int32)
            calls.append(a[1])
            return self._lib.masr_pool_step_rates(*a[:7], slots.ctypes.data, *a[7:])
    only16 = {8000: audio[16000][::2].copy(), 48000: audio[16000].astype(np.float32) / np.float32(32768.0), 16000: audio[16000]}

    def run16(proxy):
        from masr_amd import serving
        real = serving.StreamPool.feed
        # every feed of the run declared at the model's rate
        monkeypatch.setattr(serving.StreamPool, 'feed', lambda self, h, d, is_end=False, sample_rate=16000, **kw: real(self, h, d, is_end, **kw))
        try:
            return _run(predictor, only16, proxy)
        finally:
            monkeypatch.setattr(serving.StreamPool, 'feed', real)
    old, n_old = run16(None)
    new, n_new = run16(Proxy)
    assert n_old == 0 and n_new == 0 and calls
    _same(old, new)
    assert any(t is not None and t['text'] for step in old for t in step[0])
