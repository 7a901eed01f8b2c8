"""GPU: off-rate audio resampled on the device (csrc/resample.hip, masr_resample_rows, HipEngine.resample_rows, the pass code of
MASRPredictor) against the HOST resampler.  The yardstick is ``masr_amd.data_utils.resample.resample`` -- the numpy form that
tests/test_host_logic.py pins bit for bit to oracle/resample.py and to the C loop -- never the device's own output.  The bar is
``np.array_equal`` on every row of every case: the kernel repeats the host arithmetic operation for operation, so there is no
tolerance to grant."""
import ctypes as C
import io
import os
import wave

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
RATES = [(8000, 16000), (11025, 16000), (22050, 16000), (24000, 16000), (32000, 16000), (44100, 16000), (48000, 16000),
         (16000, 8000)]
FILTERS = ['kaiser_best', 'kaiser_fast']


@pytest.fixture(scope='module')
def engine():
    from masr_amd.engine import HipEngine
    return HipEngine(None)


def _shortest_input(sr_in, sr_out, n_out):
    """the fewest input samples that give at least ``n_out`` output samples"""
    n = 1
    while int(n * (float(sr_out) / sr_in)) < n_out:
        n += 1
    return n


def _padded(rows, dtype):
    m = max(len(r) for r in rows)
    out = np.zeros((len(rows), m), dtype)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


@pytest.mark.parametrize('name', FILTERS)
@pytest.mark.parametrize('sr_in,sr_out', RATES)
def test_kernel_rows_equal_the_host_resampler(engine, sr_in, sr_out, name):
    """one ragged batch per (rate, filter): rows whose outputs are 1 sample (2 from 8 kHz, where one input sample gives two), fewer
    than one wing of the filter, a few hundred, and 10 s -- as int16 PCM and as the same samples in float32 -- scattered into the rows of a wider destination in another order;
    every row equals the host's, and everything behind a row's own length is exactly zero"""
    from masr_amd.data_utils import resample as rs
    rng = np.random.default_rng(sr_in + len(name))
    n_in = [_shortest_input(sr_in, sr_out, 1), _shortest_input(sr_in, sr_out, 11), 10 * sr_in, _shortest_input(sr_in, sr_out, 700) + 1]
    pcm = [rng.integers(-20000, 20000, n).astype(np.int16) for n in n_in]
    flt = [p.astype(np.float32) * np.float32(1.0 / 32768.0) for p in pcm]
    want = [rs.resample(x, sr_in, sr_out, name) for x in flt]
    shortest = max(1, sr_out // sr_in)
    lens = [len(w) for w in want]
    assert lens[0] == shortest and 11 <= lens[1] < 16 and lens[2] == 10 * sr_out        # 16: one wing of the shorter filter
    assert want[0].dtype == np.float32 and all(np.any(w != 0) for w in want)
    n_max = 10 * sr_out + 777
    dst_rows = [4, 0, 2, 5]
    for rows, dtype in ((pcm, np.int16), (flt, np.float32)):
        src = torch.from_numpy(_padded(rows, dtype)).to(engine.device)
        out = torch.full((6, n_max), float('nan'), dtype=torch.float32, device=engine.device)
        got, n_out = engine.resample_rows(src, n_in, sr_in, sr_out, filter=name, out=out, dst_rows=dst_rows)
        assert got is out and n_out.tolist() == [len(w) for w in want]
        host = out.cpu().numpy()
        for w, r in zip(want, dst_rows):
            assert np.array_equal(host[r, :len(w)], w), (sr_in, name, dtype, r, int(np.sum(host[r, :len(w)] != w)))
            assert not np.any(host[r, len(w):]), (sr_in, name, dtype, r)                 # (also: no -0.0 -- any() is False for it,
            assert not np.any(np.signbit(host[r, len(w):]))                                #  so the sign is checked on its own)
        assert np.all(np.isnan(host[[1, 3]]))                                              # rows nobody was sent to are untouched
    # default destination: a new [R, longest output] buffer, rows in order
    src = torch.from_numpy(_padded(flt[:2], np.float32)).to(engine.device)
    out, n_out = engine.resample_rows(src, n_in[:2], sr_in, sr_out, filter=name)
    assert out.shape == (2, lens[1]) and n_out.tolist() == lens[:2]
    host = out.cpu().numpy()
    assert np.array_equal(host[0, :shortest], want[0]) and not np.any(host[0, shortest:]) and np.array_equal(host[1], want[1])


@pytest.mark.parametrize('name', FILTERS)
@pytest.mark.parametrize('sr_in,sr_out', [(48000, 16000), (44100, 16000), (8000, 16000), (16000, 8000)])
def test_no_contraction_and_denormals_kept(engine, sr_in, sr_out, name):
    """a float32 row scaled by 2^-120: inputs next to the smallest normal float32, outputs below it.  A kernel built with fused
    multiply-adds, or one that flushes float32 denormals, does not reproduce the host here; the fix for a failure is the build
    flags of resample.hip (masr_amd/build.py), not this test."""
    from masr_amd.data_utils import resample as rs
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(3 * sr_in).astype(np.float32) * np.float32(0.2)) * np.float32(2.0 ** -120)
    want = rs.resample(x, sr_in, sr_out, name)
    tiny = np.finfo(np.float32).tiny
    assert np.any(want != 0) and np.any((want != 0) & (np.abs(want) < tiny))             # not vacuous: denormal outputs exist
    out, n_out = engine.resample_rows(torch.from_numpy(x[None]).to(engine.device), [len(x)], sr_in, sr_out, filter=name)
    got = out.cpu().numpy()[0]
    assert int(n_out[0]) == len(want) and np.any(got != 0)
    assert np.array_equal(got, want), int(np.sum(got != want))
    # and at full scale, where a fused weight or a fused accumulation moves single bits
    x1 = rng.standard_normal(3 * sr_in).astype(np.float32) * np.float32(0.2)
    out, _ = engine.resample_rows(torch.from_numpy(x1[None]).to(engine.device), [len(x1)], sr_in, sr_out, filter=name)
    assert np.array_equal(out.cpu().numpy()[0], rs.resample(x1, sr_in, sr_out, name))


def test_rows_at_the_target_rate_are_converted_and_copied(engine):
    rng = np.random.default_rng(3)
    pcm = [rng.integers(-32768, 32767, n).astype(np.int16) for n in (1, 5000, 31999)]
    src = torch.from_numpy(_padded(pcm, np.int16)).to(engine.device)
    out = torch.full((3, 32100), float('nan'), dtype=torch.float32, device=engine.device)
    engine.resample_rows(src, [len(p) for p in pcm], 16000, 16000, out=out, dst_rows=[2, 1, 0])
    host = out.cpu().numpy()
    for p, r in zip(pcm, [2, 1, 0]):
        assert np.array_equal(host[r, :len(p)], p.astype(np.float32) * np.float32(1.0 / 32768.0)) and not np.any(host[r, len(p):])


def test_entry_point_refuses_what_the_host_loop_refuses(engine):
    """masr_resample_rows returns an error (masr_last_error) where masr_resample_f32 returns 1, before anything is launched"""
    from masr_amd import _lib
    from masr_amd.data_utils import resample as rs
    src = torch.zeros(1, 3000, dtype=torch.float32, device=engine.device)
    out = torch.zeros(1, 4000, dtype=torch.float32, device=engine.device)
    table, num_table = engine.resample_table(48000, 16000)

    def call(n_in, n_out, ratio, row=0, tab=table):
        rows = np.array([[n_in, n_out, row]], np.int32)
        rows_dev = engine.to_device(rows)
        return engine.lib.masr_resample_rows(engine.h, C.c_void_p(src.data_ptr()), 1, 3000, rows.ctypes.data_as(C.c_void_p),
                                             C.c_void_p(rows_dev.data_ptr()), 1, ratio, C.c_void_p(tab.data_ptr()) if tab is not None else None,
                                             table.shape[0], num_table, C.c_void_p(out.data_ptr()), 1, 4000,
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(3000, 1000, 1.0 / 3.0) == 0
    # the host entry on the same arguments: accepted / refused alike
    win = np.ascontiguousarray(table.cpu().numpy()[:, 0])
    dwin = np.ascontiguousarray(table.cpu().numpy()[:, 1])

    def host(n_in, n_out, ratio):
        x, y = np.zeros(n_in, np.float32), np.zeros(max(n_out, 1), np.float32)
        return _lib.lib().masr_resample_f32(x.ctypes.data_as(C.c_void_p), n_in, ratio, win.ctypes.data_as(C.c_void_p),
                                            dwin.ctypes.data_as(C.c_void_p), win.shape[0], num_table, y.ctypes.data_as(C.c_void_p), n_out)
    assert host(3000, 1000, 1.0 / 3.0) == 0
    for n_in, n_out, ratio, what in ((3000, 1000, 0.0, 'ratio'), (3000, 1000, -1.0, 'ratio'), (3000, 1, 1.0 / 1024.0, 'index_step'),
                                     (3000, 1001, 1.0 / 3.0, 'n >= n_orig'), (30, 1000, 1.0 / 3.0, 'n >= n_orig')):
        assert host(n_in, n_out, ratio) == 1, what
        assert call(n_in, n_out, ratio) != 0, what
        assert what.split()[0] in engine.lib.masr_last_error().decode(), (what, engine.lib.masr_last_error())
    assert call(3000, 1000, 1.0 / 3.0, row=1) != 0 and call(3001, 1000, 1.0 / 3.0) != 0 and call(3000, 4001, 2.0) != 0
    assert call(3000, 1000, 1.0 / 3.0, tab=None) != 0                                    # no table: ratio 1 only
    with pytest.raises(ValueError, match='Input signal length=2 is too small to resample from 48000->16000'):
        engine.resample_rows(src[:, :2].contiguous(), [2], 48000, 16000)
    assert engine.resample_table(48000, 16000)[0] is table                               # uploaded once per (ratio, filter)
    assert engine.resample_table(48000, 16000, 'kaiser_fast')[0] is not table
    torch.cuda.synchronize()


# ---- facade: the device path against MASR_DEVICE_RESAMPLE=0 (the host path of the parent commit) -------------------------------
CONFIG = """
encoder_conf: {output_size: 256, attention_heads: 4, linear_units: 2048, num_blocks: 12, dropout_rate: 0.1,
  positional_dropout_rate: 0.1, attention_dropout_rate: 0.1, input_layer: conv2d, normalize_before: True,
  cnn_module_kernel: 15, use_cnn_module: True, activation_type: swish, pos_enc_layer_type: rel_pos}
preprocess_conf: {feature_method: fbank, n_mels: 80, n_mfcc: 40, sample_rate: 16000, use_dB_normalization: True, target_dB: -20}
dataset_conf: {dataset_vocab: VOCAB}
use_model: conformer
streaming: True
decoder: ctc_greedy
metrics_type: cer
"""


@pytest.fixture(scope='module')
def predictor(tmp_path_factory):
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    d = tmp_path_factory.mktemp('resample_facade')
    vpath = os.path.join(d, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(4233):
            f.write(f'{t}\t1\n')
    cfg = yaml.safe_load(CONFIG.replace('VOCAB', vpath))
    mpath = os.path.join(d, 'model.pt')
    torch.save(synthetic.conformer_state_dict(0, 4233), mpath)
    return MASRPredictor(configs=cfg, model_path=mpath, use_gpu=True)


@pytest.fixture(scope='module')
def speech():
    """the test recording (16 kHz int16) as float32"""
    return np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm'].astype(np.float32) / np.float32(32768.0)


def _recorded_at(x16, rate):
    """an utterance "recorded" at ``rate``: float32 samples at that rate"""
    from masr_amd.data_utils import resample as rs
    return rs.resample_native(x16, 16000, rate).astype(np.float32)


def _as_pcm(x):
    return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)


def _wav(pcm16, rate):
    b = io.BytesIO()
    with wave.open(b, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm16.tobytes())
    return b.getvalue()


def _norm_rows(predictor, audio_list, sample_rate):
    """the audio as ONE pass through the facade's own preparation, then the normalised int16 samples the feature front-end
    makes of it (``fbank_batch(return_norm=True)``): what the encoder's features are computed from, row by row"""
    eng = predictor.predictor.engine
    pc = predictor.configs.preprocess_conf
    began = predictor._begin_pass([predictor._load_audio(a, sample_rate) for a in audio_list])
    xs, ns, gain = predictor._prepare_finish(began['prep'], pc.target_dB)
    _, _, norm = eng.fbank_batch(xs, ns, pc.use_dB_normalization, pc.target_dB, return_norm=True, gain_in=gain)
    torch.cuda.synchronize()
    norm, n = norm.cpu().numpy(), began['n']
    assert not np.any(norm[np.arange(norm.shape[1])[None, :] >= n[:, None]])            # zero padding behind every row
    return began['ok'], [norm[j, :n[j]].copy() for j in range(len(n))]


def _both_ways(monkeypatch, predictor, run):
    """``run()`` with the device path and with MASR_DEVICE_RESAMPLE=0 -> (device result, host result, device launches)"""
    eng = predictor.predictor.engine
    calls = []
    real = eng.resample_rows
    monkeypatch.setattr(eng, 'resample_rows', lambda *a, **k: (calls.append(a[2]), real(*a, **k))[1])
    monkeypatch.delenv('MASR_DEVICE_RESAMPLE', raising=False)
    on = run()
    launched = list(calls)
    monkeypatch.setenv('MASR_DEVICE_RESAMPLE', '0')
    off = run()
    assert len(calls) == len(launched), 'MASR_DEVICE_RESAMPLE=0 must restore the host path'
    monkeypatch.delenv('MASR_DEVICE_RESAMPLE', raising=False)
    return on, off, launched


def _same_norm(monkeypatch, predictor, audio_list, sample_rate):
    on, off, launched = _both_ways(monkeypatch, predictor, lambda: _norm_rows(predictor, audio_list, sample_rate))
    assert on[0] == off[0] and len(on[1]) == len(off[1]) > 0 and launched
    for j, (a, b) in enumerate(zip(on[1], off[1])):
        assert a.dtype == np.int16 and np.array_equal(a, b), (j, int(np.sum(a != b)) if a.shape == b.shape else (a.shape, b.shape))


def test_facade_32_utterances_at_48k(monkeypatch, predictor, speech):
    lens = np.linspace(24000, 64000, 32).astype(int)
    audio = [_recorded_at(speech[(7 * i) % 50: (7 * i) % 50 + n], 48000) for i, n in enumerate(lens)]
    on, off, launched = _both_ways(monkeypatch, predictor, lambda: predictor.predict_batch(audio, sample_rate=48000))
    assert on == off and len(on) == 32 and any(r['text'] for r in on), (on, off)
    assert launched == [48000]                                                           # one launch for the pass's one rate
    _same_norm(monkeypatch, predictor, audio, 48000)


def test_facade_pass_mixing_rates_and_sample_types(monkeypatch, predictor, speech):
    audio = [_wav(_as_pcm(_recorded_at(speech[:50000], 8000)), 8000),                    # 8 kHz int16 PCM
             _recorded_at(speech[10000:70000], 44100),                                   # 44.1 kHz float32
             _wav(_as_pcm(speech[20000:75000]), 16000),                                  # 16 kHz PCM, already at the model's rate
             _wav(_as_pcm(_recorded_at(speech[5000:45000], 8000)), 8000),
             _wav(_as_pcm(_recorded_at(speech[:3], 8000)), 8000)]                        # too short for one frame: set aside
    on, off, launched = _both_ways(monkeypatch, predictor, lambda: predictor.predict_batch(audio, sample_rate=44100))
    assert on == off and len(on) == 5 and on[4] == {'text': '', 'score': 0} and any(r['text'] for r in on[:4]), (on, off)
    assert sorted(launched) == [8000, 16000, 44100]                                      # one launch per distinct source rate
    _same_norm(monkeypatch, predictor, audio, 44100)
    # every row alone gives what it gives alone on the host path (a batch of one has no padding to differ by)
    for a in audio[:4]:
        one_on, one_off, _ = _both_ways(monkeypatch, predictor, lambda: predictor.predict(a, sample_rate=44100))
        assert one_on == one_off
    with pytest.raises(ValueError, match='Input signal length=2 is too small to resample from 48000->16000'):
        predictor.predict_batch([np.zeros(2, np.float32), audio[1]], sample_rate=48000)


def test_facade_balanced_passes_on_two_lanes(monkeypatch, predictor, speech):
    lens = np.linspace(20000, 60000, 24).astype(int)
    audio = [_as_pcm(_recorded_at(speech[1000 + 11 * i: 1000 + 11 * i + n], 8000)) for i, n in enumerate(lens)]
    monkeypatch.setenv('MASR_LANES', '2')
    run = lambda: predictor.predict_batch(audio, sample_rate=8000, batch_size='balanced', pass_padded=6 * 60000)
    on, off, launched = _both_ways(monkeypatch, predictor, run)
    assert on == off and len(on) == 24 and any(r['text'] for r in on), (on, off)
    assert len(launched) >= 3 and set(launched) == {8000}                                # several passes: both lanes take turns
    _same_norm(monkeypatch, predictor, audio, 8000)


def test_facade_deferred_with_two_handles_in_flight(monkeypatch, predictor, speech):
    a = [_as_pcm(_recorded_at(speech[i * 3000: i * 3000 + 48000], 8000)) for i in range(4)]
    b = [_recorded_at(speech[i * 2000: i * 2000 + 40000], 44100) for i in range(3)]

    def run():
        ha = predictor.predict_batch_deferred(a, sample_rate=8000)
        hb = predictor.predict_batch_deferred(b, sample_rate=44100)                      # launched before the first is collected
        return ha(), hb()
    on, off, launched = _both_ways(monkeypatch, predictor, run)
    assert on == off and [len(r) for r in on] == [4, 3] and any(r['text'] for part in on for r in part), (on, off)
    assert launched == [8000, 44100]
    _same_norm(monkeypatch, predictor, a, 8000)
    _same_norm(monkeypatch, predictor, b, 44100)


def test_facade_predict_long_on_an_8k_recording(monkeypatch, predictor, speech):
    from masr_amd.data_utils import resample as rs
    from masr_amd.data_utils.audio import AudioSegment
    from masr_amd.infer_utils.vad_predictor import EnergyVAD
    x16 = np.concatenate([speech, np.zeros(8000, np.float32), speech[::-1], np.zeros(4000, np.float32), speech[:70000]])
    rec = _as_pcm(_recorded_at(x16, 8000))
    run = lambda: predictor.predict_long(rec.copy(), sample_rate=8000, vad_predictor=EnergyVAD(), batch_size=8)
    on, off, launched = _both_ways(monkeypatch, predictor, run)
    assert on == off and on['text'], (on, off)
    assert launched[0] == 8000                                                           # the recording itself, as one long row
    # the recording the VAD reads: the device's single long row is the host's, sample for sample
    got = predictor._resample_long(AudioSegment.from_ndarray(rec.copy(), 8000), 16000)
    want = rs.resample(rec.astype(np.float32) * np.float32(1.0 / 32768.0), 8000, 16000)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    _same_norm(monkeypatch, predictor, [rec], 8000)
