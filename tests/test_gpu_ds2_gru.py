"""GPU: DeepSpeech2 with ``encoder_conf.use_gru: True`` (nn.GRU recurrent layers, gru.hip) against fixtures recorded from the
REAL reference (tools/make_ds2_gru_golden.py) and against torch.nn.GRU on the CPU with the same weights.

Bars as for the LSTM (test_gpu_parity.py::test_deepspeech2_against_reference_fixture): probabilities to 1e-3, argmax agreement
> 0.995 on valid frames, facade transcripts equal to the reference facade's."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
ENC_CONF = {'num_rnn_layers': 5, 'rnn_size': 1024, 'use_gru': True}


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


@pytest.fixture(scope='module')
def gru_engines():
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sd_bi = synthetic.deepspeech2_state_dict(0, 300, bidirectional=True, use_gru=True)
    sd_uni = synthetic.deepspeech2_state_dict(0, 300, bidirectional=False, use_gru=True)
    e_bi = HipEngine(sd_bi, encoder_conf=ENC_CONF, streaming=False, use_model='deepspeech2')
    e_uni = HipEngine(sd_uni, encoder_conf=ENC_CONF, streaming=True, use_model='deepspeech2')
    yield e_bi, e_uni, sd_bi, sd_uni
    e_bi.close()
    e_uni.close()


@torch.no_grad()
def cpu_probs(sd, feats, lens):
    """oracle conv front-end, then per layer torch.nn.GRU over the packed sequence and LayerNorm, then the CTC softmax"""
    from oracle import deepspeech2 as ods
    x, xl = ods.conv_frontend(sd, feats, lens)
    bi = 'encoder.rnns.0.rnn.rnn.weight_ih_l0_reverse' in sd
    H = sd['encoder.rnns.0.rnn.rnn.weight_hh_l0'].shape[1]
    i = 0
    while f'encoder.rnns.{i}.layer_norm.weight' in sd:
        p = f'encoder.rnns.{i}.rnn.rnn.'
        gru = torch.nn.GRU(x.shape[-1], H, num_layers=1, batch_first=True, bidirectional=bi)
        gru.load_state_dict({k[len(p):]: v for k, v in sd.items() if k.startswith(p)})
        packed = torch.nn.utils.rnn.pack_padded_sequence(x, xl, batch_first=True, enforce_sorted=False)
        y, _ = gru(packed)
        x, _ = torch.nn.utils.rnn.pad_packed_sequence(y, batch_first=True)
        x = F.layer_norm(x, (x.shape[-1],), sd[f'encoder.rnns.{i}.layer_norm.weight'], sd[f'encoder.rnns.{i}.layer_norm.bias'], 1e-5)
        i += 1
    return torch.softmax(F.linear(x, sd['decoder.ctc_lo.weight'], sd['decoder.ctc_lo.bias']), dim=2), xl


def test_gru_against_reference_fixture(gru_engines):
    from oracle.make_golden import golden_inputs
    e_bi, e_uni, _, _ = gru_engines
    z = np.load(os.path.join(GOLDEN, 'deepspeech2_gru_v300.npz'))
    feats, lens = golden_inputs()
    for e, key in ((e_bi, 'bi_probs'), (e_uni, 'uni_probs')):
        enc = e.encode_full(dev(feats), dev(lens, torch.int32))
        probs = e.ctc_probs(enc).cpu().numpy()
        ref = z[key]                                   # [3, 82, 300]; padded rows of the shorter utterances included
        assert probs.shape == ref.shape
        assert np.abs(probs - ref).max() < 1e-3, (key, np.abs(probs - ref).max())
        valid = [82, 49, 23]
        for b in range(3):
            assert (probs[b, :valid[b]].argmax(-1) == ref[b, :valid[b]].argmax(-1)).mean() > 0.995
        idx, mp = e.ctc_greedy_frames(enc)
        assert np.array_equal(idx.cpu().numpy(), probs.argmax(-1))
        np.testing.assert_allclose(mp.cpu().numpy(), probs.max(-1), atol=1e-6)


# B = 1, 3: wave-per-unit form; 8: matrix-core form, one sequence tile; 20: two tiles; 40: wave form past 32.
# units = 16: the matrix-core form on three full 16-column tiles (masr_debug_set key 43) instead of the default 8 units.
@pytest.mark.parametrize('B,units', [(1, 8), (3, 8), (8, 8), (20, 8), (40, 8), (8, 16), (20, 16)])
def test_gru_step_forms_ragged_against_torch_gru(gru_engines, B, units):
    from masr_amd._lib import debug_keys
    e_bi, e_uni, sd_bi, sd_uni = gru_engines
    torch.manual_seed(100 + B)
    T = 131
    lens = torch.randint(40, T + 1, (B,))
    lens[B // 2] = T
    x = (torch.randn(B, T, 80) * 3 + 13) * (torch.arange(T)[None, :, None] < lens[:, None, None])
    for e, sd in ((e_bi, sd_bi), (e_uni, sd_uni)):
        with debug_keys(e, rnn_mfma_units=units):
            probs = e.ctc_probs(e.encode_full(dev(x), dev(lens, torch.int32))).cpu()
        ref, xl = cpu_probs(sd, x, lens)
        n = ref.shape[1]                                       # pad_packed_sequence trims to the longest sequence
        assert probs.shape[0] == B and probs.shape[1] >= n
        err = (probs[:, :n] - ref).abs().max().item()
        assert err < 1e-3, (B, units, err)
        for b in range(B):
            k = int(xl[b])
            assert (probs[b, :k].argmax(-1) == ref[b, :k].argmax(-1)).float().mean().item() > 0.995


def test_gru_stream_chunks_against_reference_fixture(gru_engines):
    from oracle.make_golden import golden_inputs
    _, e, _, sd = gru_engines
    z = np.load(os.path.join(GOLDEN, 'deepspeech2_gru_v300.npz'))
    feats, _ = golden_inputs()
    sid = e.stream_open(0)
    for i, cur in enumerate(range(0, 331 - 67 + 1, 64)):
        probs, _, _ = e.encode_chunk([sid], dev(feats[:1, cur:cur + 67]))
        assert np.abs(probs[0].cpu().numpy() - z['chunk_probs'][i]).max() < 1e-3
    h, c = e.stream_export_cache(sid)
    assert np.abs(h.cpu().numpy() - z['h']).max() < 1e-3
    assert torch.equal(h, c)                     # gru.py: final_state_c = final_state_h
    e.stream_reset(sid)
    p0, _, _ = e.encode_chunk([sid], dev(feats[:1, :67]))
    assert np.abs(p0[0].cpu().numpy() - z['chunk_probs'][0]).max() < 1e-3
    e.stream_close(sid)
    # two interleaved streams with different audio == each one alone
    torch.manual_seed(11)
    xa = torch.randn(1, 195, 80) * 3 + 13
    xb = torch.randn(1, 195, 80) * 3 + 13
    alone = []
    for xx in (xa, xb):
        s = e.stream_open(0)
        alone.append([e.encode_chunk([s], dev(xx[:, cur:cur + 67]))[0][0].cpu() for cur in (0, 64, 128)])
        e.stream_close(s)
    s0, s1 = e.stream_open(0), e.stream_open(0)
    for k, cur in enumerate((0, 64, 128)):
        probs, _, _ = e.encode_chunk([s0, s1], dev(torch.cat([xa[:, cur:cur + 67], xb[:, cur:cur + 67]])))
        assert (probs[0].cpu() - alone[0][k]).abs().max().item() < 1e-5
        assert (probs[1].cpu() - alone[1][k]).abs().max().item() < 1e-5
    e.stream_close(s0)
    e.stream_close(s1)


def test_gru_cell_mismatch_is_refused(monkeypatch):
    from masr_amd import _lib, engine as eng_mod
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    gru = synthetic.deepspeech2_state_dict(0, 50, num_rnn_layers=1, bidirectional=False, use_gru=True)
    lstm = synthetic.deepspeech2_state_dict(0, 50, num_rnn_layers=1, bidirectional=False)
    conf = {'num_rnn_layers': 1, 'rnn_size': 1024}
    for sd, flag in ((gru, False), (lstm, True)):
        with pytest.raises(_lib.MasrError, match='use_gru'):
            HipEngine(sd, encoder_conf=dict(conf, use_gru=flag), streaming=True, use_model='deepspeech2')
    # the engine itself refuses as well, not only the Python check in front of it
    monkeypatch.setattr(eng_mod, '_validate_encoder_conf', lambda *a: None)
    for sd, flag in ((gru, False), (lstm, True)):
        with pytest.raises(_lib.MasrError, match='use_gru'):
            HipEngine(sd, encoder_conf=dict(conf, use_gru=flag), streaming=True, use_model='deepspeech2')
    with pytest.raises(_lib.MasrError, match='reserved'):
        HipEngine(gru, encoder_conf=dict(conf, use_gru=2), streaming=True, use_model='deepspeech2')


# ---------------------------------------------------------------------------------------------------
# the facade: MASRPredictor / StreamPool over a GRU checkpoint (fixture: predictor_deepspeech2_gru.npz)
# ---------------------------------------------------------------------------------------------------
DS2_GRU_CONFIG = """
encoder_conf: {num_rnn_layers: 5, rnn_size: 1024, use_gru: True}
preprocess_conf: {feature_method: fbank, n_mels: 80, n_mfcc: 40, sample_rate: 16000, use_dB_normalization: True, target_dB: -20}
dataset_conf: {dataset_vocab: VOCAB}
use_model: deepspeech2
streaming: STREAMING
decoder: ctc_greedy
metrics_type: cer
"""


def _predictor(d, streaming):
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    vpath = os.path.join(d, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(4233):
            f.write(f'{t}\t1\n')
    cfg = yaml.safe_load(DS2_GRU_CONFIG.replace('VOCAB', vpath).replace('STREAMING', str(streaming)))
    sd = synthetic.deepspeech2_state_dict(0, 4233, bidirectional=not streaming, use_gru=True)
    mpath = os.path.join(d, f'model_gru_{streaming}.pt')
    torch.save(sd, mpath)
    return MASRPredictor(configs=cfg, model_path=mpath, use_gpu=True)


def _same(ref_text, text, ref_score, score, what):
    """exact transcripts where this host's numpy reproduces the fixture's normalisation gain (as test_gpu_facade.py::_same)"""
    from masr_amd.engine import reference_gains
    from oracle import decoders as od
    tw = np.load(os.path.join(GOLDEN, 'testwav.npz'))
    if reference_gains(np.array([tw['mean_square']], np.float32), -20)[0] == tw['gain']:
        assert text == ref_text, (what, text, ref_text)
        assert abs(score - ref_score) < 1e-3, (what, score, ref_score)
    else:
        assert od.cer(ref_text, text) <= 0.1 and abs(score - ref_score) < 0.5, (what, text, ref_text)


def test_gru_facade_matches_reference(tmp_path, monkeypatch):
    z = np.load(os.path.join(GOLDEN, 'predictor_deepspeech2_gru.npz'))
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    p = _predictor(str(tmp_path), False)
    res = p.predict(audio_data=pcm.copy())
    _same(str(z['bi_text']), res['text'], float(z['bi_score']), res['score'], 'deepspeech2 gru (bi) predict(test.wav)')
    # ragged batch in passes of 2: two lanes == one lane
    audios = [pcm.copy(), pcm[:90000].copy(), pcm[30000:].copy(), pcm[:41000].copy(), pcm[10000:70000].copy()]
    got = {}
    for lanes in ('2', '1'):
        monkeypatch.setenv('MASR_LANES', lanes)
        got[lanes] = p.predict_batch(audios, batch_size=2)
    for a, b in zip(got['2'], got['1']):
        assert a['text'] == b['text'] and a['score'] == b['score']
    assert got['1'][0]['text'] == res['text']

    p = _predictor(str(tmp_path), True)
    res = p.predict(audio_data=pcm.copy())
    _same(str(z['uni_text']), res['text'], float(z['uni_score']), res['score'], 'deepspeech2 gru (uni) predict(test.wav)')
    p.reset_stream()
    for k, s in enumerate(range(0, len(pcm), 8000)):
        r = p.predict_stream(audio_data=pcm[s:s + 8000].tobytes(), is_end=(s + 8000 >= len(pcm)))
        valid = r is not None and r['text'] is not None
        assert valid == bool(z['stream_valid'][k]), f'call {k}: validity differs'
        if valid:
            _same(str(z['stream_text'][k]), r['text'], float(z['stream_score'][k]), r['score'], f'gru predict_stream call {k}')
    p.reset_stream()


def test_gru_stream_pool(tmp_path):
    """StreamPool over the streaming GRU model: two concurrent sessions == two sequential predict_stream runs"""
    from masr_amd.serving import StreamPool
    from oracle import decoders as od
    p = _predictor(str(tmp_path), True)
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    audios = [pcm[:64000], pcm[40000:96000]]
    want = []
    for a in audios:
        p.reset_stream()
        want.append([p.predict_stream(audio_data=a[s:s + 8000].tobytes(), is_end=(s + 8000 >= len(a)))
                     for s in range(0, len(a), 8000)])
    p.reset_stream()
    pool = StreamPool(p)
    hs = [pool.open() for _ in audios]
    got = [[] for _ in audios]
    for k in range(8):
        for i, a in enumerate(audios):
            if k * 8000 < len(a):
                pool.feed(hs[i], a[k * 8000:(k + 1) * 8000].tobytes(), is_end=((k + 1) * 8000 >= len(a)))
        out = pool.step()
        for i, h in enumerate(hs):
            if h in out:
                got[i].append(out[h])
    for i in range(2):
        assert len(got[i]) == len(want[i])
        assert any(g_ is not None for g_ in got[i])
        for g_, w_ in zip(got[i], want[i]):
            assert (g_ is None) == (w_ is None or w_['text'] is None)
            if g_ is not None:
                assert od.cer(w_['text'], g_['text']) <= 0.02 and abs(g_['score'] - w_['score']) < 0.05
    for h in hs:
        pool.close(h)
    pool.shutdown()
