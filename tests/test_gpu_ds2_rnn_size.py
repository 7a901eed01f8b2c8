"""GPU: DeepSpeech2 with ``encoder_conf.rnn_size`` off 1024 (every multiple of 256 from 256 to 2048; lstm.hip / gru.hip are
instantiated per size) against torch.nn.LSTM / torch.nn.GRU on the CPU with the same weights, against fixtures recorded from the
REAL reference (tools/make_ds2_rnn_size_golden.py), and through the facade.

Bars as in test_gpu_ds2_gru.py: probabilities to 1e-3, argmax agreement > 0.995 on valid frames, facade transcripts equal to
the reference facade's.  256 is the one-vector-per-lane edge of the wave-per-unit kernels, 768 is no power of two, 2048 is the
register maximum (one layer there: 0.35 GB of weights for the bi-directional model)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
V = 50


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def layers_of(H):
    return 1 if H == 2048 else 2


@pytest.fixture(scope='module')
def engines():
    """engine(H, gru, streaming) -> (HipEngine, state dict); one engine per (H, cell, direction) for the whole module"""
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    cache = {}

    def get(H, gru, streaming):
        key = (H, gru, streaming)
        if key not in cache:
            L = layers_of(H)
            sd = synthetic.deepspeech2_state_dict(0, V, rnn_size=H, num_rnn_layers=L, bidirectional=not streaming, use_gru=gru)
            conf = {'num_rnn_layers': L, 'rnn_size': H, 'use_gru': gru}
            cache[key] = (HipEngine(sd, encoder_conf=conf, streaming=streaming, use_model='deepspeech2'), sd)
        return cache[key]

    yield get
    for e, _ in cache.values():
        e.close()


@torch.no_grad()
def cpu_probs(sd, feats, lens):
    """oracle conv front-end, then per layer torch.nn.LSTM / torch.nn.GRU over the packed sequence and LayerNorm, then the CTC
    softmax"""
    from oracle import deepspeech2 as ods
    x, xl = ods.conv_frontend(sd, feats, lens)
    gru = 'encoder.rnns.0.rnn.rnn.weight_ih_l0' in sd
    deep = 'rnn.rnn.' if gru else 'rnn.'
    bi = f'encoder.rnns.0.{deep}weight_ih_l0_reverse' in sd
    H = sd[f'encoder.rnns.0.{deep}weight_hh_l0'].shape[1]
    i = 0
    while f'encoder.rnns.{i}.layer_norm.weight' in sd:
        p = f'encoder.rnns.{i}.{deep}'
        rnn = (torch.nn.GRU if gru else torch.nn.LSTM)(x.shape[-1], H, num_layers=1, batch_first=True, bidirectional=bi)
        rnn.load_state_dict({k[len(p):]: v for k, v in sd.items() if k.startswith(p)})
        packed = torch.nn.utils.rnn.pack_padded_sequence(x, xl, batch_first=True, enforce_sorted=False)
        y, _ = rnn(packed)
        x, _ = torch.nn.utils.rnn.pad_packed_sequence(y, batch_first=True)
        x = F.layer_norm(x, (x.shape[-1],), sd[f'encoder.rnns.{i}.layer_norm.weight'], sd[f'encoder.rnns.{i}.layer_norm.bias'], 1e-5)
        i += 1
    return torch.softmax(F.linear(x, sd['decoder.ctc_lo.weight'], sd['decoder.ctc_lo.bias']), dim=2), xl


def ragged(B, T=131):
    """lengths drawn as in test_gpu_ds2_gru.py, one sequence at full length; T = 131 feature frames = 31 steps"""
    torch.manual_seed(100 + B)
    lens = torch.randint(40, T + 1, (B,))
    lens[B // 2] = T
    x = (torch.randn(B, T, 80) * 3 + 13) * (torch.arange(T)[None, :, None] < lens[:, None, None])
    return x, lens


# B = 1, 3: wave-per-unit form; 8: matrix-core form, one sequence tile; 20: two tiles; 40: wave form past 32
@pytest.mark.parametrize('B', [1, 3, 8, 20, 40])
@pytest.mark.parametrize('gru', [False, True], ids=['lstm', 'gru'])
@pytest.mark.parametrize('H', [256, 768, 2048])
def test_step_forms_ragged_against_torch(engines, H, gru, B):
    x, lens = ragged(B)
    for streaming in (False, True):
        e, sd = engines(H, gru, streaming)
        probs = e.ctc_probs(e.encode_full(dev(x), dev(lens, torch.int32))).cpu()
        ref, xl = cpu_probs(sd, x, lens)
        n = ref.shape[1]                                       # pad_packed_sequence trims to the longest sequence
        assert probs.shape[0] == B and probs.shape[1] >= n
        err = (probs[:, :n] - ref).abs().max().item()
        print(f'H {H} gru {gru} B {B} streaming {streaming}: max prob err {err:.2e}')
        assert err < 1e-3, (H, gru, B, streaming, err)
        for b in range(B):
            k = int(xl[b])
            assert (probs[b, :k].argmax(-1) == ref[b, :k].argmax(-1)).float().mean().item() > 0.995


# rnn_size <= 512 runs the matrix-core form on 4 units per workgroup; key 43 = -8 runs the 8 of the larger sizes.  A column's dot
# product is formed by the same waves over the same k order either way, so the two must agree bit for bit.
@pytest.mark.parametrize('B', [8, 20])
@pytest.mark.parametrize('gru', [False, True], ids=['lstm', 'gru'])
def test_units_per_workgroup_give_the_same_bits(engines, gru, B):
    from masr_amd._lib import debug_keys
    x, lens = ragged(B)
    for streaming in (False, True):
        e, sd = engines(512, gru, streaming)
        with debug_keys(e, rnn_mfma_units=-8):
            eight = e.encode_full(dev(x), dev(lens, torch.int32)).clone()
        four = e.encode_full(dev(x), dev(lens, torch.int32))
        assert torch.equal(four, eight)
        ref, _ = cpu_probs(sd, x, lens)
        assert (e.ctc_probs(four).cpu()[:, :ref.shape[1]] - ref).abs().max().item() < 1e-3


@pytest.mark.parametrize('H,gru', [(768, False), (2048, True)], ids=['h768-lstm', 'h2048-gru'])
def test_against_reference_fixture(H, gru):
    """the fixture's models have 2 layers at both sizes, so these engines are the test's own"""
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    from oracle.make_golden import golden_inputs
    z = np.load(os.path.join(GOLDEN, 'deepspeech2_rnn_sizes.npz'))
    k = f'h{H}_{"gru" if gru else "lstm"}_'
    feats, lens = golden_inputs()
    conf = {'num_rnn_layers': 2, 'rnn_size': H, 'use_gru': gru}
    for streaming, key in ((False, 'bi_probs'), (True, 'uni_probs')):
        sd = synthetic.deepspeech2_state_dict(0, V, rnn_size=H, num_rnn_layers=2, bidirectional=not streaming, use_gru=gru)
        e = HipEngine(sd, encoder_conf=conf, streaming=streaming, use_model='deepspeech2')
        try:
            enc = e.encode_full(dev(feats), dev(lens, torch.int32))
            probs = e.ctc_probs(enc).cpu().numpy()
            ref = z[k + key]                               # [3, 82, 50]; padded rows of the shorter utterances included
            assert probs.shape == ref.shape
            err = np.abs(probs - ref).max()
            print(f'{k}{key}: max prob err {err:.2e}')
            assert err < 1e-3, (key, err)
            valid = [82, 49, 23]
            for b in range(3):
                assert (probs[b, :valid[b]].argmax(-1) == ref[b, :valid[b]].argmax(-1)).mean() > 0.995
            idx, mp = e.ctc_greedy_frames(enc)
            assert np.array_equal(idx.cpu().numpy(), probs.argmax(-1))
            np.testing.assert_allclose(mp.cpu().numpy(), probs.max(-1), atol=1e-6)
            if not streaming:
                continue
            # streaming: the 5 chunks and the final state of the fixture, the exported cache, reset
            sid = e.stream_open(0)
            for i, cur in enumerate(range(0, 331 - 67 + 1, 64)):
                p, _, _ = e.encode_chunk([sid], dev(feats[:1, cur:cur + 67]))
                assert np.abs(p[0].cpu().numpy() - z[k + 'chunk_probs'][i]).max() < 1e-3
            h, c = e.stream_export_cache(sid)
            assert tuple(h.shape) == (2, 1, 1, H) and tuple(c.shape) == (2, 1, 1, H)
            assert np.abs(h.cpu().numpy() - z[k + 'h']).max() < 1e-3
            assert np.abs(c.cpu().numpy() - z[k + 'c']).max() < 1e-3
            if gru:
                assert torch.equal(h, c)                   # gru.py: final_state_c = final_state_h
            e.stream_reset(sid)
            p0, _, _ = e.encode_chunk([sid], dev(feats[:1, :67]))
            assert np.abs(p0[0].cpu().numpy() - z[k + 'chunk_probs'][0]).max() < 1e-3
            e.stream_close(sid)
        finally:
            e.close()


@pytest.mark.parametrize('H,gru', [(256, True), (768, False), (2048, True)], ids=['h256-gru', 'h768-lstm', 'h2048-gru'])
def test_interleaved_streams_equal_each_alone(engines, H, gru):
    e, _ = engines(H, gru, True)
    torch.manual_seed(11)
    xa = torch.randn(1, 195, 80) * 3 + 13
    xb = torch.randn(1, 195, 80) * 3 + 13
    alone = []
    for xx in (xa, xb):
        s = e.stream_open(0)
        alone.append([e.encode_chunk([s], dev(xx[:, cur:cur + 67]))[0][0].cpu() for cur in (0, 64, 128)])
        h, c = e.stream_export_cache(s)
        assert tuple(h.shape) == (layers_of(H), 1, 1, H) and tuple(c.shape) == tuple(h.shape)
        assert torch.equal(h, c) == gru
        e.stream_close(s)
    s0, s1 = e.stream_open(0), e.stream_open(0)
    for k, cur in enumerate((0, 64, 128)):
        probs, _, _ = e.encode_chunk([s0, s1], dev(torch.cat([xa[:, cur:cur + 67], xb[:, cur:cur + 67]])))
        assert (probs[0].cpu() - alone[0][k]).abs().max().item() < 1e-5
        assert (probs[1].cpu() - alone[1][k]).abs().max().item() < 1e-5
    e.stream_close(s0)
    e.stream_close(s1)


@pytest.mark.parametrize('gru', [False, True], ids=['lstm', 'gru'])
def test_explicit_1024_equals_default(gru):
    """an explicit ``rnn_size: 1024`` builds the engine that the absent key builds: the two agree bit for bit.  (Both run this
    tree's kernels, so this says nothing about an earlier tree; that 1024 still computes what it did is what the 1e-3 tests of
    test_gpu_parity.py and test_gpu_ds2_gru.py hold.)"""
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sd = synthetic.deepspeech2_state_dict(0, V, num_rnn_layers=1, bidirectional=True, use_gru=gru)
    e0 = HipEngine(sd, encoder_conf={'num_rnn_layers': 1, 'use_gru': gru}, streaming=False, use_model='deepspeech2')
    e1 = HipEngine(sd, encoder_conf={'num_rnn_layers': 1, 'use_gru': gru, 'rnn_size': 1024}, streaming=False, use_model='deepspeech2')
    try:
        assert e0.d_model == e1.d_model == 1024
        for B in (2, 8, 20):
            x, lens = ragged(B)
            a = e0.encode_full(dev(x), dev(lens, torch.int32))
            b = e1.encode_full(dev(x), dev(lens, torch.int32))
            assert torch.equal(a, b)
            ref, _ = cpu_probs(sd, x, lens)
            assert (e1.ctc_probs(b).cpu()[:, :ref.shape[1]] - ref).abs().max().item() < 1e-3
    finally:
        e0.close()
        e1.close()


def test_refusals_at_the_c_level(monkeypatch):
    from masr_amd import _lib, engine as eng_mod
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sd = synthetic.deepspeech2_state_dict(0, V, rnn_size=256, num_rnn_layers=1, bidirectional=False)
    # the Python check in front of the engine
    with pytest.raises(_lib.MasrError, match='rnn_size'):
        HipEngine(sd, encoder_conf={'num_rnn_layers': 1, 'rnn_size': 1000}, streaming=True, use_model='deepspeech2')
    with pytest.raises(_lib.MasrError, match='rnn_size'):
        HipEngine(sd, encoder_conf={'num_rnn_layers': 1, 'rnn_size': 512}, streaming=True, use_model='deepspeech2')
    # and the engine itself
    monkeypatch.setattr(eng_mod, '_validate_rnn_size', lambda *a: None)
    for size in (1000, 128, 2304):
        with pytest.raises(_lib.MasrError, match='rnn_size'):
            HipEngine(sd, encoder_conf={'num_rnn_layers': 1, 'rnn_size': size}, streaming=True, use_model='deepspeech2')
    with pytest.raises(_lib.MasrError, match='expected'):          # masr_finalize: the tensors have the checkpoint's shapes
        HipEngine(sd, encoder_conf={'num_rnn_layers': 1, 'rnn_size': 512}, streaming=True, use_model='deepspeech2')
    e = HipEngine(sd, encoder_conf={'num_rnn_layers': 1, 'rnn_size': 256}, streaming=True, use_model='deepspeech2')
    e.close()


# ---------------------------------------------------------------------------------------------------
# the facade: MASRPredictor / StreamPool at rnn_size 512 (fixture: predictor_deepspeech2_h512.npz)
# ---------------------------------------------------------------------------------------------------
DS2_H512_CONFIG = """
encoder_conf: {num_rnn_layers: 5, rnn_size: 512, use_gru: False}
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
    cfg = yaml.safe_load(DS2_H512_CONFIG.replace('VOCAB', vpath).replace('STREAMING', str(streaming)))
    sd = synthetic.deepspeech2_state_dict(0, 4233, rnn_size=512, bidirectional=not streaming)
    mpath = os.path.join(d, f'model_h512_{streaming}.pt')
    torch.save(sd, mpath)
    return MASRPredictor(configs=cfg, model_path=mpath, use_gpu=True)


def _same(ref_text, text, ref_score, score, what):
    """exact transcripts where this host's numpy reproduces the fixture's normalisation gain (as test_gpu_ds2_gru.py::_same)"""
    from masr_amd.engine import reference_gains
    from oracle import decoders as od
    tw = np.load(os.path.join(GOLDEN, 'testwav.npz'))
    if reference_gains(np.array([tw['mean_square']], np.float32), -20)[0] == tw['gain']:
        assert text == ref_text, (what, text, ref_text)
        assert abs(score - ref_score) < 1e-3, (what, score, ref_score)
    else:
        assert od.cer(ref_text, text) <= 0.1 and abs(score - ref_score) < 0.5, (what, text, ref_text)


def test_h512_facade_matches_reference(tmp_path, monkeypatch):
    z = np.load(os.path.join(GOLDEN, 'predictor_deepspeech2_h512.npz'))
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    p = _predictor(str(tmp_path), False)
    res = p.predict(audio_data=pcm.copy())
    _same(str(z['bi_text']), res['text'], float(z['bi_score']), res['score'], 'deepspeech2 rnn_size 512 (bi) predict(test.wav)')
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
    _same(str(z['uni_text']), res['text'], float(z['uni_score']), res['score'], 'deepspeech2 rnn_size 512 (uni) predict(test.wav)')
    p.reset_stream()
    for k, s in enumerate(range(0, len(pcm), 8000)):
        r = p.predict_stream(audio_data=pcm[s:s + 8000].tobytes(), is_end=(s + 8000 >= len(pcm)))
        valid = r is not None and r['text'] is not None
        assert valid == bool(z['stream_valid'][k]), f'call {k}: validity differs'
        if valid:
            _same(str(z['stream_text'][k]), r['text'], float(z['stream_score'][k]), r['score'], f'h512 predict_stream call {k}')
    p.reset_stream()


def test_h512_stream_pool(tmp_path):
    """StreamPool over the streaming rnn_size 512 model: two concurrent sessions == two sequential predict_stream runs"""
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
