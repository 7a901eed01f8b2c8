"""The conv2d6 and conv2d8 encoder front-ends (encoder_conf.input_layer; reference conformer/subsampling.py:115-211).

conv2d6: conv1 3x3 stride 2, then 5x5 stride 3 (gemm_f32.hip: the A_CONV5 gather, conv2_rows_kernel<RB_X1, 5, 3>), 12 bins into
``embed.linear``; conv2d8: conv1 and conv2 as conv2d, then a third 3x3 stride-2 conv over conv2's [B, T2, 19, d] output, 9 bins.
The restatement below feeds the layer functions of oracle/conformer.py; only the front-end and its mask are new.  The CPU tests
pin the length helpers against the reference's mask slicing and the config validation (which refused both layers before)."""
import math
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

LAYERS = ('conv2d6', 'conv2d8')
MIN_FRAMES = {'conv2d': 7, 'conv2d6': 11, 'conv2d8': 15}


# ---- torch-CPU restatement of the new front-ends ------------------------------------------------------------------------
def embed_il(sd, feats, il):
    """GlobalCMVN + Conv2dSubsampling6 / 8 forward (subsampling.py:152-155, 204-210) incl. x * sqrt(d) (embedding.py:97)."""
    x = ((feats - sd['encoder.global_cmvn.mean']) * sd['encoder.global_cmvn.istd']).unsqueeze(1)
    x = F.relu(F.conv2d(x, sd['encoder.embed.conv.0.weight'], sd['encoder.embed.conv.0.bias'], stride=2))
    x = F.relu(F.conv2d(x, sd['encoder.embed.conv.2.weight'], sd['encoder.embed.conv.2.bias'], stride=3 if il == 'conv2d6' else 2))
    if il == 'conv2d8':
        x = F.relu(F.conv2d(x, sd['encoder.embed.conv.4.weight'], sd['encoder.embed.conv.4.bias'], stride=2))
    b, c, t, f = x.shape
    x = F.linear(x.transpose(1, 2).reshape(b, t, c * f), sd['encoder.embed.linear.weight'], sd['encoder.embed.linear.bias'])
    return x * math.sqrt(x.shape[-1])


def mask_il(m, il):
    """the subsampled mask of subsampling.py:112 / 156 / 210 on the last axis"""
    m = m[..., :-2:2]
    if il == 'conv2d':
        return m[..., :-2:2]
    if il == 'conv2d6':
        return m[..., :-4:3]
    return m[..., :-2:2][..., :-2:2]


def encoder_full_il(sd, feats, lens, il, streaming, decoding_chunk_size=-1, heads=4, kernel=15):
    """oracle.conformer.encoder_full with the conv2d6 / conv2d8 front-end"""
    from oracle import conformer as oc
    if not streaming:
        decoding_chunk_size = -1
    B, T, _ = feats.shape
    x = embed_il(sd, feats, il)
    Tp = x.shape[1]
    pad_s = mask_il(torch.arange(T)[None, :] < lens[:, None], il)
    pos_emb = oc.positional_table(5000, x.shape[-1], x.dtype)[:Tp].unsqueeze(0)
    idx = torch.arange(Tp)
    if decoding_chunk_size < 0:
        chunk = torch.ones(Tp, Tp, dtype=torch.bool)
    else:
        chunk = idx[None, :] < ((idx[:, None] // decoding_chunk_size + 1) * decoding_chunk_size)
    att_mask = pad_s[:, None, :] & chunk[None]
    for i in range(oc.num_blocks_of(sd)):
        x, _, _ = oc._layer(sd, i, x, pos_emb, att_mask, pad_s, heads, kernel, causal=streaming)
    return oc._ln(sd, 'encoder.after_norm', x)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('il', ('conv2d',) + LAYERS)
def test_length_helpers_match_reference_masks(il):
    from masr_amd.engine import MIN_FRAMES as MF, subsampled_len
    assert MF[il] == MIN_FRAMES[il]
    for T in range(1, 401):
        n = mask_il(torch.ones(T, dtype=torch.bool), il).numel()
        if T < MIN_FRAMES[il]:
            assert subsampled_len(T, il) <= 0, T
            continue
        assert subsampled_len(T, il) == n, (il, T)
        # frame t of an utterance of `ln` frames is valid iff rate * t < ln (the kernels' sub_lens test)
        rate = {'conv2d': 4, 'conv2d6': 6, 'conv2d8': 8}[il]
        for ln in (1, T // 3 + 1, T - 1, T):
            m = mask_il(torch.arange(T) < ln, il)
            assert torch.equal(m, rate * torch.arange(n) < ln), (il, T, ln)
    # array form (HipEngine.enc_frames feeds frame-count arrays through it)
    T = np.arange(1, 401)
    assert np.array_equal(np.maximum(subsampled_len(T, il), 0),
                          [max(subsampled_len(int(t), il), 0) for t in T])


@pytest.mark.parametrize('il', ('conv2d',) + LAYERS)
def test_conv_geometry_matches_torch(il):
    """T' and the bins behind the last conv from torch's own conv arithmetic (one channel, zero weights)"""
    from masr_amd.engine import subsampled_len
    from masr_amd.utils import synthetic
    sd = synthetic.conformer_state_dict(0, 8, num_blocks=1, input_layer=il)
    lin = sd['encoder.embed.out.0.weight' if il == 'conv2d' else 'encoder.embed.linear.weight']
    F_last = {'conv2d': 19, 'conv2d6': 12, 'conv2d8': 9}[il]
    assert tuple(lin.shape) == (256, 256 * F_last)
    for T in (MIN_FRAMES[il], MIN_FRAMES[il] + 1, 67, 1001):
        x = torch.zeros(1, 1, T, 80)
        x = F.conv2d(x, torch.zeros(1, 1, 3, 3), stride=2)
        if il == 'conv2d6':
            x = F.conv2d(x, torch.zeros(1, 1, 5, 5), stride=3)
        else:
            x = F.conv2d(x, torch.zeros(1, 1, 3, 3), stride=2)
            if il == 'conv2d8':
                x = F.conv2d(x, torch.zeros(1, 1, 3, 3), stride=2)
        assert x.shape[2:] == (subsampled_len(T, il), F_last)


def test_validation_accepts_conv2d6_conv2d8_only():
    from masr_amd import _lib
    from masr_amd.engine import _validate_encoder_conf
    for model in ('conformer', 'efficient_conformer'):
        for il in ('conv2d',) + LAYERS:
            _validate_encoder_conf(model, {'input_layer': il}, None)
        for il in ('linear', 'conv2d2'):
            with pytest.raises(_lib.MasrError, match='input_layer'):
                _validate_encoder_conf(model, {'input_layer': il}, None)


def test_synthetic_default_unchanged():
    from masr_amd.utils import synthetic
    a = synthetic.conformer_state_dict(0, 16, num_blocks=1)
    b = synthetic.conformer_state_dict(0, 16, num_blocks=1, input_layer='conv2d')
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert 'encoder.embed.out.0.weight' in a and 'encoder.embed.linear.weight' not in a


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _engine(il, streaming=True, num_blocks=4, kind='conformer'):
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sd = getattr(synthetic, kind + '_state_dict')(0, 512, num_blocks=num_blocks, input_layer=il)
    enc = {'input_layer': il, 'num_blocks': num_blocks}
    return HipEngine(sd, encoder_conf=enc, vocab_size=512, streaming=streaming, use_model=kind), sd


def _feats(B, T, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, 80, generator=gen) * 3 + 13


def _valid(a, n):
    return torch.cat([a[i, :k] for i, k in enumerate(n)])


@pytest.mark.gpu
@pytest.mark.parametrize('streaming', (True, False))
@pytest.mark.parametrize('il', LAYERS)
def test_encode_full_against_restatement(il, streaming):
    from masr_amd.engine import subsampled_len
    from oracle import conformer as oc
    eng, sd = _engine(il, streaming)
    try:
        T = 211
        lens = torch.tensor([T, 150, MIN_FRAMES[il]], dtype=torch.int32)
        feats = _feats(3, T, 7)
        for i, n in enumerate(lens.tolist()):
            feats[i, n:] = 0
        for chunk in ((-1, 4) if streaming else (-1,)):
            with torch.no_grad():
                ref = encoder_full_il(sd, feats, lens, il, streaming, chunk)
                ref_p = oc.ctc_probs(sd, ref)
            enc = eng.encode_full(feats.cuda(), lens.cuda(), chunk)
            probs = eng.ctc_probs(enc)
            assert enc.shape == ref.shape == (3, subsampled_len(T, il), 256)
            n = [int(x) for x in (lens - 1) // {'conv2d6': 6, 'conv2d8': 8}[il] + 1]      # valid frames: rate * t < len
            e, r = _valid(enc.cpu(), n), _valid(ref, n)
            assert (e - r).abs().max() < 1e-3, (e - r).abs().max()
            p, rp = _valid(probs.cpu(), n), _valid(ref_p, n)
            assert (p - rp).abs().max() < 1e-3
            assert torch.equal(p.argmax(-1), rp.argmax(-1))
            # frame counts of the engine's own helpers
            # (a padded batch keeps the mask's count, ceil(len / rate), which may exceed the utterance's own T')
            m = MIN_FRAMES[il]
            assert eng.enc_frames(np.array([T, 150, m, m - 1])).tolist() == [subsampled_len(t, il) for t in (T, 150, m)] + [0]
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('il', LAYERS)
def test_chunks_over_facade_windows_against_restatement(il):
    """67-frame windows every 64 frames (predict.py:283-306: 10 / 7 encoder frames per window), the last one short.  (The
    Efficient Conformer's half-rate layers need an even number of frames per chunk -- its reference chunk forward fails on the
    7 frames of a conv2d8 window -- so it is not covered here.)"""
    from masr_amd.engine import subsampled_len
    from oracle import conformer as oc
    mod = oc
    eng, sd = _engine(il, True)
    try:
        feats = _feats(1, 67 + 64 * 3 + 20, 11)
        sid = eng.stream_open(200)
        att = torch.zeros(0, 0, 0, 0)
        cnn = torch.zeros(0, 0, 0, 0)
        off = 0
        n_win = 0
        with mock.patch.object(oc, 'embed', lambda sd_, x: embed_il(sd_, x, il)):
            for cur in range(0, feats.shape[1] - 7 + 1, 64):
                ch = feats[:, cur:cur + 67]
                if subsampled_len(ch.shape[1], il) <= 0:
                    continue
                with torch.no_grad():
                    ref, att, cnn = mod.get_encoder_out_chunk(sd, ch, off, -16, att, cnn)
                off += ref.shape[1]
                p, _, _ = eng.encode_chunk([sid], ch.cuda().contiguous())
                assert p.shape == ref.shape, (p.shape, ref.shape)
                assert (p.cpu() - ref).abs().max() < 1e-3
                n_win += 1
        assert n_win >= 4
        eng.stream_close(sid)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('il', LAYERS)
def test_batch_32x10s_against_restatement(il):
    """B = 32 x 10 s (998 frames): M = 5 280 / 3 936 encoder rows; the row-block front-end (conv1 fused into conv2's gather
    under conv2d8, masr_debug_set key 41 -- bit-identical on and off) against the restatement"""
    from masr_amd._lib import debug_keys
    eng, sd = _engine(il, False, num_blocks=1)
    try:
        B, T = 32, 998
        feats = _feats(B, T, 3)
        lens = torch.full((B,), T, dtype=torch.int32)
        enc = eng.encode_full(feats.cuda(), lens.cuda(), -1).clone()
        assert enc.shape[0] * enc.shape[1] == {'conv2d6': 5280, 'conv2d8': 3936}[il]
        with debug_keys(eng, conv1_fused=0):
            enc0 = eng.encode_full(feats.cuda(), lens.cuda(), -1).clone()
        assert torch.equal(enc, enc0)
        with torch.no_grad():
            ref = encoder_full_il(sd, feats, lens.long(), il, False)
        assert (enc.cpu() - ref).abs().max() < 1e-3, (enc.cpu() - ref).abs().max()
    finally:
        eng.close()


@pytest.mark.gpu
def test_checkpoint_of_another_front_end_is_refused():
    from masr_amd import _lib
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sd = synthetic.conformer_state_dict(0, 64, num_blocks=1, input_layer='conv2d8')
    for il in ('conv2d', 'conv2d6'):
        with pytest.raises(_lib.MasrError):
            HipEngine(sd, encoder_conf={'input_layer': il, 'num_blocks': 1}, vocab_size=64)


# ---- fixtures recorded from the reference modules (tools/make_input_layer_golden.py) -----------------------------------------
GOLDEN = __import__('os').path.join(__import__('os').path.dirname(__file__), 'golden')


def _golden(name):
    return np.load(__import__('os').path.join(GOLDEN, name))


def _generator():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'make_input_layer_golden.py')
    spec = importlib.util.spec_from_file_location('make_input_layer_golden', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference_present():
    from oracle import shims
    return shims.reference_available()


@pytest.mark.skipif(not _reference_present(), reason='the reference checkout is not on this machine')
def test_fixtures_match_live_reference(tmp_path):
    gen = _generator()
    recs = {f'conformer_{il}_v512.npz': lambda il=il: gen.conformer_record(il, True, str(tmp_path)) for il in LAYERS}
    recs.update({f'conformer_{il}_nonstreaming_v512.npz': lambda il=il: gen.conformer_record(il, False, str(tmp_path))
                 for il in LAYERS})
    recs['efficient_conformer_conv2d8_v512.npz'] = lambda: gen.efficient_record('conv2d8', str(tmp_path))
    recs['predictor_conv2d8.npz'] = lambda: gen.facade_record(str(tmp_path))
    for name, make in recs.items():
        z, live = _golden(name), make()
        assert sorted(z.files) == sorted(live), name
        for k in z.files:
            a, b = z[k], np.asarray(live[k])
            if a.dtype.kind == 'f':
                assert np.allclose(a, b, rtol=0, atol=1e-5), (name, k, np.abs(a - b).max())
            else:
                assert np.array_equal(a, b), (name, k)


def _engine12(kind, il, streaming=True, vocab=512):
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sd = getattr(synthetic, kind + '_state_dict')(0, vocab, input_layer=il)
    return HipEngine(sd, encoder_conf={'input_layer': il}, vocab_size=vocab, streaming=streaming, use_model=kind)


@pytest.mark.gpu
@pytest.mark.parametrize('streaming', (True, False))
@pytest.mark.parametrize('il', LAYERS)
def test_conformer_against_reference_fixture(il, streaming):
    z = _golden(f'conformer_{il}_v512.npz' if streaming else f'conformer_{il}_nonstreaming_v512.npz')
    eng = _engine12('conformer', il, streaming)
    try:
        feats, lens = torch.from_numpy(z['feats']).cuda(), torch.from_numpy(z['lens']).cuda()
        rate = {'conv2d6': 6, 'conv2d8': 8}[il]
        n = [int(x) for x in (z['lens'] - 1) // rate + 1]
        for chunk, key in ((-1, 'enc'), (4, 'enc4')) if streaming else ((-1, 'enc'),):
            enc = eng.encode_full(feats, lens, chunk)
            assert enc.shape == z[key].shape
            e, r = _valid(enc.cpu(), n), _valid(torch.from_numpy(z[key]), n)
            assert (e - r).abs().max() < 1e-3, (key, (e - r).abs().max())
            if key == 'enc':
                p, rp = _valid(eng.ctc_probs(enc).cpu(), n), _valid(torch.from_numpy(z['probs']), n)
                assert (p - rp).abs().max() < 1e-3
                assert torch.equal(p.argmax(-1), rp.argmax(-1))          # greedy transcripts
        if streaming:           # get_encoder_out_chunk over the facade's windows
            sid = eng.stream_open(400)
            out = []
            for a, b in z['chunk_spans']:
                p, _, _ = eng.encode_chunk([sid], feats[:1, a:b].contiguous())
                out.append(p[0].cpu())
            eng.stream_close(sid)
            got = torch.cat(out)
            assert got.shape == z['chunk_probs'].shape
            assert (got - torch.from_numpy(z['chunk_probs'])).abs().max() < 1e-3
    finally:
        eng.close()


@pytest.mark.gpu
def test_efficient_conformer_conv2d8_against_reference_fixture():
    from masr_amd import _lib
    z = _golden('efficient_conformer_conv2d8_v512.npz')
    eng = _engine12('efficient_conformer', 'conv2d8')
    try:
        feats, lens = torch.from_numpy(z['feats']).cuda(), torch.from_numpy(z['lens']).cuda()
        enc = eng.encode_full(feats, lens, -1)
        probs = eng.ctc_probs(enc)
        assert enc.shape == z['enc'].shape
        n = [int(x) for x in ((z['lens'] - 1) // 8 + 1 + 1) // 2]        # valid frames behind the stride layer: ceil(ceil(len / 8) / 2)
        e, r = _valid(enc.cpu(), n), _valid(torch.from_numpy(z['enc']), n)
        assert (e - r).abs().max() < 1e-3, (e - r).abs().max()
        p, rp = _valid(probs.cpu(), n), _valid(torch.from_numpy(z['probs']), n)
        assert (p - rp).abs().max() < 1e-3
        assert torch.equal(p.argmax(-1), rp.argmax(-1))
        # chunked: 7 frames per 67-frame window; the reference's chunk forward fails on the second window -- refused here
        sid = eng.stream_open(200)
        eng.encode_chunk([sid], feats[:1, 0:67].contiguous())
        with pytest.raises(_lib.MasrError, match='odd number of encoder frames'):
            eng.encode_chunk([sid], feats[:1, 64:131].contiguous())
        eng.stream_close(sid)
    finally:
        eng.close()


FACADE = """
encoder_conf: {output_size: 256, attention_heads: 4, linear_units: 2048, num_blocks: 12, input_layer: conv2d8,
  normalize_before: True, cnn_module_kernel: 15, use_cnn_module: True, activation_type: swish, pos_enc_layer_type: rel_pos}
preprocess_conf: {feature_method: fbank, n_mels: 80, n_mfcc: 40, sample_rate: 16000, use_dB_normalization: False, target_dB: -20}
dataset_conf: {dataset_vocab: VOCAB}
use_model: conformer
streaming: True
decoder: ctc_greedy
metrics_type: cer
"""


@pytest.fixture(scope='module')
def facade8(tmp_path_factory):
    import os
    import yaml
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    d = tmp_path_factory.mktemp('facade8')
    vpath = os.path.join(d, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(4233):
            f.write(f'{t}\t1\n')
    cfg = yaml.safe_load(FACADE.replace('VOCAB', vpath))
    return MASRPredictor(configs=cfg, use_gpu=True, state_dict=synthetic.conformer_state_dict(0, 4233, input_layer='conv2d8'))


@pytest.mark.gpu
def test_facade_conv2d8_against_reference_facade(facade8):
    """predict / predict_stream of a conv2d8 Conformer against the reference facade (no dB normalisation: exact on any host)"""
    z = _golden('predictor_conv2d8.npz')
    pcm = np.load(__import__('os').path.join(GOLDEN, 'testwav.npz'))['pcm']
    res = facade8.predict(audio_data=pcm.copy())
    assert res['text'] == str(z['offline_text']) and abs(res['score'] - float(z['offline_score'])) < 1e-3
    facade8.reset_stream()
    step = 8000
    for k, s in enumerate(range(0, len(pcm), step)):
        r = facade8.predict_stream(audio_data=pcm[s:s + step].tobytes(), is_end=(s + step >= len(pcm)))
        valid = r is not None and r['text'] is not None
        assert valid == bool(z['stream_valid'][k]), k
        if valid:
            assert r['text'] == str(z['stream_text'][k]), (k, r['text'], str(z['stream_text'][k]))
            assert abs(r['score'] - float(z['stream_score'][k])) < 1e-3
    facade8.reset_stream()
    # predict_batch: the minimum-length check (15 frames under conv2d8) sets a 14-frame utterance aside
    short = pcm[:400 + 13 * 160].copy()
    out = facade8.predict_batch([short, pcm[:400 + 14 * 160].copy(), pcm.copy()])
    assert out[0] == {'text': '', 'score': 0}
    assert out[2]['text'] == str(z['offline_text'])


@pytest.mark.gpu
def test_stream_pool_short_last_window_and_exact_room(facade8):
    """a session whose last window is below conv2d8's minimum (8-14 frames) keeps the transcript of the windows before it, and
    a stream sized to exactly the frames its windows give is not refused (the pool counts frames per front-end)"""
    from masr_amd.engine import subsampled_len
    from masr_amd.serving import StreamPool
    pcm = np.load(__import__('os').path.join(GOLDEN, 'testwav.npz'))['pcm']
    nfr = lambda n: 1 + (n - 400) // 160
    spans = lambda T: [(c, min(c + 67, T)) for c in range(0, T - 7 + 1, 64)]
    # an utterance whose last window has 10 frames: 64 k + 10 frames in all
    T = 64 * 3 + 10
    n = 400 + (T - 1) * 160
    assert nfr(n) == T and spans(T)[-1][1] - spans(T)[-1][0] == 10 and subsampled_len(10, 'conv2d8') <= 0
    T0 = T - 10 + 3                               # the same audio without the short tail's new frames (window ends unchanged)
    need = sum(max(subsampled_len(b - a, 'conv2d8'), 0) for a, b in spans(T))
    results = []
    for frames_out in (need, 0):
        pool = StreamPool(facade8, max_frames_out=frames_out)
        try:
            h = pool.open()
            pool.feed(h, pcm[:n].copy(), is_end=True)
            out = pool.step()
            assert h not in pool.errors, pool.errors
            results.append(out[h])
        finally:
            pool.shutdown()
    assert results[0] == results[1] and results[0]['text']
    facade8.reset_stream()
    ref = facade8.predict_stream(audio_data=pcm[:400 + (T0 - 1) * 160].tobytes(), is_end=True)
    facade8.reset_stream()
    assert ref['text'] == results[0]['text']
