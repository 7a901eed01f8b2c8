"""cnn_module_norm: batch_norm on the GPU: the Efficient Conformer's full-context forward and chunk steps against the reference
fixture tests/golden/efficient_bn_v50.npz (tools/make_efficient_bn_golden.py), and the fused conv-module head stage of the
BatchNorm builds against the separate launches.  The parity bound is the one of every fixture test of test_gpu_parity.py:
max abs < 1e-3."""
import os

import numpy as np
import pytest
import torch

from masr_amd._lib import MasrError, debug_keys

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
V = 50
EFF_CONF = {'output_size': 256, 'attention_heads': 4, 'linear_units': 2048, 'num_blocks': 5, 'cnn_module_kernel': 15,
            'cnn_module_norm': 'batch_norm',
            'efficient_conf': {'stride_layer_idx': [3], 'stride': [2], 'group_layer_idx': [0, 1, 2, 3], 'group_size': 3,
                               'stride_kernel': True}}
CHUNKS = [(c, 67) for c in range(0, 331 - 67 + 1, 64)]


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


@pytest.fixture(scope='module')
def z():
    return np.load(os.path.join(GOLDEN, 'efficient_bn_v50.npz'))


@pytest.fixture(scope='module')
def batch32(z):
    """the 32 x <= 998-frame batch of the fixture tool, regenerated (the file holds its lengths and a probe of the features)"""
    rng = np.random.default_rng(3)
    lens = rng.integers(300, 999, 32)
    lens[0] = 998
    feats = rng.standard_normal((32, 998, 80)).astype(np.float32) * 3 + 13
    feats *= (np.arange(998)[None, :, None] < lens[:, None, None])
    assert np.array_equal(lens, z['b32_lens']) and np.array_equal(feats[0, 0, :8], z['b32_probe']), 'generator drift'
    return dev(feats), dev(lens, torch.int32), lens


def _engine(family, streaming, norm):
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    if family == 'efficient_conformer':
        sd = synthetic.efficient_conformer_state_dict(0, V, num_blocks=5, cnn_module_norm=norm)
        conf = dict(EFF_CONF, cnn_module_norm=norm)
    else:
        sd = synthetic.conformer_state_dict(0, V, num_blocks=2, cnn_module_norm=norm)
        conf = {'num_blocks': 2, 'cnn_module_norm': norm}
    return HipEngine(sd, conf, vocab_size=V, streaming=streaming, use_model=family)


@pytest.fixture(scope='module')
def eff():
    """the Efficient Conformer BatchNorm engines: streaming: True / False"""
    es = {True: _engine('efficient_conformer', True, 'batch_norm'), False: _engine('efficient_conformer', False, 'batch_norm')}
    yield es
    for e in es.values():
        e.close()


def _probs(e, feats, lens):
    enc = e.encode_full(feats, lens, -1)
    return enc.cpu().numpy(), e.ctc_probs(enc).cpu().numpy()


@pytest.mark.parametrize('streaming', [True, False])
def test_full_forward_ragged_batch(eff, z, streaming):
    from oracle.make_golden import golden_inputs
    e, k = eff[streaming], 's_' if streaming else 'n_'
    feats, lens = golden_inputs()
    enc, probs = _probs(e, dev(feats), dev(lens, torch.int32))
    assert enc.shape == z[k + 'b3_enc'].shape and probs.shape == z[k + 'b3_probs'].shape
    err_e, err_p = np.abs(enc - z[k + 'b3_enc']).max(), np.abs(probs - z[k + 'b3_probs']).max()
    print(f'B = 3, streaming {streaming}: encoder max err {err_e:.3e}, probs max err {err_p:.3e}')
    assert err_e < 1e-3 and err_p < 1e-3


@pytest.mark.parametrize('streaming', [True, False])
@pytest.mark.parametrize('T', [203, 204, 205, 331])
def test_full_forward_single_utterances(eff, z, streaming, T):
    """T' mod 3 = 0 / 1 / 2 (grouping pad) and odd / even T' at the stride layer; one utterance = the few-rows launches"""
    e, k = eff[streaming], 's_' if streaming else 'n_'
    _, probs = _probs(e, dev(z[f'single_feats_{T}']), dev(np.array([T]), torch.int32))
    ref = z[k + f'single_probs_{T}']
    assert probs.shape == ref.shape
    err = np.abs(probs - ref).max()
    print(f'T = {T}, streaming {streaming}: probs max err {err:.3e}')
    assert err < 1e-3


def _rows012(e, batch32, ref):
    """max err of the valid frames of utterances 0-2 of the 32-utterance pass against the reference's three-utterance batch"""
    feats, lens_dev, lens = batch32
    _, probs = _probs(e, feats, lens_dev)
    nv = np.asarray(e.enc_frames(lens))
    assert probs.shape[1:] == ref.shape[1:]
    return max(np.abs(probs[b, :nv[b]] - ref[b, :nv[b]]).max() for b in range(3)), probs


@pytest.mark.parametrize('streaming', [True, False])
def test_full_forward_32_utterances(eff, z, batch32, streaming):
    """249 full-rate row blocks: the fused conv-module head on the 16-row FFN kernel; 125 half-rate ones behind the stride layer"""
    err, _ = _rows012(eff[streaming], batch32, z[('s_' if streaming else 'n_') + 'b32_probs'])
    print(f'32 utterances, streaming {streaming}: probs max err {err:.3e}')
    assert err < 1e-3


def test_chunk_steps_and_cnn_cache(eff, z):
    from oracle.make_golden import golden_inputs
    e = eff[True]
    feats, _ = golden_inputs()
    sid = e.stream_open(0)
    for i, (cur, n) in enumerate(CHUNKS):
        p, _, _ = e.encode_chunk([sid], dev(feats[:1, cur:cur + n]))
        assert p[0].shape == z['s_chunk_probs'][i].shape
        assert np.abs(p[0].cpu().numpy() - z['s_chunk_probs'][i]).max() < 1e-3
    _, cnn = e.stream_export_cache(sid)
    assert tuple(cnn.shape) == z['s_chunk_cnn'].shape == (5, 1, 256, 14)
    assert np.abs(cnn.cpu().numpy() - z['s_chunk_cnn']).max() < 1e-3
    e.stream_close(sid)


def test_two_sessions_out_of_phase(eff, z):
    """two sessions of one engine in lock-step calls, the second a chunk behind the first: each repeats the fixture's run"""
    from oracle.make_golden import golden_inputs
    e = eff[True]
    feats, _ = golden_inputs()
    s0, s1 = e.stream_open(0), e.stream_open(0)
    win = [dev(feats[:1, cur:cur + n]) for cur, n in CHUNKS]
    for step in range(len(CHUNKS) + 1):
        ids, xs, which = [], [], []
        if step < len(CHUNKS):
            ids, xs, which = [s0], [win[step]], [step]
        if step >= 1:
            ids, xs, which = ids + [s1], xs + [win[step - 1]], which + [step - 1]
        p, _, _ = e.encode_chunk(ids, torch.cat(xs))
        for j, i in enumerate(which):
            assert np.abs(p[j].cpu().numpy() - z['s_chunk_probs'][i]).max() < 1e-3
    for sid in (s0, s1):
        _, cnn = e.stream_export_cache(sid)
        assert np.abs(cnn.cpu().numpy() - z['s_chunk_cnn']).max() < 1e-3
        e.stream_close(sid)


def _fused_vs(family, streaming, batch32, keys, one_utterance_too):
    """{norm: [max abs difference between the default launches and the launches under `keys`, per call shape]} and the default
    probabilities of the BatchNorm build's 32-utterance pass"""
    feats, lens_dev, _ = batch32
    diffs, bn_probs = {}, None
    for norm in ('layer_norm', 'batch_norm'):
        e = _engine(family, streaming, norm)
        try:
            calls = [(feats, lens_dev)] + ([(feats[:1].contiguous(), lens_dev[:1].contiguous())] if one_utterance_too else [])
            diffs[norm] = []
            for f, l in calls:
                a = e.encode_full(f, l, -1).cpu().numpy()
                with debug_keys(e, **keys):
                    b = e.encode_full(f, l, -1).cpu().numpy()
                diffs[norm].append(0.0 if np.array_equal(a, b) else float(np.abs(a - b).max()))
            if norm == 'batch_norm':
                bn_probs = e.ctc_probs(e.encode_full(feats, lens_dev, -1)).cpu().numpy()
                nv = np.asarray(e.enc_frames(batch32[2]))
        finally:
            e.close()
    print(f'{family} streaming {streaming} default vs {keys}: {diffs}')
    for ln, bn in zip(diffs['layer_norm'], diffs['batch_norm']):
        # the LayerNorm build is the control: where its fused launches equal its separate ones bit for bit, so must the
        # BatchNorm build's; elsewhere the BatchNorm build may differ by no more than the control does
        assert bn <= ln, (diffs, keys)
    return bn_probs, nv


@pytest.mark.parametrize('streaming', [True, False])
def test_conformer_fused_equals_unfused(z, batch32, streaming):
    """Conformer BatchNorm build: the chain + head-stage launches against key no_chain (out-projection, pw1, depthwise + BN + SiLU
    and pw2 as their own launches), on the 32-utterance batch and on one utterance (few rows), and the fixture rows"""
    probs, nv = _fused_vs('conformer', streaming, batch32, {'no_chain': 1}, True)
    ref = z['conf_' + ('s_' if streaming else 'n_') + 'b32_probs']
    assert max(np.abs(probs[b, :nv[b]] - ref[b, :nv[b]]).max() for b in range(3)) < 1e-3


def test_conformer_head_stage_on_the_32_row_kernel(batch32):
    """the 32-row FFN kernel's BatchNorm head stage (key ffn16 = 0) against the 16-row kernel's, and against separate launches"""
    _fused_vs('conformer', True, batch32, {'ffn16': 0}, False)
    _fused_vs('conformer', True, batch32, {'ffn16': 0, 'no_ffn_head': 1}, False)


def test_efficient_fused_equals_unfused(batch32):
    """Efficient Conformer BatchNorm build: key efficient_fused = 0 keeps separate out-projection / pw1 / depthwise / pw2 launches"""
    _fused_vs('efficient_conformer', True, batch32, {'efficient_fused': 0}, False)


@pytest.fixture(scope='module')
def predictor(tmp_path_factory):
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    vpath = os.path.join(tmp_path_factory.mktemp('bn'), 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(V):
            f.write(f'{t}\t1\n')
    cfg = {'encoder_conf': dict(EFF_CONF),
           'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'efficient_conformer', 'streaming': True,
           'decoder': 'ctc_greedy', 'metrics_type': 'cer'}
    sd = synthetic.efficient_conformer_state_dict(0, V, num_blocks=5, cnn_module_norm='batch_norm')
    return MASRPredictor(configs=cfg, use_gpu=True, state_dict=sd)


def _greedy(probs, vocab):
    from oracle import decoders as od
    return od.greedy_decoder(probs, vocab)[1]


def test_facade_reaches_the_engine_and_decodes_the_fixture(predictor, eff, z):
    """the YAML key arrives at the engine through MASRPredictor; the fixture's own probabilities and the engine's give the same
    greedy transcripts; predict_batch returns the greedy transcripts of the engine's probabilities for its audio"""
    from masr_amd.utils import synthetic
    from oracle import decoders as od
    from oracle.make_golden import golden_inputs
    eng = predictor.predictor.engine
    assert eng.use_model == 'efficient_conformer' and eng.cfg.reserved[4] == 1 and eng.cfg.reserved[0] == 3
    vocab = synthetic.synthetic_vocab(V)
    feats, lens = golden_inputs()
    _, probs = _probs(eng, dev(feats), dev(lens, torch.int32))
    nv = np.asarray(eng.enc_frames(lens.numpy()))
    for b in range(3):
        assert _greedy(probs[b, :nv[b]], vocab) == _greedy(z['s_b3_probs'][b, :nv[b]], vocab)
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    # (equal lengths and the margins of test_gpu_facade.test_predict_batch_equals_single: a ragged batch keeps one padding-
    #  contaminated attention key per utterance, and one utterance alone runs the few-rows launches)
    audios = [pcm[:48000].copy(), pcm[50000:98000].copy()]
    got = predictor.predict_batch(audios)
    for a, r in zip(audios, got):
        one = predictor.predict(audio_data=a.copy())
        assert od.cer(one['text'], r['text']) <= 0.05 and abs(one['score'] - r['score']) < 0.2
    assert any(len(r['text']) > 0 for r in got)


def test_stream_pool_two_sessions_out_of_phase(predictor):
    """StreamPool over the BatchNorm model: two sessions, the second one chunk behind, get the partials of their own predict_stream"""
    from masr_amd.serving import StreamPool
    from oracle import decoders as od
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    audios, step = [pcm[:40000], pcm[30000:62000]], 8000
    want = []
    for a in audios:
        predictor.reset_stream()
        want.append([predictor.predict_stream(audio_data=a[s:s + step].tobytes(), is_end=(s + step >= len(a)))
                     for s in range(0, len(a), step)])
    predictor.reset_stream()
    pool = StreamPool(predictor)
    hs = [pool.open() for _ in audios]
    got = [[] for _ in audios]
    for k in range(len(audios[0]) // step + 2):
        for i, a in enumerate(audios):
            s = (k - i) * step                      # session i starts i steps late
            if 0 <= s < len(a):
                pool.feed(hs[i], a[s:s + step].tobytes(), is_end=(s + step >= len(a)))
        out = pool.step()
        for i, a in enumerate(audios):
            if 0 <= (k - i) * step < len(a):
                got[i].append(out.get(hs[i]))
    for i in range(len(audios)):
        assert len(got[i]) == len(want[i])
        for g_, w_ in zip(got[i], want[i]):
            assert (g_ is None) == (w_ is None or w_['text'] is None)
            if g_ is not None:
                assert od.cer(w_['text'], g_['text']) <= 0.02 and abs(g_['score'] - w_['score']) < 0.05
    for h in hs:
        pool.close(h)


def test_conformer_batch_norm_streaming_stays_refused():
    e = _engine('conformer', True, 'batch_norm')
    try:
        with pytest.raises(MasrError, match='batch_norm'):
            e.stream_open(0)
    finally:
        e.close()
