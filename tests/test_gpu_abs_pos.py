"""The Conformer with pos_enc_layer_type abs_pos / no_pos on the GPU (plain attention: the POS = 0 instantiations of attention.hip;
abs_pos: the sinusoid rows added behind the input projection), at 256 / 4 and 512 / 8, against the reference fixture
tests/golden/conformer_abs_pos_v50.npz (tools/make_abs_pos_golden.py).

Every full-context case and every chunk step holds the budget rule of tests/budget.py with its constant C = 8 over the valid
frames -- truth = the fixture's float64 record, yardstick = its float32 record -- and max abs error < 1e-3 against the float32
record (the bound of every fixture test of test_gpu_parity.py).  The exported caches are compared with the recorded probes."""
import os

import numpy as np
import pytest
import torch

from tests import budget
from masr_amd._lib import MasrError, debug_keys
from tools import make_abs_pos_golden as tool

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
V = tool.V
BUILDS = tool.builds()
STREAMING_BUILDS = [b for b in BUILDS if b[2]]
BUILDS_256 = [b for b in BUILDS if b[1] == 256]
ident = lambda b: tool.prefix(*b).rstrip('_')


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


@pytest.fixture(scope='module')
def z():
    return np.load(tool.OUT)


def _engine(mode, width, streaming, sd=None):
    from masr_amd.engine import HipEngine
    return HipEngine(sd if sd is not None else tool.state_dict(mode, width), dict(tool.encoder_conf(mode, width), linear_units=2048),
                     vocab_size=V, streaming=streaming, use_model='conformer')


@pytest.fixture(scope='module')
def eng():
    """the engine of a build, made on first use"""
    es = {}

    def get(build):
        if build not in es:
            es[build] = _engine(*build)
            assert es[build].cfg.reserved[2] == {'abs': 1, 'no': 2}[build[0]]
        return es[build]
    yield get
    for e in es.values():
        e.close()


def _run(e, feats, lens, chunk=-1):
    enc = e.encode_full(dev(feats), dev(lens, torch.int32), chunk)
    return enc.cpu().numpy(), e.ctc_probs(enc).cpu().numpy()


def _settle(name, z, key, got, mask=None):
    """budget rule against the float64 record, then the 1e-3 bound against the float32 record"""
    budget.check(name, tool.truth(z, key), z[key], got, mask)
    err = np.abs(got - z[key])
    err = float((err[mask] if mask is not None else err).max())
    print(f'{name}: max abs error against the float32 record {err:.3e}')
    assert err < 1e-3, (name, err)


@pytest.mark.parametrize('build', BUILDS, ids=ident)
def test_ragged_batch(eng, z, build):
    k = tool.prefix(*build)
    feats, lens = tool.ragged_inputs()
    enc, probs = _run(eng(build), feats, lens)
    mask = budget.valid_mask(probs.shape, tool.LENS)
    _settle(k + 'b3 probs', z, k + 'b3_probs', probs, mask)
    _settle(k + 'b3 enc', z, k + 'b3_enc', np.ascontiguousarray(enc[:, :, ::tool.PROBE]), mask)


@pytest.mark.parametrize('build', BUILDS_256, ids=ident)
def test_one_utterance_of_67_frames(eng, z, build):
    """T' = 16: a single partial tile of every kernel"""
    k = tool.prefix(*build)
    _, probs = _run(eng(build), tool.single_inputs()[67], torch.tensor([67]))
    _settle(k + 'T=67', z, k + 'single_probs_67', probs)


@pytest.mark.parametrize('build', BUILDS_256, ids=ident)
def test_one_utterance_of_403_frames_on_both_attention_kernels(eng, z, build):
    """T' = 100 takes the key-split kernel by default; attention_fewq = 0 sends it through the tiled one"""
    k, e = tool.prefix(*build), eng(build)
    x = tool.single_inputs()[403]
    _, probs = _run(e, x, torch.tensor([403]))
    _settle(k + 'T=403 key-split', z, k + 'single_probs_403', probs)
    with debug_keys(e, attention_fewq=0):
        _, tiled = _run(e, x, torch.tensor([403]))
    _settle(k + 'T=403 attention_fewq=0', z, k + 'single_probs_403', tiled)


def _check_caches(e, sid, z, k, rcs, width):
    att, cnn = e.stream_export_cache(sid)
    t, H = (48 if rcs < 0 else 16), tool.WIDTHS[width]
    assert tuple(att.shape) == (2, H, t, 128) and tuple(cnn.shape) == (2, 1, width, 14)
    assert np.abs(att.cpu().numpy()[..., ::tool.PROBE] - z[k + f'chunk_att_{rcs}']).max() < 1e-3
    assert np.abs(cnn.cpu().numpy()[:, :, ::tool.CNN_PROBE] - z[k + f'chunk_cnn_{rcs}']).max() < 1e-3


@pytest.mark.parametrize('rcs', tool.CACHE_SIZES)
@pytest.mark.parametrize('build', STREAMING_BUILDS, ids=ident)
def test_chunk_steps_and_caches(eng, z, build, rcs):
    """three steps of one session: the second and third start at offsets 16 and 32 (abs_pos: rows pe[16:32], pe[32:48])"""
    k, e = tool.prefix(*build), eng(build)
    x = tool.single_inputs()[403]
    sid = e.stream_open(0)
    e.stream_set_history(sid, rcs)
    got = np.stack([e.encode_chunk([sid], dev(x[:1, cur:cur + n]))[0][0].cpu().numpy() for cur, n in tool.CHUNKS])
    for i in range(len(tool.CHUNKS)):
        f = budget.check(f'{k}chunk {i} required_cache_size={rcs}', tool.truth(z, k + f'chunk_probs_{rcs}')[i],
                         z[k + f'chunk_probs_{rcs}'][i], got[i])
        assert f['max'] < 1e-3
    assert np.abs(got - z[k + f'chunk_probs_{rcs}']).max() < 1e-3
    _check_caches(e, sid, z, k, rcs, build[1])
    e.stream_close(sid)


@pytest.mark.parametrize('build', STREAMING_BUILDS, ids=ident)
def test_two_sessions_out_of_phase(eng, z, build):
    """two sessions in lock-step calls, the second a chunk behind the first: different offsets in one call, so each stream of an
    abs_pos engine takes its own rows of the table; each repeats the fixture's run"""
    k, e = tool.prefix(*build), eng(build)
    x = tool.single_inputs()[403]
    win = [dev(x[:1, cur:cur + n]) for cur, n in tool.CHUNKS]
    s0, s1 = e.stream_open(0), e.stream_open(0)
    for step in range(len(tool.CHUNKS) + 1):
        ids, xs, which = [], [], []
        if step < len(tool.CHUNKS):
            ids, xs, which = [s0], [win[step]], [step]
        if step >= 1:
            ids, xs, which = ids + [s1], xs + [win[step - 1]], which + [step - 1]
        p, _, _ = e.encode_chunk(ids, torch.cat(xs))
        for j, i in enumerate(which):
            budget.check(f'{k}out of phase step {step} session {j}', tool.truth(z, k + 'chunk_probs_-1')[i], z[k + 'chunk_probs_-1'][i],
                         p[j].cpu().numpy())
            assert np.abs(p[j].cpu().numpy() - z[k + 'chunk_probs_-1'][i]).max() < 1e-3, (step, j)
    for sid in (s0, s1):
        _check_caches(e, sid, z, k, -1, build[1])
        e.stream_close(sid)


def test_both_lanes_give_the_same_bits(eng):
    e = eng(('abs', 256, True))
    feats, lens = tool.ragged_inputs()
    a = _run(e, feats, lens)
    e.select_lane(1)
    try:
        b = _run(e, feats, lens)
    finally:
        e.select_lane(0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_an_abs_pos_checkpoint_under_a_rel_pos_config_names_the_key():
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    with pytest.raises(MasrError, match='pos_enc_layer_type') as ei:
        HipEngine(tool.state_dict('abs', 256), {'num_blocks': 2}, vocab_size=V, streaming=True, use_model='conformer')
    assert 'self_attn.' in str(ei.value)
    with pytest.raises(MasrError, match='pos_enc_layer_type'):
        _engine('abs', 256, True, sd=synthetic.conformer_state_dict(0, V, num_blocks=2))


def test_masr_finalize_names_the_disagreement_in_both_directions():
    """the library's own check, behind the facade's: load a checkpoint of the other kind into a created engine"""
    import ctypes as C
    from masr_amd import _lib
    from masr_amd.engine import HipEngine, _stream
    from masr_amd.utils import synthetic
    for mode, other in (('abs', synthetic.conformer_state_dict(0, V, num_blocks=2)), ('rel', tool.state_dict('abs', 256))):
        e = HipEngine(None, dict(num_blocks=2, **({'pos_enc_layer_type': 'abs_pos'} if mode == 'abs' else {})), vocab_size=V,
                      streaming=True, use_model='conformer')
        try:
            for name, t in other.items():
                e._load(name, t)
            rc = e.lib.masr_finalize(e.h, _stream())
            msg = e.lib.masr_last_error().decode()
            assert rc != 0 and 'pos_enc_layer_type' in msg and 'self_attn.' in msg, msg
        finally:
            e.close()


def test_a_rel_pos_engine_after_an_abs_pos_one_keeps_its_own_arithmetic(eng):
    """the mode is per engine: rel_pos engines built after (and run next to) an abs_pos one match their own references -- the 512 / 8
    fixture of test_gpu_wide.py, and the float64 oracle at 256 / 4"""
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    from oracle import f64
    from tools import make_wide_golden as wide
    feats, lens = tool.ragged_inputs()
    a = eng(('abs', 256, True))
    before = _run(a, feats, lens)[1]
    mask = budget.valid_mask(before.shape, tool.LENS)
    zw = np.load(wide.OUT)
    e = HipEngine(wide.state_dict(), {'output_size': 512, 'attention_heads': 8, 'num_blocks': 2}, vocab_size=V, streaming=True,
                  use_model='conformer')
    try:
        assert e.cfg.reserved[2] == 0
        probs = _run(e, *wide.ragged_inputs())[1]
        assert np.abs(probs - zw['s_b3_probs'])[mask].max() < 1e-3
    finally:
        e.close()
    sd = synthetic.conformer_state_dict(0, V, num_blocks=2)
    r32, r64 = f64.both('conformer', sd, feats, lens, heads=4, streaming=True, decoding_chunk_size=-1)
    e = HipEngine(sd, {'num_blocks': 2}, vocab_size=V, streaming=True, use_model='conformer')
    try:
        probs = _run(e, feats, lens)[1]
        budget.check('rel_pos 256 after abs_pos', r64['probs'], r32['probs'], probs, mask)
        assert np.abs(probs - before)[mask].max() > 1e-2          # (and it is not the abs_pos function)
    finally:
        e.close()
    assert np.array_equal(_run(a, feats, lens)[1], before)


@pytest.fixture(scope='module')
def predictor(tmp_path_factory):
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    vpath = os.path.join(tmp_path_factory.mktemp('abs_pos'), 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(V):
            f.write(f'{t}\t1\n')
    cfg = {'encoder_conf': dict(tool.encoder_conf('abs', 256), linear_units=2048, cnn_module_kernel=15),
           'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'conformer', 'streaming': True,
           'decoder': 'ctc_greedy', 'metrics_type': 'cer'}
    return MASRPredictor(configs=cfg, use_gpu=True, state_dict=tool.state_dict('abs', 256))


def test_facade_predict_batch_agrees_with_predict(predictor):
    from oracle import decoders as od
    assert predictor.predictor.engine.pos_enc_layer_type == 'abs_pos'
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    audios = [pcm[:48000].copy(), pcm[50000:98000].copy()]
    got = predictor.predict_batch(audios)
    for a, r in zip(audios, got):
        one = predictor.predict(audio_data=a.copy())
        assert od.cer(one['text'], r['text']) <= 0.05 and abs(one['score'] - r['score']) < 0.2
    assert any(len(r['text']) > 0 for r in got)


def test_stream_pool_step_with_two_sessions_agrees_with_predict_stream(predictor):
    """two sessions, the second one step late (different offsets in every pool step)"""
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
