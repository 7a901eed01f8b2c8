"""The Conformer with encoder_conf.activation_type relu / gelu / tanh / hardtanh / selu on the GPU: the width-generic layer of
separate launches (csrc/wide.hip + the tiled GEMM) at 256 / 4 and 512 / 8, the activation in the epilogue of the first FFN GEMM and
behind the conv module's LayerNorm.

Every case holds the budget rule of tests/budget.py with its constant C = 8 over the valid frames -- truth = tests/activation_ref.py
in float64, yardstick = the same in float32 -- and, where tests/golden/conformer_activation_v50.npz (recorded from the reference
model built with each activation, tools/make_activation_golden.py) holds the case, max abs error < 1e-3 against the float32
record, the bound of every fixture test."""
import os

import numpy as np
import pytest
import torch

from masr_amd.utils import synthetic
from oracle import f64
from tests import activation_ref as ar
from tests import budget
from tools import make_activation_golden as tool

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
V = tool.V
ACTS = tool.ACTS
CHUNKS = [(0, 67), (64, 67), (128, 67)]


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


@pytest.fixture(scope='module')
def z():
    return np.load(tool.OUT)


def _sd(width, **kw):
    return synthetic.conformer_state_dict(0, V, d=width, heads=tool.WIDTHS[width], num_blocks=tool.BLOCKS, **kw)


def _engine(act, width, streaming, sd=None, **conf):
    from masr_amd.engine import ACTIVATION_TYPES, HipEngine
    c = dict({'output_size': width, 'attention_heads': tool.WIDTHS[width], 'num_blocks': tool.BLOCKS}, **conf)
    if act is not None:
        c['activation_type'] = act
    e = HipEngine(sd if sd is not None else _sd(width), c, vocab_size=V, streaming=streaming, use_model='conformer')
    assert e.cfg.reserved[4] == ACTIVATION_TYPES[act or 'swish'] and e.activation_type == (act or 'swish')
    return e


@pytest.fixture(scope='module')
def eng():
    """the engine of (act, width, streaming) on the default checkpoint, made on first use"""
    es = {}

    def get(act, width, streaming):
        key = (act, width, streaming)
        if key not in es:
            es[key] = _engine(*key)
        return es[key]
    yield get
    for e in es.values():
        e.close()


def _run(e, feats, lens, chunk=-1):
    enc = e.encode_full(dev(feats), dev(lens, torch.int32), chunk)
    return enc.cpu().numpy(), e.ctc_probs(enc).cpu().numpy()


def _inputs(case):
    if case == 'b3':
        return tool.ragged_inputs()
    return tool.single_inputs()[case], torch.tensor([case])


def _budget(name, e, sd, case, act, width, streaming, rate=4, **kw):
    """encoder rows and probabilities of one case under the budget rule -> (enc, probs, valid mask)"""
    feats, lens = _inputs(case)
    r32, r64 = f64.both('conformer', sd, feats, lens, encoder_fn=ar.encoder_full, act=act, heads=tool.WIDTHS[width],
                        streaming=streaming, **kw)
    enc, probs = _run(e, feats, lens, kw.get('decoding_chunk_size', -1))
    assert enc.shape == tuple(r64['enc'].shape) and probs.shape == tuple(r64['probs'].shape)
    mask = budget.valid_mask(probs.shape, lens.tolist(), rate)
    budget.check(name + ' enc', r64['enc'], r32['enc'], enc, mask)
    budget.check(name + ' probs', r64['probs'], r32['probs'], probs, mask)
    return enc, probs, mask


def _fixture(name, z, key, got, mask=None):
    err = np.abs(got - z[key])
    err = float((err[mask] if mask is not None else err).max())
    print(f'{name}: max abs error against the float32 record {key} {err:.3e}')
    assert err < 1e-3, (name, err)


@pytest.mark.parametrize('streaming', [True, False], ids=['s', 'n'])
@pytest.mark.parametrize('width', [256, 512])
@pytest.mark.parametrize('act', ACTS)
def test_ragged_batch(eng, z, act, width, streaming):
    k = tool.prefix(act, width, streaming)
    enc, probs, mask = _budget(k + 'b3', eng(act, width, streaming), _sd(width), 'b3', act, width, streaming)
    _fixture(k + 'b3 probs', z, k + 'b3_probs', probs, mask)
    _fixture(k + 'b3 enc', z, k + 'b3_enc', np.ascontiguousarray(enc[:, :, ::tool.PROBE]), mask)


@pytest.mark.parametrize('act', ACTS)
def test_one_utterance_of_67_frames(eng, z, act):
    """T' = 16: a single partial tile of every kernel"""
    k = tool.prefix(act, 256, True)
    _, probs, _ = _budget(k + 'T=67', eng(act, 256, True), _sd(256), 67, act, 256, True)
    _fixture(k + 'T=67', z, k + 'single_probs_67', probs)


@pytest.mark.parametrize('act', tool.LONG_ACTS)
def test_one_utterance_of_403_frames(eng, z, act):
    """T' = 100: the key-split attention kernel"""
    k = tool.prefix(act, 256, True)
    _, probs, _ = _budget(k + 'T=403', eng(act, 256, True), _sd(256), 403, act, 256, True)
    _fixture(k + 'T=403', z, k + 'single_probs_403', probs)


def test_decoding_chunk_size_16(eng):
    _budget('relu 256 b3 chunk=16', eng('relu', 256, True), _sd(256), 'b3', 'relu', 256, True, decoding_chunk_size=16)


@pytest.mark.parametrize('kernel', [7, 31])
def test_cnn_module_kernel(kernel):
    """7: the 8-tap registers of the run-time tap kernel, 31: its 32"""
    sd = _sd(256, kernel=kernel)
    e = _engine('gelu', 256, True, sd=sd, cnn_module_kernel=kernel)
    try:
        _budget(f'gelu 256 b3 cnn_module_kernel={kernel}', e, sd, 'b3', 'gelu', 256, True, kernel=kernel)
    finally:
        e.close()


def test_abs_pos():
    sd = _sd(256, pos_enc_layer_type='abs_pos')
    e = _engine('relu', 256, True, sd=sd, pos_enc_layer_type='abs_pos')
    try:
        _budget('relu 256 b3 abs_pos', e, sd, 'b3', 'relu', 256, True, pos_enc='abs_pos')
    finally:
        e.close()


def test_input_layer_conv2d6():
    sd = _sd(256, input_layer='conv2d6')
    e = _engine('relu', 256, True, sd=sd, input_layer='conv2d6')
    try:
        _budget('relu 256 T=67 conv2d6', e, sd, 67, 'relu', 256, True, rate=6, input_layer='conv2d6')
    finally:
        e.close()


def _session(e, win, rcs=-1):
    sid = e.stream_open(0)
    e.stream_set_history(sid, rcs)
    got = np.stack([e.encode_chunk([sid], w)[0][0].cpu().numpy() for w in win])
    shapes = tuple(tuple(c.shape) for c in e.stream_export_cache(sid))
    e.stream_close(sid)
    return got, shapes


@pytest.mark.parametrize('act,width', [(a, 256) for a in ACTS] + [('relu', 512)])
def test_chunk_steps(eng, act, width):
    """three steps of one session against the helper's chunk runner; the exported caches have the shapes of a swish engine; two
    sessions a chunk apart in one call give each session's own bits"""
    e, x = eng(act, width, True), tool.single_inputs()[403]
    win = [dev(x[:1, cur:cur + n]) for cur, n in CHUNKS]
    (r32, _, _), (r64, _, _) = ar.both_chunks(_sd(width), x, CHUNKS, act, required_cache_size=-1, heads=tool.WIDTHS[width])
    got, shapes = _session(e, win)
    budget.check(f'{act} {width} chunk steps', r64, r32, got.reshape(-1, V))
    swish = eng(None, width, True)
    assert shapes == _session(swish, win)[1] == ((2, tool.WIDTHS[width], 48, 128), (2, 1, width, 14))
    s0, s1 = e.stream_open(0), e.stream_open(0)
    for sid in (s0, s1):
        e.stream_set_history(sid, -1)
    for step in range(len(CHUNKS) + 1):
        ids, xs, which = [], [], []
        if step < len(CHUNKS):
            ids, xs, which = [s0], [win[step]], [step]
        if step >= 1:
            ids, xs, which = ids + [s1], xs + [win[step - 1]], which + [step - 1]
        p, _, _ = e.encode_chunk(ids, torch.cat(xs))
        for j, i in enumerate(which):
            assert np.array_equal(p[j].cpu().numpy(), got[i]), (step, j)
    for sid in (s0, s1):
        e.stream_close(sid)


def test_both_lanes_give_the_same_bits(eng):
    e = eng('relu', 256, True)
    feats, lens = tool.ragged_inputs()
    a = _run(e, feats, lens)
    e.select_lane(1)
    try:
        b = _run(e, feats, lens)
    finally:
        e.select_lane(0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('width', [256, 512])
def test_swish_by_name_is_the_absent_key(eng, width):
    """{'activation_type': 'swish'} and an absent key are one configuration: the same slot value and the same encoder bits"""
    feats, lens = tool.ragged_inputs()
    named, absent = eng('swish', width, True), eng(None, width, True)
    assert named.cfg.reserved[4] == absent.cfg.reserved[4] == 0
    assert np.array_equal(_run(named, feats, lens)[0], _run(absent, feats, lens)[0])
    # and relu is another function of the same weights
    assert np.abs(_run(eng('relu', width, True), feats, lens)[1] - _run(absent, feats, lens)[1]).max() > 1e-3


@pytest.fixture(scope='module')
def predictor(tmp_path_factory):
    from masr_amd.predict import MASRPredictor
    vpath = os.path.join(tmp_path_factory.mktemp('activation'), 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(V):
            f.write(f'{t}\t1\n')
    cfg = {'encoder_conf': dict(tool.encoder_conf('relu', 256), linear_units=2048, cnn_module_kernel=15),
           'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'conformer', 'streaming': True,
           'decoder': 'ctc_greedy', 'metrics_type': 'cer'}
    return MASRPredictor(configs=cfg, use_gpu=True, state_dict=_sd(256))


def test_facade_predict_batch_agrees_with_predict(predictor):
    from oracle import decoders as od
    assert predictor.predictor.engine.activation_type == 'relu'
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    audios = [pcm[:48000].copy(), pcm[50000:98000].copy()]
    got = predictor.predict_batch(audios)
    for a, r in zip(audios, got):
        one = predictor.predict(audio_data=a.copy())
        assert od.cer(one['text'], r['text']) <= 0.05 and abs(one['score'] - r['score']) < 0.2
    assert any(len(r['text']) > 0 for r in got)


def test_stream_pool_two_sessions_agree_with_predict_stream(predictor):
    """predict_stream over the same audio, then the pool with the second session one step late"""
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
