"""The Conformer at output_size 512 / attention_heads 8 on the GPU (the width-generic path of engine_conformer.hip + wide.hip): full-context
forwards and chunk steps under the float64 budget rule of tests/budget.py (C = 8, valid frames, truth = the oracle in float64
with heads = 8), parity with the reference fixture tests/golden/conformer_wide_v50.npz (tools/make_wide_golden.py; max abs < 1e-3,
the bound of every fixture test of test_gpu_parity.py), two sessions out of phase, both lanes, and the facade."""
import os

import numpy as np
import pytest
import torch

from tests import budget
from masr_amd._lib import MasrError, debug_keys

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
V, D, HEADS = 50, 512, 8
CONF = {'output_size': D, 'attention_heads': HEADS, 'linear_units': 2048, 'num_blocks': 2}
CHUNKS = [(0, 67), (64, 67), (128, 67)]


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


@pytest.fixture(scope='module')
def z():
    return np.load(os.path.join(GOLDEN, 'conformer_wide_v50.npz'))


@pytest.fixture(scope='module')
def tool():
    from tools import make_wide_golden
    return make_wide_golden


@pytest.fixture(scope='module')
def sd(tool):
    return tool.state_dict()


def _engine(sd, streaming, **conf):
    from masr_amd.engine import HipEngine
    return HipEngine(sd, dict(CONF, **conf), vocab_size=V, streaming=streaming, use_model='conformer')


@pytest.fixture(scope='module')
def eng(sd):
    """the 512 / 8 engines: streaming: True / False"""
    es = {True: _engine(sd, True), False: _engine(sd, False)}
    yield es
    for e in es.values():
        e.close()


@pytest.fixture(scope='module')
def truth(sd, tool):
    """{(case, streaming[, chunk]): (float32 oracle, float64 oracle)} computed once per case"""
    from oracle import f64
    cache = {}

    def get(case, streaming, chunk=-1, sd_=None):
        key = (case, streaming, chunk, id(sd_))
        if key not in cache:
            if case == 'b3':
                feats, lens = tool.ragged_inputs()
            else:
                feats, lens = tool.single_inputs()[case], torch.tensor([case])
            cache[key] = (feats, lens) + f64.both('conformer', sd_ or sd, feats, lens, heads=HEADS, streaming=streaming,
                                                  decoding_chunk_size=chunk)
        return cache[key]
    return get


def _run(e, feats, lens, chunk=-1):
    enc = e.encode_full(dev(feats), dev(lens, torch.int32), chunk)
    return enc.cpu().numpy(), e.ctc_probs(enc).cpu().numpy()


def _budget(name, e, case, streaming, truth, chunk=-1, sd_=None):
    feats, lens, r32, r64 = truth(case, streaming, chunk, sd_)
    enc, probs = _run(e, feats, lens, chunk)
    mask = budget.valid_mask(probs.shape, lens.tolist())
    assert enc.shape == tuple(r64['enc'].shape) and probs.shape == tuple(r64['probs'].shape)
    budget.check(name + ' enc', r64['enc'], r32['enc'], enc, mask)
    budget.check(name + ' probs', r64['probs'], r32['probs'], probs, mask)
    return enc, probs


@pytest.mark.parametrize('streaming', [True, False])
def test_ragged_batch_budget_and_fixture(eng, z, truth, streaming):
    k = 's_' if streaming else 'n_'
    enc, probs = _budget(f'wide b3 streaming={streaming}', eng[streaming], 'b3', streaming, truth)
    mask = budget.valid_mask(probs.shape, [131, 99, 67])
    err_p = np.abs(probs - z[k + 'b3_probs'])[mask].max()
    err_e = np.abs(enc[:, :, ::8] - z[k + 'b3_enc'])[mask].max()
    print(f'B = 3, streaming {streaming}: fixture probs max err {err_p:.3e}, encoder probe max err {err_e:.3e}')
    assert err_p < 1e-3 and err_e < 1e-3


def test_decoding_chunk_size_16(eng, truth):
    _budget('wide b3 chunk=16', eng[True], 'b3', True, truth, chunk=16)


@pytest.mark.parametrize('streaming', [True, False])
def test_one_utterance_of_67_frames(eng, z, truth, streaming):
    """T' = 16: a single partial tile of every kernel"""
    _, probs = _budget(f'wide T=67 streaming={streaming}', eng[streaming], 67, streaming, truth)
    assert np.abs(probs - z[('s_' if streaming else 'n_') + 'single_probs_67']).max() < 1e-3


@pytest.mark.parametrize('streaming', [True, False])
def test_one_utterance_of_403_frames_on_both_attention_kernels(eng, z, truth, streaming):
    """T' = 100 takes the key-split attention kernel by default; attention_fewq = 0 sends it through the tiled one: both write
    the 512-wide output rows"""
    e = eng[streaming]
    ref = z[('s_' if streaming else 'n_') + 'single_probs_403']
    _, probs = _budget(f'wide T=403 streaming={streaming}', e, 403, streaming, truth)
    assert np.abs(probs - ref).max() < 1e-3
    with debug_keys(e, attention_fewq=0):
        _, probs = _budget(f'wide T=403 streaming={streaming} attention_fewq=0', e, 403, streaming, truth)
    assert np.abs(probs - ref).max() < 1e-3


def test_linear_units_384(truth):
    """d_ff a multiple of 128 but not of 256"""
    from masr_amd.utils import synthetic
    sd384 = synthetic.conformer_state_dict(0, V, d=D, heads=HEADS, d_ff=384, num_blocks=2)
    e = _engine(sd384, True, linear_units=384)
    try:
        _budget('wide b3 d_ff=384', e, 'b3', True, truth, sd_=sd384)
    finally:
        e.close()


def _oracle_chunks(sd, x, rcs, dtype):
    """the chunk steps through oracle.conformer.get_encoder_out_chunk with heads = 8 in ``dtype`` -> probabilities [3, 16, V]"""
    from oracle import conformer as oc, f64
    sdd = f64.cast_state_dict(sd, dtype)
    att, cnn, off, out = torch.zeros(0, 0, 0, 0, dtype=dtype), torch.zeros(0, 0, 0, 0, dtype=dtype), 0, []
    with torch.no_grad():
        for cur, n in CHUNKS:
            p, att, cnn = oc.get_encoder_out_chunk(sdd, x[:1, cur:cur + n].to(dtype), off, rcs, att, cnn, heads=HEADS)
            off += p.shape[1]
            out.append(p[0])
    return torch.stack(out)


@pytest.fixture(scope='module')
def chunk_truth(sd, tool):
    x = tool.single_inputs()[403]
    return x, {r: (_oracle_chunks(sd, x, r, torch.float32), _oracle_chunks(sd, x, r, torch.float64)) for r in (-1, 16)}


@pytest.mark.parametrize('rcs', [-1, 16])
def test_chunk_steps_and_caches(eng, z, chunk_truth, rcs):
    e = eng[True]
    x, both = chunk_truth
    sid = e.stream_open(0)
    e.stream_set_history(sid, rcs)
    got = np.stack([e.encode_chunk([sid], dev(x[:1, cur:cur + n]))[0][0].cpu().numpy() for cur, n in CHUNKS])
    budget.check(f'wide chunks required_cache_size={rcs}', both[rcs][1], both[rcs][0], got)
    assert np.abs(got - z[f's_chunk_probs_{rcs}']).max() < 1e-3
    att, cnn = e.stream_export_cache(sid)
    t = 48 if rcs < 0 else 16
    assert tuple(att.shape) == z[f's_chunk_att_{rcs}'].shape == (2, 8, t, 128)
    assert tuple(cnn.shape) == z[f's_chunk_cnn_{rcs}'].shape == (2, 1, 512, 14)
    assert np.abs(att.cpu().numpy() - z[f's_chunk_att_{rcs}']).max() < 1e-3
    assert np.abs(cnn.cpu().numpy() - z[f's_chunk_cnn_{rcs}']).max() < 1e-3
    e.stream_close(sid)


def test_two_sessions_out_of_phase(eng, z, tool):
    """two sessions of one engine in lock-step calls, the second a chunk behind the first: each repeats the fixture's run"""
    e = eng[True]
    x = tool.single_inputs()[403]
    win = [dev(x[:1, cur:cur + n]) for cur, n in CHUNKS]
    s0, s1 = e.stream_open(0), e.stream_open(0)
    for step in range(len(CHUNKS) + 1):
        ids, xs, which = [], [], []
        if step < len(CHUNKS):
            ids, xs, which = [s0], [win[step]], [step]
        if step >= 1:
            ids, xs, which = ids + [s1], xs + [win[step - 1]], which + [step - 1]
        p, _, _ = e.encode_chunk(ids, torch.cat(xs))
        for j, i in enumerate(which):
            assert np.abs(p[j].cpu().numpy() - z['s_chunk_probs_-1'][i]).max() < 1e-3, (step, j)
    for sid in (s0, s1):
        att, cnn = e.stream_export_cache(sid)
        assert np.abs(att.cpu().numpy() - z['s_chunk_att_-1']).max() < 1e-3
        assert np.abs(cnn.cpu().numpy() - z['s_chunk_cnn_-1']).max() < 1e-3
        e.stream_close(sid)


def test_both_lanes_give_the_same_bits(eng, tool):
    e = eng[True]
    feats, lens = tool.ragged_inputs()
    a = _run(e, feats, lens)
    e.select_lane(1)
    try:
        b = _run(e, feats, lens)
    finally:
        e.select_lane(0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_a_256_checkpoint_under_a_512_config_names_the_tensor():
    from masr_amd.utils import synthetic
    sd256 = synthetic.conformer_state_dict(0, V, num_blocks=2)
    with pytest.raises(MasrError, match=r'tensor encoder\.embed\.conv\.0\.weight'):
        _engine(sd256, True)


@pytest.fixture(scope='module')
def predictor(tmp_path_factory, sd):
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    vpath = os.path.join(tmp_path_factory.mktemp('wide'), 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(V):
            f.write(f'{t}\t1\n')
    cfg = {'encoder_conf': dict(CONF, cnn_module_kernel=15),
           'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'conformer', 'streaming': True,
           'decoder': 'ctc_greedy', 'metrics_type': 'cer'}
    return MASRPredictor(configs=cfg, use_gpu=True, state_dict=sd)


def test_facade_predict_batch_agrees_with_predict(predictor):
    from oracle import decoders as od
    eng_ = predictor.predictor.engine
    assert eng_.d_model == D and eng_.heads == HEADS
    pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
    audios = [pcm[:48000].copy(), pcm[50000:98000].copy()]
    got = predictor.predict_batch(audios)
    for a, r in zip(audios, got):
        one = predictor.predict(audio_data=a.copy())
        assert od.cer(one['text'], r['text']) <= 0.05 and abs(one['score'] - r['score']) < 0.2
    assert any(len(r['text']) > 0 for r in got)


def test_stream_pool_two_sessions_agree_with_predict_stream(predictor):
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
