"""GPU: the encoders at layer layouts off the shipped ones -- the Squeezeformer's reduce_idx / recover_idx and the Efficient
Conformer's stride layer / leading grouped layers (tools/make_layout_golden.py lists them) -- under the budget rule of tests/budget.py
(C = 8 against the float64 oracle, no other tolerance): full context on two ragged batches whose T' = 34 / 35 is even and odd and
1 / 2 mod 3, chunk steps with their exported caches and stream counters, the row-block kernel routes forced by their switches, one
serving-pool session per family, and the refusals of the layouts the engine does not take, through HipEngine.

Every case prints its figures before it asserts (``BUDGET ...``); ``MASR_BUDGET_TABLE=<path>`` writes them as a markdown table
(docs/LAB_NOTES.md section 17b keeps the one measured when this module was added)."""
import os
import time

import numpy as np
import pytest
import torch

from masr_amd._lib import MasrError, debug_keys
from tests import budget
from tests.test_gpu_f64_budget import ROWS, dev, held, settle
from tests.test_layouts_cpu import KEY, REFUSALS
from tools import make_layout_golden as tool

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
BUILDS = [(l, s) for l in tool.LAYOUTS for s in (True, False)]
IDS = [f'{tool.name_of(l)}_{"s" if s else "n"}' for l, s in BUILDS]
STREAMED = {'efficient_conformer': ('efficient_conformer', 5, 2, 1), 'squeezeformer': ('squeezeformer', 4, 1, 2)}   # the extra runs
SHIPPED = ('efficient_conformer', 5, 3, 4)          # the control of the fused-launch comparison (tests/test_gpu_efficient_bn.py)
FORCE_ROWS = {'ffn_split_blocks': 0, 'rowgemm_small': 0}


def rate_of(layout):
    return 8 if layout[0] == 'efficient_conformer' else 4


@pytest.fixture(scope='module', autouse=True)
def table():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    t0, first = time.time(), len(ROWS)
    yield
    rows = ROWS[first:]
    print(f'layout module: {time.time() - t0:.0f} s wall, {len(rows)} figures', flush=True)
    path = os.environ.get('MASR_BUDGET_TABLE')
    if path:
        with open(path, 'w') as f:
            f.write('| case | output | max err | ref max err | ratio max | ratio rms | C |\n|---|---|---|---|---|---|---|\n')
            for case, key, r in rows:
                f.write(f'| {case} | {key} | {r["max"]:.2e} | {r["max_ref"]:.2e} | {r["ratio_max"]:.2f} | {r["ratio_rms"]:.2f} | '
                        f'{r["c"]:g} |\n')


@pytest.fixture(scope='module')
def engines():
    """engines of this module by (layout, streaming), built on first use and closed at the end"""
    from masr_amd.engine import HipEngine
    cache = {}

    def get(layout, streaming):
        if (layout, streaming) not in cache:
            sd = tool.state_dict(layout, streaming)
            cache[layout, streaming] = (HipEngine(sd, tool.encoder_conf(layout), vocab_size=tool.V, streaming=streaming,
                                                  use_model=layout[0]), sd)
        return cache[layout, streaming]
    yield get
    for e, _ in cache.values():
        e.close()


@pytest.fixture(scope='module')
def reference():
    """(float32, float64) oracle results of the full-context cases, computed once and left unchanged"""
    from oracle import f64
    cache = {}

    def get(layout, streaming, T, chunk=-1):
        key = (layout, streaming, T, chunk)
        if key not in cache:
            feats, lens = tool.ragged_batch(T)
            kw = tool.oracle_kw(layout, streaming)
            if chunk > 0:
                kw['decoding_chunk_size'] = chunk
            cache[key] = f64.both(layout[0], tool.state_dict(layout, streaming), feats, lens, **kw)
        return cache[key]
    return get


def run_full(case, e, layout, ref, T, chunk=-1):
    """encode_full + ctc_probs on the batch of T frames: shapes and frame counts against the oracle's, enc and probs under the
    rule, the argmax where the float64 margin decides it -> (figures, enc on the host)"""
    r32, r64 = ref
    feats, lens = tool.ragged_batch(T)
    assert int(lens[0]) == T
    enc = e.encode_full(dev(feats), dev(lens, torch.int32), chunk)
    probs, idx, _ = e.ctc_probs(enc, want_argmax=True)
    n = r64['enc'].shape[1]
    assert tuple(enc.shape) == tuple(r64['enc'].shape) and tuple(probs.shape) == tuple(r64['probs'].shape)
    from masr_amd.engine import C, check
    got = C.c_int32()
    check(e.lib.masr_encoder_frames(e.h, T, C.byref(got)))
    assert got.value == n == e.out_frames(T), (got.value, n)
    assert e.frame_reduction() == rate_of(layout)
    mask = budget.valid_mask(r64['enc'].shape, lens, rate_of(layout))
    assert mask[0].all()
    res = [(case, k, held(case, k, r64[k], r32[k], g, mask)) for k, g in (('enc', enc), ('probs', probs))]
    e_ref = np.abs(budget.as64(r32['probs']) - budget.as64(r64['probs']))[mask].max()
    decided = budget.argmax_margin(r64['probs'], e_ref) & mask
    assert 1 - decided[mask].mean() <= 0.02, case
    want = budget.as64(r64['probs']).argmax(-1)
    assert (idx.cpu().numpy().reshape(want.shape)[decided] == want[decided]).all(), case
    return res, enc.cpu().numpy()


# ---- full context, default launches and the row-block routes --------------------------------------------------------------------
@pytest.mark.parametrize('T', tool.T_BATCH)
@pytest.mark.parametrize('layout,streaming', BUILDS, ids=IDS)
def test_full_context(engines, reference, layout, streaming, T):
    e, _ = engines(layout, streaming)
    name = f'{tool.name_of(layout)} {"s" if streaming else "n"} T={T}'
    ref = reference(layout, streaming, T)
    res, _ = run_full(name, e, layout, ref, T)
    if streaming and layout in STREAMED.values():
        res += run_full(f'{name} chunk 16', e, layout, reference(layout, streaming, T, 16), T, 16)[0]
    settle(res)


@pytest.mark.parametrize('T', tool.T_BATCH)
@pytest.mark.parametrize('layout,streaming', [b for b in BUILDS if b[0][0] == 'squeezeformer'],
                         ids=[i for i, b in zip(IDS, BUILDS) if b[0][0] == 'squeezeformer'])
def test_squeezeformer_fused_stages_are_bit_identical(engines, reference, layout, streaming, T):
    """sqz_fused_blocks = 1 forces the fused stage kernels at these row counts (the default takes the separate launches), 0 never
    takes them: the same bits, as sqz_layer.hip promises -- whether the next layer's QKV projection rides along depends on exactly
    these indices.  The promise is about the launches the stages restate, so the separate side is held on them, as
    tests/test_gpu_ffn_dff.py::test_squeezeformer_fused_and_separate does: the full FFN kernel (ffn_split_blocks = 0), no K-split
    projection (rowgemm_small = 0), and the padded frames computed on both sides (skip_padding = 0)."""
    e, _ = engines(layout, streaming)
    name = f'{tool.name_of(layout)} {"s" if streaming else "n"} T={T}'
    ref = reference(layout, streaming, T)
    with debug_keys(e, dict(FORCE_ROWS, skip_padding=0, sqz_fused_blocks=1)):
        res, fused = run_full(f'{name} fused stages', e, layout, ref, T)
    with debug_keys(e, dict(FORCE_ROWS, skip_padding=0, sqz_fused_blocks=0)):
        res0, plain = run_full(f'{name} separate launches', e, layout, ref, T)
    settle(res + res0)
    assert np.array_equal(fused, plain), float(np.abs(fused - plain).max())


@pytest.fixture(scope='module')
def control(engines):
    """max |fused - separate| of the shipped layout's engine per (streaming, T): what the fused launches may differ by"""
    cache = {}

    def get(streaming, T):
        if (streaming, T) not in cache:
            cache[streaming, T] = _fused_diff(engines(SHIPPED, streaming)[0], T)[0]
        return cache[streaming, T]
    return get


def _fused_diff(e, T):
    feats, lens = tool.ragged_batch(T)
    f, l = dev(feats), dev(lens, torch.int32)
    with debug_keys(e, dict(FORCE_ROWS, efficient_fused=1)):
        a = e.encode_full(f, l, -1).cpu().numpy()
    with debug_keys(e, dict(FORCE_ROWS, efficient_fused=0)):
        b = e.encode_full(f, l, -1).cpu().numpy()
    return (0.0 if np.array_equal(a, b) else float(np.abs(a - b).max())), a, b


@pytest.mark.parametrize('T', tool.T_BATCH)
@pytest.mark.parametrize('layout,streaming', [b for b in BUILDS if b[0][0] == 'efficient_conformer'],
                         ids=[i for i, b in zip(IDS, BUILDS) if b[0][0] == 'efficient_conformer'])
def test_efficient_fused_launches(engines, reference, control, layout, streaming, T):
    """ffn_split_blocks = 0 and rowgemm_small = 0 put these few rows on the row-block kernels; efficient_fused 1 against 0 under the
    criterion of tests/test_gpu_efficient_bn.py: the shipped layout is the control -- where its fused launches equal its separate
    ones bit for bit so must this layout's, elsewhere this layout may differ by no more than the control does.  Both runs also go
    under the budget."""
    e, _ = engines(layout, streaming)
    name = f'{tool.name_of(layout)} {"s" if streaming else "n"} T={T}'
    ref = reference(layout, streaming, T)
    with debug_keys(e, dict(FORCE_ROWS, efficient_fused=1)):
        res, fused = run_full(f'{name} row blocks fused', e, layout, ref, T)
    with debug_keys(e, dict(FORCE_ROWS, efficient_fused=0)):
        res0, plain = run_full(f'{name} row blocks separate', e, layout, ref, T)
    diff = 0.0 if np.array_equal(fused, plain) else float(np.abs(fused - plain).max())
    want = control(streaming, T)
    print(f'{name}: fused vs separate {diff:.3e}, shipped layout {want:.3e}')
    settle(res + res0)
    assert diff <= want, (diff, want)


# ---- chunk steps ---------------------------------------------------------------------------------------------------------------
def _counters(e, sid):
    from masr_amd.engine import C, check
    n = C.c_int32()
    check(e.lib.masr_stream_cache_len(e.h, sid, C.byref(n)))
    return e.stream_offset(sid), n.value


@pytest.mark.parametrize('layout', tool.LAYOUTS, ids=[tool.name_of(l) for l in tool.LAYOUTS])
def test_chunk_steps_and_exported_caches(engines, layout):
    """203 frames in three 67-frame windows and a short last one: probabilities of every chunk and the exported caches under the
    rule; the stream's offset and cache length are the oracle's cache sizes"""
    from oracle import f64
    e, sd = engines(layout, True)
    x = tool.chunked_input()[:1]
    (p32, a32, c32), (p64, a64, c64) = f64.both_chunks(layout[0], sd, x, tool.WINDOWS, **tool.oracle_kw(layout))
    sid = e.stream_open(0)
    try:
        outs = [e.encode_chunk([sid], dev(x[:, cur:cur + n]))[0][0] for cur, n in tool.WINDOWS]
        off, clen = _counters(e, sid)
        att, cnn = e.stream_export_cache(sid)
    finally:
        e.stream_close(sid)
    case = f'{tool.name_of(layout)} chunks'
    got = torch.cat(outs)
    assert got.shape == p64.shape and att.shape == a64.shape and cnn.shape == c64.shape
    assert off == clen == a64.shape[2] == 50                       # all history kept: 3 x 16 + 2 input-rate frames
    settle([(case, 'probs', held(case, 'probs', p64, p32, got)), (case, 'att_cache', held(case, 'att_cache', a64, a32, att)),
            (case, 'cnn_cache', held(case, 'cnn_cache', c64, c32, cnn))])


@pytest.mark.parametrize('family', sorted(STREAMED))
def test_two_streams_out_of_phase_with_a_bounded_history(engines, family):
    """required_cache_size = 16, two streams of one engine in lock-step calls, the second a window behind the first and on its own
    utterance: each equals its own single-stream oracle run"""
    from oracle import f64
    layout = STREAMED[family]
    e, sd = engines(layout, True)
    x = tool.chunked_input()
    refs = [f64.both_chunks(family, sd, x[i:i + 1], tool.WINDOWS, required_cache_size=16, **tool.oracle_kw(layout)) for i in range(2)]
    sids = [e.stream_open(0), e.stream_open(0)]
    outs = [[], []]
    try:
        for s in sids:
            e.stream_set_history(s, 16)
        nw = len(tool.WINDOWS)
        for step in range(nw + 1):
            which = [i for i in range(2) if 0 <= step - i < nw]
            same = {tool.WINDOWS[step - i][1] for i in which}
            # (windows of one call have one length: the short last window of stream 0 goes alone, then stream 1's last two)
            calls = [which] if len(same) == 1 else [[i] for i in which]
            for ids in calls:
                xs = torch.cat([x[i:i + 1, tool.WINDOWS[step - i][0]:sum(tool.WINDOWS[step - i])] for i in ids])
                p = e.encode_chunk([sids[i] for i in ids], dev(xs))[0]
                for j, i in enumerate(ids):
                    outs[i].append(p[j])
        res = []
        for i in range(2):
            (p32, a32, c32), (p64, a64, c64) = refs[i]
            off, clen = _counters(e, sids[i])
            att, cnn = e.stream_export_cache(sids[i])
            got = torch.cat(outs[i])
            assert got.shape == p64.shape and att.shape == a64.shape and cnn.shape == c64.shape
            assert off == 50 and clen == a64.shape[2] == 16
            case = f'{tool.name_of(layout)} history 16 stream {i}'
            res += [(case, 'probs', held(case, 'probs', p64, p32, got)), (case, 'att_cache', held(case, 'att_cache', a64, a32, att)),
                    (case, 'cnn_cache', held(case, 'cnn_cache', c64, c32, cnn))]
    finally:
        for s in sids:
            e.stream_close(s)
    settle(res)


# ---- the fixture (recorded from the reference modules) ----------------------------------------------------------------------------
@pytest.mark.parametrize('layout,streaming', BUILDS, ids=IDS)
def test_fixture_rows(engines, layout, streaming):
    """the reference's own probabilities of the T = 139 batch (and of its chunk run), at the documented 1e-3 parity bound"""
    z = np.load(tool.OUT)
    e, _ = engines(layout, streaming)
    feats, lens = tool.ragged_batch(tool.T_BATCH[0])
    probs = e.ctc_probs(e.encode_full(dev(feats), dev(lens, torch.int32), -1)).cpu().numpy()
    want = z[f'{tool.name_of(layout)}_{"s" if streaming else "n"}_b3']
    mask = budget.valid_mask(want.shape, lens, rate_of(layout))
    assert probs.shape == want.shape and np.abs(probs - want)[mask].max() < 1e-3
    if streaming:
        x = tool.chunked_input()[:1]
        sid = e.stream_open(0)
        try:
            got = torch.cat([e.encode_chunk([sid], dev(x[:, cur:cur + n]))[0][0] for cur, n in tool.CHUNKS]).cpu().numpy()
        finally:
            e.stream_close(sid)
        want = z[f'{tool.name_of(layout)}_s_chunks']
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-3


# ---- refusals through the facade -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout,key', REFUSALS, ids=[tool.name_of(l) for l, _ in REFUSALS])
def test_hip_engine_refuses_by_name(layout, key):
    from masr_amd.engine import HipEngine
    with pytest.raises(MasrError) as ei:
        HipEngine(tool.state_dict(layout), tool.encoder_conf(layout), vocab_size=tool.V, streaming=True, use_model=layout[0])
    assert KEY[key] in str(ei.value) and layout[0] in str(ei.value), str(ei.value)


# ---- serving pool ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', sorted(STREAMED))
def test_stream_pool_session_agrees_with_predict_stream(tmp_path, family):
    """one serving-pool session at an off-default layout gets the partials of predict_stream (the pattern and margins of
    tests/test_gpu_wide.py::test_stream_pool_two_sessions_agree_with_predict_stream)"""
    from masr_amd.predict import MASRPredictor
    from masr_amd.serving import StreamPool
    from masr_amd.utils import synthetic
    from oracle import decoders as od
    layout = STREAMED[family]
    vpath = os.path.join(tmp_path, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(tool.V):
            f.write(f'{t}\t1\n')
    cfg = {'encoder_conf': tool.encoder_conf(layout),
           'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': family, 'streaming': True,
           'decoder': 'ctc_greedy', 'metrics_type': 'cer'}
    predictor = MASRPredictor(configs=cfg, use_gpu=True, state_dict=tool.state_dict(layout, True))
    eng = predictor.predictor.engine
    try:
        assert (eng.cfg.reserved[0], eng.cfg.reserved[1]) == (layout[2], layout[3])
        pcm = np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']
        a, step = pcm[:40000], 8000
        predictor.reset_stream()
        want = [predictor.predict_stream(audio_data=a[s:s + step].tobytes(), is_end=(s + step >= len(a))) for s in range(0, len(a), step)]
        predictor.reset_stream()
        pool = StreamPool(predictor)
        h = pool.open()
        got = []
        for s in range(0, len(a), step):
            pool.feed(h, a[s:s + step].tobytes(), is_end=(s + step >= len(a)))
            got.append(pool.step().get(h))
        pool.close(h)
        assert len(got) == len(want) and any(w is not None and w['text'] for w in want)
        for g_, w_ in zip(got, want):
            assert (g_ is None) == (w_ is None or w_['text'] is None)
            if g_ is not None:
                assert od.cer(w_['text'], g_['text']) <= 0.02 and abs(g_['score'] - w_['score']) < 0.05
    finally:
        eng.close()
