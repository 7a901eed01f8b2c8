"""encoder_conf.cnn_module_kernel off the shipped values on the GPU: Conformer 256 / 4 and 512 / 8 and the Squeezeformer, full
context and chunk steps, under the float64 budget rule of tests/budget.py (C = 8, valid frames, truth = the oracle in float64 with
kernel = K), and within max abs < 1e-3 of the reference fixture tests/golden/conv_kernel_v50.npz
(tools/make_conv_kernel_golden.py), the bound of every fixture test here.

Which depthwise code a case runs (LayerNorm Conformer at 256): below 112 row blocks, and in the chunk steps, the depthwise prologue
of the small-M row kernel (rowgemm_small.hip: up to 15 taps in registers, 16 .. 32 streamed), so the few-row cases of any K run
that; the separate launch -- dwconv_ln_silu_kernel<31> for 31 taps, dwconv_ln_silu_taps_kernel<8 / 16 / 32> for every other count --
runs with few_rows_path = 0 (test_conformer_separate_depthwise_launch: every class, both norms' history modes, T' < K - 1), in the
B = 129 case, in every batch_norm case and in the Squeezeformer's separate launches.  At 512 / 8 every case runs
dwconv_ln_silu_wide_kernel<15> or dwconv_ln_silu_wide_taps_kernel<8 / 16 / 32>."""
import os

import numpy as np
import pytest
import torch

from tests import budget
from masr_amd import _lib
from masr_amd._lib import debug_keys

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
V = 50
CHUNKS = [(0, 67), (64, 67), (128, 67)]
B_ = {True: 's', False: 'n'}


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


@pytest.fixture(scope='module')
def z():
    return np.load(os.path.join(GOLDEN, 'conv_kernel_v50.npz'))


@pytest.fixture(scope='module')
def tool():
    from tools import make_conv_kernel_golden
    return make_conv_kernel_golden


def _conformer(sd, K, streaming, **conf):
    from masr_amd.engine import HipEngine
    wide = sd['encoder.after_norm.weight'].shape[0] == 512
    c = {'output_size': 512 if wide else 256, 'attention_heads': 8 if wide else 4, 'linear_units': 2048, 'num_blocks': 2,
         'cnn_module_kernel': K}
    return HipEngine(sd, dict(c, **conf), vocab_size=V, streaming=streaming, use_model='conformer')


def _squeezeformer(sd, K, streaming):
    from masr_amd.engine import HipEngine
    c = {'encoder_dim': 256, 'attention_heads': 4, 'feed_forward_expansion_factor': 8, 'num_blocks': 4, 'cnn_module_kernel': K,
         'reduce_idx': 1, 'recover_idx': 3}
    return HipEngine(sd, c, vocab_size=V, streaming=streaming, use_model='squeezeformer')


def _inputs(tool, case):
    if case == 'b3':
        return tool.ragged_inputs()
    return tool.single_inputs()[case], torch.tensor([case])


def _run(e, feats, lens):
    enc = e.encode_full(dev(feats), dev(lens, torch.int32), -1)
    return enc.cpu().numpy(), e.ctc_probs(enc).cpu().numpy()


def _budget(name, e, family, sd, feats, lens, **kw):
    """one full-context forward against the float32 / float64 oracle under the budget -> probabilities"""
    from oracle import f64
    r32, r64 = f64.both(family, sd, feats, lens, **kw)
    enc, probs = _run(e, feats, lens)
    mask = budget.valid_mask(probs.shape, lens.tolist())
    assert enc.shape == tuple(r64['enc'].shape) and probs.shape == tuple(r64['probs'].shape)
    budget.check(name + ' enc', r64['enc'], r32['enc'], enc, mask)
    budget.check(name + ' probs', r64['probs'], r32['probs'], probs, mask)
    return probs, mask


def _fixture(name, probs, mask, ref):
    err = np.abs(probs - ref)[mask].max()
    print(f'{name}: fixture probs max err {err:.3e}')
    assert err < 1e-3


# ---- Conformer 256 / 4, full context --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,streaming', [(31, True), (31, False), (9, True), (9, False), (8, True), (3, True)])
def test_conformer_full_context(tool, z, K, streaming):
    """the ragged batch (T' = 32 / 24 / 16), 67 frames (T' = 16: shorter than the 30-row halo of K = 31, one partial tile) and 403
    frames (T' = 100: across tile edges)"""
    sd = tool.conformer_sd(K)
    e = _conformer(sd, K, streaming)
    try:
        for case in ('b3', 67, 403):
            feats, lens = _inputs(tool, case)
            name = f'conformer K={K} streaming={streaming} {case}'
            probs, mask = _budget(name, e, 'conformer', sd, feats, lens, kernel=K, streaming=streaming)
            _fixture(name, probs, mask, z[f'c{K}{B_[streaming]}_{case}'])
    finally:
        e.close()


@pytest.mark.parametrize('K,streaming', [(31, False), (31, True), (9, True), (9, False)])
def test_conformer_batch_norm_full_context(tool, z, K, streaming):
    """(the fixture holds one build per K; the other runs under the budget alone)"""
    sd = tool.conformer_sd(K, 'batch_norm')
    e = _conformer(sd, K, streaming, cnn_module_norm='batch_norm')
    try:
        for case in ('b3', 67, 403):
            feats, lens = _inputs(tool, case)
            name = f'conformer batch_norm K={K} streaming={streaming} {case}'
            probs, mask = _budget(name, e, 'conformer', sd, feats, lens, kernel=K, streaming=streaming)
            if case == 'b3' and f'cbn{K}{B_[streaming]}_b3' in z.files:
                _fixture(name, probs, mask, z[f'cbn{K}{B_[streaming]}_b3'])
    finally:
        e.close()


@pytest.mark.parametrize('K,streaming', [(23, False), (20, True), (30, True), (17, False), (9, False), (8, True), (3, True), (3, False)])
def test_conformer_separate_depthwise_launch(tool, K, streaming):
    """few_rows_path = 0 keeps the depthwise conv out of the small-M row kernel's prologue: ffn() launches
    dwconv_ln_silu_taps_kernel -- class 32 (23, 20, 30, 17), 16 (9) and 8 (8, 3), the gconst rows of the offline causal build and the
    zero rows of the symmetric one, on T' = 16 (shorter than K - 1 for the 32 class: one partial tile), the ragged batch and
    T' = 100 (seven tiles, the last partial).  The default path (the prologue) runs next to it under the same budget."""
    from oracle import f64
    sd = tool.conformer_sd(K)
    e = _conformer(sd, K, streaming)
    try:
        for case in (67, 'b3', 403):
            feats, lens = _inputs(tool, case)
            name = f'conformer K={K} streaming={streaming} {case}'
            r32, r64 = f64.both('conformer', sd, feats, lens, kernel=K, streaming=streaming)
            mask = budget.valid_mask(r64['probs'].shape, lens.tolist())
            for keys in ({'few_rows_path': 0}, {}):
                with debug_keys(e, keys):
                    enc, probs = _run(e, feats, lens)
                budget.check(f'{name} {keys} enc', r64['enc'], r32['enc'], enc, mask)
                budget.check(f'{name} {keys} probs', r64['probs'], r32['probs'], probs, mask)
    finally:
        e.close()


# ---- chunk steps ----------------------------------------------------------------------------------------------------------------
def _oracle_chunks(module, sd, x, rcs, dtype, **kw):
    """the chunk steps through the oracle in ``dtype`` -> (probabilities [3, 16, V], att cache, cnn cache)"""
    from oracle import f64
    sdd = f64.cast_state_dict(sd, dtype)
    att, cnn, off, out = torch.zeros(0, 0, 0, 0, dtype=dtype), torch.zeros(0, 0, 0, 0, dtype=dtype), 0, []
    with torch.no_grad():
        for cur, n in CHUNKS:
            p, att, cnn = module.get_encoder_out_chunk(sdd, x[:1, cur:cur + n].to(dtype), off, rcs, att, cnn, **kw)
            off += p.shape[1]
            out.append(p[0])
    return torch.stack(out), att, cnn


def _chunk_case(name, e, module, sd, x, rcs, ref, cnn_shape, **kw):
    """one session over the three windows under the budget and against the fixture; the exported cnn cache against the oracle's;
    then two sessions out of phase: each one's probabilities hold the same budget (two streams in one call are other launches
    than one, so not the same bits) and its caches equal the single session's within the cache bound"""
    o32 = _oracle_chunks(module, sd, x, rcs, torch.float32, **kw)
    o64 = _oracle_chunks(module, sd, x, rcs, torch.float64, **kw)
    win = [dev(x[:1, cur:cur + n]) for cur, n in CHUNKS]
    sid = e.stream_open(0)
    if rcs >= 0:
        e.stream_set_history(sid, rcs)
    got = np.stack([e.encode_chunk([sid], w)[0][0].cpu().numpy() for w in win])
    budget.check(name, o64[0], o32[0], got)
    err = np.abs(got - ref).max()
    print(f'{name}: fixture probs max err {err:.3e}')
    assert err < 1e-3
    att, cnn = (t.cpu().numpy() for t in e.stream_export_cache(sid))
    e.stream_close(sid)
    assert cnn.shape == cnn_shape == tuple(o32[2].shape), (cnn.shape, cnn_shape, o32[2].shape)
    assert att.shape == tuple(o32[1].shape)
    assert np.abs(cnn - o32[2].numpy()).max() < 1e-3
    s0, s1 = e.stream_open(0), e.stream_open(0)
    for sid in (s0, s1):
        if rcs >= 0:
            e.stream_set_history(sid, rcs)
    both = [[None] * len(CHUNKS), [None] * len(CHUNKS)]
    for step in range(len(CHUNKS) + 1):
        ids, xs, which = [], [], []
        if step < len(CHUNKS):
            ids, xs, which = [s0], [win[step]], [step]
        if step >= 1:
            ids, xs, which = ids + [s1], xs + [win[step - 1]], which + [step - 1]
        p, _, _ = e.encode_chunk(ids, torch.cat(xs))
        for j, i in enumerate(which):
            both[0 if ids[j] == s0 else 1][i] = p[j].cpu().numpy()
    for k in (0, 1):
        budget.check(f'{name} session {k} of two', o64[0], o32[0], np.stack(both[k]))
    for sid in (s0, s1):
        a2, c2 = (t.cpu().numpy() for t in e.stream_export_cache(sid))
        assert np.abs(a2 - att).max() < 1e-3 and np.abs(c2 - cnn).max() < 1e-3
        e.stream_close(sid)
    return att, cnn


@pytest.mark.parametrize('K', [31, 8])
def test_conformer_chunk_steps(tool, z, K):
    from oracle import conformer as oc
    sd = tool.conformer_sd(K)
    x = tool.single_inputs()[403]
    e = _conformer(sd, K, True)
    try:
        for rcs in (-1, 16):
            att, cnn = _chunk_case(f'conformer K={K} chunks required_cache_size={rcs}', e, oc, sd, x, rcs, z[f'c{K}_chunk_{rcs}'],
                                   (2, 1, 256, K - 1), kernel=K)
            if (K, rcs) == (8, 16):
                assert np.abs(att - z['c8_chunk_att_16']).max() < 1e-3 and np.abs(cnn - z['c8_chunk_cnn_16']).max() < 1e-3
    finally:
        e.close()


# ---- Conformer 512 / 8 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('streaming', [True, False])
def test_wide_conformer_full_context(tool, z, streaming):
    sd = tool.conformer_sd(31, wide=True)
    e = _conformer(sd, 31, streaming)
    try:
        for case in ('b3', 67, 403):
            feats, lens = _inputs(tool, case)
            name = f'conformer 512 / 8 K=31 streaming={streaming} {case}'
            probs, mask = _budget(name, e, 'conformer', sd, feats, lens, kernel=31, heads=8, streaming=streaming)
            if case != 403:               # (the fixture holds the two short inputs at this width)
                _fixture(name, probs, mask, z[f'w31{B_[streaming]}_{case}'])
    finally:
        e.close()


@pytest.mark.parametrize('K,streaming', [(9, True), (9, False), (8, True), (23, False)])
def test_wide_conformer_other_classes(tool, K, streaming):
    """dwconv_ln_silu_wide_taps_kernel<512, 16 / 8 / 32> (K = 31 above runs the 32 class only), under the budget"""
    sd = tool.conformer_sd(K, wide=True)
    e = _conformer(sd, K, streaming)
    try:
        for case in (67, 'b3'):
            feats, lens = _inputs(tool, case)
            _budget(f'conformer 512 / 8 K={K} streaming={streaming} {case}', e, 'conformer', sd, feats, lens, kernel=K, heads=8,
                    streaming=streaming)
    finally:
        e.close()


def test_wide_conformer_chunk_steps(tool, z):
    from oracle import conformer as oc
    sd = tool.conformer_sd(31, wide=True)
    e = _conformer(sd, 31, True)
    try:
        _chunk_case('conformer 512 / 8 K=31 chunks', e, oc, sd, tool.single_inputs()[403], -1, z['w31_chunk_-1'], (2, 1, 512, 30),
                    kernel=31, heads=8)
    finally:
        e.close()


# ---- Squeezeformer --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,streaming', [(15, True), (15, False), (8, True), (7, False)])
def test_squeezeformer_full_context(tool, z, K, streaming):
    """reduce_idx 1 / recover_idx 3: layers 1 and 2 run the depthwise kernel at half rate (T' = 16 / 8 for the ragged batch).
    K = 15 additionally with the fused stage kernels (sqz_layer.hip carries 15 taps; threshold lowered to one row block) and with
    the separate launches (threshold 0); the default threshold sends these few rows through the separate launches too."""
    sd = tool.squeezeformer_sd(K, streaming)
    e = _squeezeformer(sd, K, streaming)
    kw = dict(tool.SQZ_IDX, kernel=K, causal=streaming)
    try:
        for case in ('b3', 67, 403):
            feats, lens = _inputs(tool, case)
            name = f'squeezeformer K={K} streaming={streaming} {case}'
            probs, mask = _budget(name, e, 'squeezeformer', sd, feats, lens, **kw)
            _fixture(name, probs, mask, z[f'q{K}{B_[streaming]}_{case}'])
        if K == 15:
            feats, lens = _inputs(tool, 'b3')
            for blocks in (1, 0):
                with debug_keys(e, sqz_fused_blocks=blocks):
                    name = f'squeezeformer K=15 streaming={streaming} b3 sqz_fused_blocks={blocks}'
                    probs, mask = _budget(name, e, 'squeezeformer', sd, feats, lens, **kw)
                    _fixture(name, probs, mask, z[f'q15{B_[streaming]}_b3'])
    finally:
        e.close()


@pytest.mark.parametrize('K', [15, 8])
def test_squeezeformer_chunk_steps(tool, z, K):
    from oracle import squeezeformer as osq
    sd = tool.squeezeformer_sd(K, True)
    e = _squeezeformer(sd, K, True)
    try:
        _, cnn = _chunk_case(f'squeezeformer K={K} chunks', e, osq, sd, tool.single_inputs()[403], -1, z[f'q{K}_chunk_-1'],
                             (4, 1, 256, K - 1), kernel=K, **tool.SQZ_IDX)
        if K == 8:
            assert np.abs(cnn - z['q8_chunk_cnn_-1']).max() < 1e-3
    finally:
        e.close()


# ---- a size at which K = 15 fuses -----------------------------------------------------------------------------------------------
FULL_B, FULL_T, FULL_DFF = 129, 131, 256        # M = 129 * 32 rows = 129 row blocks of 32


@pytest.mark.parametrize('K', [9, 31])
def test_fallback_at_a_size_that_fuses_for_15(K):
    """129 utterances of 131 frames (T' = 32): M = 4128 rows = 129 row blocks is the smallest count at which ffn_plan runs the full
    launch (nsplit = max(1, 256 / rowblocks) = 1 from 129 row blocks on; 128 still split in two) with the head stage in the kernel
    for 15 taps; for 9 and 31 taps the plan keeps the head out of the kernel and ffn() launches the depthwise kernel and
    pointwise_conv2 in front of the block.  linear_units = 256 keeps the float64 oracle of 4128 rows short."""
    from masr_amd.utils import synthetic
    M = FULL_B * ((((FULL_T - 1) // 2) - 1) // 2)
    assert M == 4128
    p15, below = _lib.ffn_plan(FULL_DFF, M, head_ktaps=15), _lib.ffn_plan(FULL_DFF, M - 32, head_ktaps=15)
    assert p15.nsplit == 1 and p15.head_in_kernel == 1 and below.nsplit > 1 and below.head_in_kernel == 0
    pk = _lib.ffn_plan(FULL_DFF, M, head_ktaps=K)
    assert pk.nsplit == 1 and pk.head_in_kernel == 0
    sd = synthetic.conformer_state_dict(0, V, num_blocks=2, kernel=K, d_ff=FULL_DFF)
    rng = np.random.default_rng(13)
    feats = torch.from_numpy(rng.standard_normal((FULL_B, FULL_T, 80)).astype(np.float32) * 3 + 13)
    lens = torch.full((FULL_B,), FULL_T, dtype=torch.int64)
    lens[1::2] = 99                              # (every second utterance padded: 24 valid frames of 32)
    feats *= (torch.arange(FULL_T)[None, :, None] < lens[:, None, None])
    e = _conformer(sd, K, True, linear_units=FULL_DFF)
    keep = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        _budget(f'conformer K={K} B={FULL_B} full row blocks', e, 'conformer', sd, feats, lens, kernel=K, streaming=True)
    finally:
        torch.set_num_threads(keep)
        e.close()


def test_both_lanes_give_the_same_bits(tool):
    sd = tool.conformer_sd(31)
    e = _conformer(sd, 31, True)
    try:
        feats, lens = tool.ragged_inputs()
        a = _run(e, feats, lens)
        e.select_lane(1)
        try:
            b = _run(e, feats, lens)
        finally:
            e.select_lane(0)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        e.close()


# ---- facade ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def predictor(tmp_path_factory, tool):
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    vpath = os.path.join(tmp_path_factory.mktemp('conv_kernel'), 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(V):
            f.write(f'{t}\t1\n')
    cfg = {'encoder_conf': {'output_size': 256, 'attention_heads': 4, 'linear_units': 2048, 'num_blocks': 2, 'cnn_module_kernel': 31},
           'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'conformer', 'streaming': True,
           'decoder': 'ctc_greedy', 'metrics_type': 'cer'}
    return MASRPredictor(configs=cfg, use_gpu=True, state_dict=tool.conformer_sd(31))


def test_facade_predict_batch_agrees_with_predict(predictor):
    from oracle import decoders as od
    assert predictor.predictor.engine.cnn_kernel == 31
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
