"""GPU: the HIP path under the budget rule of tests/budget.py -- every output is compared with the oracle evaluated in FLOAT64
(oracle/f64.py), and may be at most C = 8 times as far from it as the float32 CPU oracle is (max and rms, valid frames).

The fixed ``< 1e-3`` bars of the other modules stay what they are (the documented contract); they sit two orders of magnitude
above the arithmetic noise and cannot see a wrong eps, a degraded exp / rcp in an epilogue or a softmax that loses bits.
This module is the tighter net beside them: depth ladder (depth 1 = embed + one layer + after-norm is the closest thing to
a per-kernel test the public surface allows), attention modes, chunk steps with their exported caches, the shapes that select
every kernel route, DeepSpeech2 (LSTM / GRU), stress checkpoints that drive the gated epilogues and the softmax where they are
weakest, and single kernels at their edges.  tests/test_f64_budget_cpu.py shows on the CPU that the rule rejects such
defects and accepts a reordered float32 evaluation.

Every case prints its figures before it asserts (``BUDGET ...``); with ``MASR_BUDGET_TABLE=<path>`` the figures of the run
are also written there as a markdown table (docs/LAB_NOTES.md section 17 keeps the one measured when this module was added)."""
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import budget

pytestmark = pytest.mark.gpu

ROWS = []                                    # (case, output, figures) of this run
WINDOWS = [(c, 67) for c in range(0, 331 - 67 + 1, 64)] + [(320, 11)]          # five 67-frame windows and a short last chunk


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def held(case, key, y64, y32, y, mask=None, c_max=None):
    """one output of one case under the rule; the figures are kept for the table whether it holds or not"""
    f = budget.evaluate(y64, y32, y, mask, c_max=c_max)
    ROWS.append((case, key, f))
    print(budget.line(f'{case} {key}', f), flush=True)
    return f


def settle(results):
    over = [budget.line(f'{case} {key}', f) for case, key, f in results if not f['ok']]
    assert not over, 'over budget:\n' + '\n'.join(over)


@pytest.fixture(scope='module', autouse=True)
def table():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    t0 = time.time()
    yield
    print(f'float64 budget module: {time.time() - t0:.0f} s wall, {len(ROWS)} figures', flush=True)
    path = os.environ.get('MASR_BUDGET_TABLE')
    if path:
        with open(path, 'w') as f:
            f.write('| case | output | max err | ref max err | ratio max | ratio rms | C |\n|---|---|---|---|---|---|---|\n')
            for case, key, r in ROWS:
                f.write(f'| {case} | {key} | {r["max"]:.2e} | {r["max_ref"]:.2e} | {r["ratio_max"]:.2f} | {r["ratio_rms"]:.2f} | '
                        f'{r["c"]:g} |\n')
            f.write(f'\nwall time of the module: {time.time() - t0:.0f} s\n')


# ---- engines ----------------------------------------------------------------------------------------------------------------
EFF_CONF = {'output_size': 256, 'attention_heads': 4, 'linear_units': 2048, 'cnn_module_kernel': 15,
            'efficient_conf': {'stride_layer_idx': [3], 'stride': [2], 'group_layer_idx': [0, 1, 2, 3], 'group_size': 3,
                               'stride_kernel': True}}
SQZ_CONF = {'encoder_dim': 256, 'attention_heads': 4, 'feed_forward_expansion_factor': 8, 'cnn_module_kernel': 31}


def model(kind, depth, streaming=True, vocab=512, norm='layer_norm', il='conv2d', reduce=None, recover=None):
    """(state dict, HipEngine keywords, oracle family, oracle keywords, frame rate of the valid-frame mask)"""
    from masr_amd.utils import synthetic
    if kind == 'conformer':
        sd = synthetic.conformer_state_dict(0, vocab, num_blocks=depth, cnn_module_norm=norm, input_layer=il)
        conf = {'num_blocks': depth, 'cnn_module_norm': norm, 'input_layer': il}
        okw = {'streaming': streaming}
        if il != 'conv2d':
            from tests.test_gpu_input_layers import encoder_full_il
            okw = {'encoder_fn': lambda s, x, l, decoding_chunk_size=-1: encoder_full_il(s, x, l, il, streaming, decoding_chunk_size)}
        rate = {'conv2d': 4, 'conv2d6': 6, 'conv2d8': 8}[il]
    elif kind == 'efficient_conformer':
        sd = synthetic.efficient_conformer_state_dict(0, vocab, num_blocks=depth)
        conf = dict(EFF_CONF, num_blocks=depth)
        okw, rate = {'streaming': streaming}, 8
    else:
        sd = synthetic.squeezeformer_state_dict(0, vocab, num_blocks=depth, streaming=streaming)
        conf = dict(SQZ_CONF, num_blocks=depth, reduce_idx=reduce, recover_idx=recover)
        okw, rate = {'reduce_idx': reduce, 'recover_idx': recover, 'causal': streaming}, 4
    return sd, dict(encoder_conf=conf, vocab_size=vocab, streaming=streaming, use_model=kind), kind, okw, rate


@pytest.fixture(scope='module')
def engines():
    """engines of this module by their ``model`` arguments, built on first use and closed at the end"""
    from masr_amd.engine import HipEngine
    cache = {}

    def get(*a, **k):
        key = (a, tuple(sorted(k.items())))
        if key not in cache:
            sd, ekw, fam, okw, rate = model(*a, **k)
            cache[key] = (HipEngine(sd, **ekw), sd, fam, okw, rate)
        return cache[key]
    yield get
    for e in cache.values():
        e[0].close()


def batch(B, T, seed, ragged=True):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, 80, generator=gen) * 3 + 13
    lens = torch.randint(max(T // 3, 20), T + 1, (B,), generator=gen) if ragged else torch.full((B,), T)
    lens[0] = T
    return x * (torch.arange(T)[None, :, None] < lens[:, None, None]), lens


def full_case(case, eng, feats, lens, chunk=-1):
    """encode_full + ctc_probs of one engine on one batch under the rule -> figures of enc and probs"""
    from oracle import f64
    e, sd, fam, okw, rate = eng
    kw = dict(okw)
    if chunk > 0:
        kw['decoding_chunk_size'] = chunk
    r32, r64 = f64.both(fam, sd, feats, lens, **kw)
    assert torch.isfinite(r32['probs']).all()
    enc = e.encode_full(dev(feats), dev(lens, torch.int32), chunk)
    probs = e.ctc_probs(enc)
    mask = budget.valid_mask(r64['enc'].shape, lens, rate)
    assert tuple(enc.shape) == tuple(r64['enc'].shape)
    return [(case, k, held(case, k, r64[k], r32[k], g, mask)) for k, g in (('enc', enc), ('probs', probs))]


# ---- depth ladder x attention modes on the golden batch ---------------------------------------------------------------------
LADDER = [('conformer', d, dict(streaming=s, norm=n)) for d in (1, 2, 12) for s in (True, False) for n in ('layer_norm', 'batch_norm')]
LADDER += [('conformer', d, dict(il=il)) for d in (1, 2) for il in ('conv2d6', 'conv2d8')]
LADDER += [('efficient_conformer', d, {}) for d in (5, 6, 12)]
LADDER += [('squeezeformer', 12, dict(streaming=s, reduce=5, recover=11)) for s in (False, True)]
LADDER += [('squeezeformer', 4, dict(streaming=s, reduce=1, recover=3)) for s in (False, True)]
LADDER += [('squeezeformer', 2, dict(streaming=False)), ('squeezeformer', 1, dict(streaming=True))]      # reduce_idx: null


def _name(kind, depth, opt):
    return f'{kind} depth {depth}' + ''.join(f' {k}={v}' for k, v in sorted(opt.items()))


@pytest.mark.parametrize('kind,depth,opt', LADDER, ids=[_name(*c).replace(' ', '_') for c in LADDER])
def test_depth_ladder_and_attention_modes(engines, kind, depth, opt):
    """golden batch (3 ragged utterances): full attention everywhere; chunk masks 16 and 4 where the build has them"""
    from oracle.make_golden import golden_inputs
    feats, lens = golden_inputs()
    eng = engines(kind, depth, **opt)
    chunks = (-1, 16, 4) if opt.get('streaming', True) else (-1,)
    res = []
    for chunk in chunks:
        res += full_case(f'{_name(kind, depth, opt)} chunk {chunk}', eng, feats, lens, chunk)
    settle(res)


# ---- shapes that select every kernel route (depth 2: routing depends on rows, not on depth) ----------------------------------
SHAPES = [(1, 250), (3, 611), (8, 444), (8, 448), (16, 382), (16, 384), (32, 257), (17, 963), (17, 971), (17, 1439), (33, 995),
          (32, 998)]


@pytest.mark.parametrize('B,T', SHAPES)
def test_kernel_routes_at_depth_2(engines, B, T):
    feats, lens = batch(B, T, 1000 * B + T, ragged=(B, T) != (32, 998))       # 32 x 998 full length: the contract size
    res = full_case(f'conformer depth 2 B={B} T={T}', engines('conformer', 2), feats, lens)
    if (B, T) in ((3, 611), (17, 963)):
        res += full_case(f'conformer depth 2 B={B} T={T} chunk 16', engines('conformer', 2), feats, lens, 16)
        res += full_case(f'conformer nonstreaming depth 2 B={B} T={T}', engines('conformer', 2, streaming=False), feats, lens)
        res += full_case(f'efficient_conformer depth 5 B={B} T={T}', engines('efficient_conformer', 5), feats, lens)
        res += full_case(f'squeezeformer depth 4 B={B} T={T}', engines('squeezeformer', 4, streaming=False, reduce=1, recover=3),
                         feats, lens)
    settle(res)


def test_depth_12_on_a_ragged_batch(engines):
    feats, lens = batch(3, 611, 611)
    res = []
    for kind, opt in (('conformer', {}), ('efficient_conformer', {}), ('squeezeformer', dict(streaming=False, reduce=5, recover=11))):
        res += full_case(f'{kind} depth 12 B=3 T=611', engines(kind, 12, **opt), feats, lens)
    settle(res)


# ---- chunk steps: probabilities and exported caches ---------------------------------------------------------------------------
CHUNKED = [('conformer', 1, {}), ('conformer', 2, {}), ('conformer', 12, {}), ('efficient_conformer', 12, {}),
           ('squeezeformer', 12, dict(streaming=True, reduce=5, recover=11))]


@pytest.mark.parametrize('kind,depth,opt', CHUNKED, ids=[_name(*c).replace(' ', '_') for c in CHUNKED])
def test_chunk_steps_and_exported_caches(engines, kind, depth, opt):
    from oracle import f64
    from oracle.make_golden import golden_inputs
    feats, _ = golden_inputs()
    e, sd, fam, _, _ = engines(kind, depth, **opt)
    (p32, a32, c32), (p64, a64, c64) = f64.both_chunks(fam, sd, feats, WINDOWS)
    sid = e.stream_open(400 if kind == 'conformer' else 0)
    try:
        outs = [e.encode_chunk([sid], dev(feats[:1, cur:cur + n]))[0][0] for cur, n in WINDOWS]
        att, cnn = e.stream_export_cache(sid)
    finally:
        e.stream_close(sid)
    case = f'{_name(kind, depth, opt)} chunks'
    got = torch.cat(outs)
    assert got.shape == p64.shape and att.shape == a64.shape and cnn.shape == c64.shape
    settle([(case, 'probs', held(case, 'probs', p64, p32, got)), (case, 'att_cache', held(case, 'att_cache', a64, a32, att)),
            (case, 'cnn_cache', held(case, 'cnn_cache', c64, c32, cnn))])


def test_260_lock_step_streams(engines):
    """4160 rows per chunk step: the row-block / query-tiled kernels with the separate cache append"""
    from oracle import f64
    e, sd, fam, _, _ = engines('conformer', 2)
    gen = torch.Generator().manual_seed(12)
    feats = torch.randn(2, 131, 80, generator=gen) * 3 + 13
    wins = [(0, 67), (64, 67)]
    ref = [f64.both_chunks(fam, sd, feats[i:i + 1], wins) for i in range(2)]
    n = 260
    x = dev(feats[torch.arange(n) % 2])
    sids = [e.stream_open(40) for _ in range(n)]
    try:
        many = torch.cat([e.encode_chunk(sids, x[:, cur:cur + k].contiguous())[0] for cur, k in wins], dim=1)
    finally:
        for s in sids:
            e.stream_close(s)
    res = []
    for i in range(2):
        (p32, _, _), (p64, _, _) = ref[i]
        for j in (i, n - 2 + i):                                   # first and last stream fed with input i
            res.append(('260 streams', f'probs[{j}]', held('conformer depth 2 260 streams', f'probs[{j}]', p64, p32, many[j])))
    settle(res)


# ---- DeepSpeech2 --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ds2():
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    cache = {}

    def get(gru, bi):
        if (gru, bi) not in cache:
            sd = synthetic.deepspeech2_state_dict(0, 300, bidirectional=bi, use_gru=gru)
            conf = {'num_rnn_layers': 5, 'rnn_size': 1024, 'use_gru': gru}
            cache[gru, bi] = (HipEngine(sd, encoder_conf=conf, streaming=not bi, use_model='deepspeech2'), sd)
        return cache[gru, bi]
    yield get
    for e, _ in cache.values():
        e.close()


@pytest.mark.parametrize('bi', [False, True], ids=['streaming', 'bidirectional'])
@pytest.mark.parametrize('gru', [False, True], ids=['lstm', 'gru'])
def test_deepspeech2(ds2, gru, bi):
    from oracle import f64
    e, sd = ds2(gru, bi)
    name = f'deepspeech2 {"gru" if gru else "lstm"} {"bi" if bi else "uni"}'
    res = []
    for B in (1, 7, 20):
        feats, lens = batch(B, 131, 100 + B)
        r32, r64 = f64.both('deepspeech2', sd, feats, lens)
        enc = e.encode_full(dev(feats), dev(lens, torch.int32))
        probs = e.ctc_probs(enc)
        n = r64['enc'].shape[1]                                    # the oracle trims to the longest sequence, as pad_packed does
        mask = budget.valid_mask((B, n), None, counts=r64['lens'].tolist())
        for k, g in (('enc', enc), ('probs', probs)):
            res.append((name, k, held(f'{name} B={B}', k, r64[k], r32[k], g[:, :n], mask)))
    if not bi:                                                     # chunk steps: probabilities and the exported state
        from oracle.make_golden import golden_inputs
        feats, _ = golden_inputs()
        wins = WINDOWS[:5]
        (p32, h32, c32), (p64, h64, c64) = f64.both_chunks('deepspeech2', sd, feats, wins)
        sid = e.stream_open(0)
        try:
            got = torch.cat([e.encode_chunk([sid], dev(feats[:1, cur:cur + k]))[0][0] for cur, k in wins])
            h, c = e.stream_export_cache(sid)
        finally:
            e.stream_close(sid)
        assert h.shape == h64.shape and c.shape == c64.shape
        res += [(name, k, held(f'{name} chunks', k, t, r, g)) for k, t, r, g in (('probs', p64, p32, got), ('h', h64, h32, h),
                                                                                  ('c', c64, c32, c))]
    settle(res)


# ---- stress checkpoints -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('depth', [1, 2])
@pytest.mark.parametrize('level', [(3, 4, 4), (6, 8, 8)], ids=['3-4-4', '6-8-8'])
def test_stress_checkpoints(level, depth):
    """raised q / k, FFN / GLU and CTC gains (tests/budget.py:stress_state_dict; the CPU module checks that the oracle stays
    finite and decided on them): the same rule -- the reference's own error sets the scale -- plus what needs no tolerance"""
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    from oracle import f64
    from oracle.make_golden import golden_inputs
    feats, lens = golden_inputs()
    sd = budget.stress_state_dict(synthetic.conformer_state_dict(0, 512, num_blocks=depth), *level)
    r = {c: f64.both('conformer', sd, feats, lens, decoding_chunk_size=c) for c in (-1, 16)}
    for r32, r64 in r.values():                                    # finite on the CPU before anything is launched
        assert all(torch.isfinite(x[k]).all() for x in (r32, r64) for k in ('enc', 'logits', 'probs'))
    e = HipEngine(sd, encoder_conf={'num_blocks': depth}, vocab_size=512)
    res = []
    try:
        for chunk, (r32, r64) in r.items():
            case = f'stress {level} depth {depth} chunk {chunk}'
            enc = e.encode_full(dev(feats), dev(lens, torch.int32), chunk)
            probs, idx, mp = e.ctc_probs(enc, want_argmax=True)
            mask = budget.valid_mask(r64['enc'].shape, lens)
            assert torch.isfinite(enc).all() and torch.isfinite(probs).all(), case
            assert (probs.sum(-1) - 1).abs().max().item() < 1e-4, case
            res += [(case, k, held(case, k, r64[k], r32[k], g, mask)) for k, g in (('enc', enc), ('probs', probs))]
            e_ref = np.abs(budget.as64(r32['probs']) - budget.as64(r64['probs']))[mask].max()
            decided = budget.argmax_margin(r64['probs'], e_ref) & mask
            assert 1 - decided[mask].mean() <= 0.02, case
            want = budget.as64(r64['probs']).argmax(-1)
            assert (idx.cpu().numpy().reshape(want.shape)[decided] == want[decided]).all(), case
            idx2, _ = e.ctc_greedy_frames(enc)
            assert (idx2.cpu().numpy().reshape(want.shape)[decided] == want[decided]).all(), case
    finally:
        e.close()
    settle(res)


# ---- single kernels at their edges --------------------------------------------------------------------------------------------
def _act(x, act):
    return torch.relu(x) if act == 1 else x * torch.sigmoid(x) if act == 2 else x


@pytest.mark.parametrize('act', [0, 1, 2], ids=['linear', 'relu', 'swish'])
def test_op_gemm_edges(engines, act):
    """res + alpha * act(a w^T + b) at the row counts around the 16 / 64 / 128-row tiles and at every K of the models;
    reference = the same formula in torch CPU float32.

    K = 4864 (the embed projection, 19 x 256) has its own allowance on the MAX criterion, 8 * sqrt(4864 / 2048) = 12.3: the
    a-priori C assumes that the reference's error grows with K like the kernel's, but the CPU GEMM blocks K and stays at the
    rounding floor of its output (measured reference rms 1.37e-7 at K = 2048, 1.51e-7 at K = 4864: no growth), while a
    sequential accumulation chain grows with sqrt(K).  Measured when this test was written: rms ratio 3.7 ... 4.2 at every M
    (within C = 8, which the rms criterion keeps), max ratio 4.2 ... 8.3 (M = 64, linear: 8.32) -- the same at every M, so a
    property of the summation order and not of a tile edge."""
    e = engines('conformer', 1)[0]
    res = []
    for K in (64, 256, 2048, 4864):
        for M in (1, 15, 16, 17, 63, 64, 65, 127, 129):
            gen = torch.Generator().manual_seed(M * 10007 + K + act)
            N = 256 if K != 256 else 2048
            a = torch.randn(M, K, generator=gen)
            w = torch.randn(N, K, generator=gen) / np.sqrt(K)
            b = torch.randn(N, generator=gen)
            r = torch.randn(M, N, generator=gen)
            y32 = r + 0.5 * _act(F.linear(a, w, b), act)
            y64 = r.double() + 0.5 * _act(F.linear(a.double(), w.double(), b.double()), act)
            got = e.op_gemm(dev(a), dev(w), dev(b), dev(r), act=act, alpha=0.5)
            case = f'op_gemm act {act} M={M} K={K} N={N}'
            res.append((case, 'out', held(case, 'out', y64, y32, got, c_max=budget.C * np.sqrt(K / 2048) if K == 4864 else None)))
    settle(res)


def test_op_gemm_swish_limits(engines):
    """pre-activations of exactly +-100: 1 + exp(100) overflows float32, so the gate must come out as exactly 1 / (sub)zero --
    v * sigmoid(v) = 100 exactly and -100 * 3.7e-44 (a float32 subnormal, or zero where subnormals are flushed); never NaN"""
    e = engines('conformer', 1)[0]
    for M in (1, 16, 17, 129):
        K, N = 64, 256
        a = torch.zeros(M, K)
        a[:, 0] = 100.0 * (1 - 2 * (torch.arange(M) % 2))           # +100, -100, +100, ...
        w = torch.zeros(N, K)
        w[:, 0] = 1.0
        got = e.op_gemm(dev(a), dev(w), dev(torch.zeros(N)), None, act=2, alpha=1.0).cpu()
        assert torch.isfinite(got).all(), M
        assert (got[0::2] == 100.0).all(), (M, got[0::2].min().item(), got[0::2].max().item())
        if M > 1:
            assert (got[1::2] <= 0).all() and (got[1::2] >= -4e-42).all(), (M, got[1::2].min().item())


def test_op_layernorm_edges(engines):
    e = engines('conformer', 1)[0]
    D = 256
    res = []
    for M in (1, 3, 4, 5):
        gen = torch.Generator().manual_seed(M)
        w = torch.randn(D, generator=gen)
        b = torch.randn(D, generator=gen)
        rows = {'mean 1e3 unit variance': torch.randn(M, D, generator=gen) + 1e3,
                'variance 1e-4': torch.randn(M, D, generator=gen) * 1e-2,        # eps-dominated: a wrong eps is a 2x error
                'unit': torch.randn(M, D, generator=gen)}
        for name, x in rows.items():
            y32 = F.layer_norm(x, (D,), w, b, 1e-5)
            y64 = F.layer_norm(x.double(), (D,), w.double(), b.double(), 1e-5)
            got = e.op_layernorm(dev(x), dev(w), dev(b))
            res.append((f'op_layernorm M={M} {name}', 'out', held(f'op_layernorm M={M} {name}', 'out', y64, y32, got)))
        # constant rows: x - mean = 0 exactly (3.0 * 256 / 256), so the output is the bias whatever the scale -- as long as eps
        # sits inside the square root (0 * rsqrt(0 + eps)); rsqrt(0) outside it would give 0 * inf = NaN
        x = torch.full((M, D), 3.0)
        got = e.op_layernorm(dev(x), dev(w), dev(b)).cpu()
        assert torch.equal(got, b.expand(M, D)), (M, (got - b).abs().max().item())
    settle(res)


@pytest.mark.parametrize('V', [512, 4233, 12000])
def test_ctc_head_with_logits_at_80(V):
    """hand-made encoder rows: 80 times the (normalised) head row of one class minus 80 times that of another, so the logits
    reach about +-80 (exp(80) = 5.5e34 is still a float32, the sum over V = 12 000 of such terms would not be without the
    max subtraction); probabilities under the rule, fused greedy head equal to the float64 argmax where that is decided"""
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sd = synthetic.conformer_state_dict(0, V, num_blocks=1)
    W, bias = sd['ctc.ctc_lo.weight'], sd['ctc.ctc_lo.bias']
    gen = torch.Generator().manual_seed(V)
    rows = 67
    j, k = torch.randint(0, V, (rows,), generator=gen), torch.randint(0, V, (rows,), generator=gen)
    unit = W / (W * W).sum(-1, keepdim=True)
    enc = 80.0 * unit[j] - 80.0 * unit[k] + 0.1 * torch.randn(rows, W.shape[1], generator=gen)
    enc[::5] *= 0.25                                                 # some rows with a flatter distribution
    enc = enc.reshape(1, rows, -1).contiguous()
    l32 = F.linear(enc, W, bias)
    l64 = F.linear(enc.double(), W.double(), bias.double())
    assert l64.max() > 70 and l64.min() < -70 and torch.isfinite(l32).all()
    p32, p64 = torch.softmax(l32, -1), torch.softmax(l64, -1)
    e = HipEngine(sd, encoder_conf={'num_blocks': 1}, vocab_size=V)
    try:
        probs, idx, mp = e.ctc_probs(dev(enc), want_argmax=True)
        idx2, mp2 = e.ctc_greedy_frames(dev(enc))
    finally:
        e.close()
    case = f'ctc head V={V} logits +-80'
    assert torch.isfinite(probs).all() and (probs.sum(-1) - 1).abs().max().item() < 1e-4
    res = [(case, 'probs', held(case, 'probs', p64, p32, probs)),
           (case, 'max prob', held(case, 'max prob', p64.max(-1).values, p32.max(-1).values, mp.reshape(1, rows))),
           (case, 'greedy max prob', held(case, 'greedy max prob', p64.max(-1).values, p32.max(-1).values, mp2.reshape(1, rows)))]
    e_ref = (p32.double() - p64).abs().max().item()
    decided = budget.argmax_margin(p64, e_ref)
    assert decided.mean() >= 0.98
    want = p64.argmax(-1).numpy()
    assert (idx.cpu().numpy().reshape(want.shape)[decided] == want[decided]).all()
    assert (idx2.cpu().numpy().reshape(want.shape)[decided] == want[decided]).all()
    settle(res)
