"""GPU: the five relative-position attention kernels of masr_amd/csrc/attention.hip, one launch at a time (masr_op_attention),
against tests/attention_ref.py in float64 under the budget rule of tests/budget.py (C = 8), at the edges of their tiles and masks.

Which kernel a call runs is decided by the process-wide switches, exactly as in a forward pass (launch_attention /
launch_attention_grouped); every case runs under the settings of KERNELS / GROUPED_KERNELS below:

    tiled_fold      attention_kernel<1>            keys 7 = 0, 14 = 1      128 queries x (even | odd) 32-key tiles per workgroup
    tiled_two_term  attention_kernel<0>            keys 7 = 0, 14 = 0
    key_split       attention_fewq_kernel          key 28 raised (and the default when no sequence has more than 32 queries):
                                                   wave w owns key tiles w, w + 8, ...
    grouped_fold    attention_grouped_fold_kernel  key 26 = 1              96 queries per workgroup, key tiles in pairs
    grouped_2wave   attention_grouped_kernel       key 26 = 0              64 queries per workgroup

The test owns the memory around the operands.  K, V and the positional table are NaN wherever the formula does not name a row:
GUARD rows behind the last key row nk - 1 of every sequence, behind positional row pos0 + pos_stride * (nk - 1), the rows
between two positional rows at pos_stride 2, the q rows from nq on, and the columns of the interleaved layouts that belong to
no operand.  The padded key rows klen <= j < nk hold finite values of magnitude 1e3 ("probability zero times a finite
value").  ``out`` is filled with a sentinel; the rows below nq must be written in full, every other row must keep it.  A kernel
that reads one row too far, or weighs a masked row, leaves a NaN or an error far over the budget.

The engine passes pos_stride 1 and 2 only (full rate, and the half rate behind a time reduction / stride layer), so these are the
strides of the chunk-mask cases.  Conditions on the inputs (finite references, the number of fully masked rows, at least two
weighty keys per row of the wide-spread cases) are asserted in ``prepare`` on the CPU before any launch;
tests/test_attention_ref_cpu.py runs ``prepare`` for every case without a GPU."""
import collections
import functools
import math

import pytest
import torch

from tests import attention_ref as ar
from tests import budget

pytestmark = pytest.mark.gpu

GUARD = 4                 # NaN rows behind every operand
TAIL = 64                 # NaN rows at the end of every buffer: a whole tile pair past the last key stays inside the allocation
SENT = -777.25            # what ``out`` holds before a call
BIG = 1.0e3               # magnitude of the padded (masked) key / value rows
DK = 64

KERNELS = {'tiled_fold': {'attention_fewq': 0, 'attention_fold': 1},
           'tiled_two_term': {'attention_fewq': 0, 'attention_fold': 0},
           'key_split': {'attention_fewq': 1, 'attention_fewq_wgs': 1 << 30}}
GROUPED_KERNELS = {'grouped_fold': {'attention_grouped_fold': 1}, 'grouped_2wave': {'attention_grouped_fold': 0}}

Case = collections.namedtuple('Case', 'name seqs heads layout chunk stride spread masked group t_true')
CASES = {}


def S(nq, nk, klen=None, q_abs0=0):
    return dict(nq=nq, nk=nk, klen=nk if klen is None else klen, q_abs0=q_abs0)


def plain(name, seqs, heads=4, layout='dense', chunk=0, stride=1, spread=None, masked=0):
    assert name not in CASES
    CASES[name] = Case(name, seqs, heads, layout, chunk, stride, spread, masked, 1, 0)
    return name


def grouped(name, Tg, t_true, klens=(None,), chunk=0, spread=None, masked=0):
    assert name not in CASES and 3 * Tg - 2 <= t_true <= 3 * Tg
    CASES[name] = Case(name, [S(Tg, Tg, k) for k in klens], 4, 'planar', chunk, 3, spread, masked, 3, t_true)
    return name


# ---- the cases -----------------------------------------------------------------------------------------------------------------
# key counts: the 32-key tile, the tile pair of the tiled kernels (64), the first and second round of the key-split kernel (256);
# 33 queries = one full wave of 32 and a wave with a single live lane
NK_EDGES = [plain(f'nk{nk}', [S(33, nk)]) for nk in (1, 31, 32, 33, 63, 64, 65, 96, 255, 256, 257, 289)]
# query counts: the 32-query wave and the 128-query workgroup; 65 keys = a pair and a lone even tile with one key
NQ_EDGES = [plain(f'nq{nq}', [S(nq, 65)]) for nq in (1, 16, 31, 32, 33, 127, 128, 129)]
# both head counts x the three memory layouts: dense, q | k | v interleaved in rows of 3 d (offline), q in rows of 3 d against a
# k | v cache in rows of 2 d (chunk steps)
LAYOUTS = [plain(f'h{h}_{lay}', [S(33, 97), S(16, 40)], heads=h, layout=lay)
           for h in (4, 8) for lay in ('dense', 'qkv3', 'kv2') if (h, lay) != (4, 'dense')]
# pad masks, three sequences per launch
PADS = [
    # tiled kernels: klen 20 of 64 leaves the odd tile of the pair without a visible key (m_run = -inf in the odd wave, merge with an
    # empty partner); klen 0 = a sequence without any visible key (exact zeros); klen 1
    plain('pad_parity', [S(33, 64, 20), S(33, 96, 0), S(40, 65, 1)], masked=33),
    # key-split kernel: klen 40 of 257 leaves waves 2 .. 7 and the second round of wave 0 without a visible key
    plain('pad_waves', [S(16, 257, 40), S(16, 257, 0), S(16, 64, 31)], masked=16),
    plain('pad_tile', [S(33, 96, 31), S(33, 96, 32), S(33, 96, 33)]),                 # one below, at, one above a tile boundary
    plain('pad_round', [S(20, 289, 255), S(20, 289, 256), S(20, 289, 257)]),          # ... and the 8-tile round of the key split
    plain('pad_h8_qkv3', [S(33, 64, 20), S(33, 96, 0), S(40, 65, 33)], heads=8, layout='qkv3', masked=33),
]
# chunk masks (chunk_size 16).  At pos_stride 1 the limit of query i is 16 (i // 16 + 1): the two halves of a 32-lane group differ,
# limits 16 and 48 end inside a tile, 32 and 64 at its edge.  At pos_stride 2 it is 8 (i // 8 + 1): four limits per 32 lanes.
CHUNKS = [
    plain('chunk_s1', [S(70, 70)], chunk=16, stride=1),
    plain('chunk_s2', [S(70, 70)], chunk=16, stride=2),
    plain('chunk_s1_pad', [S(70, 70, 41), S(33, 40, 40), S(16, 16)], chunk=16, stride=1),
    plain('chunk_q16_s1', [S(20, 60, q_abs0=16)], chunk=16, stride=1),                # queries 16 .. 35 against 60 keys
    plain('chunk_q16_s2', [S(20, 60, q_abs0=16)], chunk=16, stride=2),
    # queries 1008 .. 1047 see 1024 (a tile edge), 1040 and all 1048 keys: the smallest key count at which q_abs0 = 1008 masks at all
    plain('chunk_q1008_s1', [S(40, 1048, q_abs0=1008)], chunk=16, stride=1),
    plain('chunk_q504_s2', [S(40, 530, q_abs0=504)], chunk=16, stride=2),             # the same frames at half rate
]
# score spread: the float64 scores of a row span about +-40; the row maximum sits in the first key tile, in the last, or rises
# tile by tile.  300 keys = 10 tiles (12 keys in the last): five pairs of the tiled kernels, two rounds of the key split.
SPREADS = [plain(f'spread_{s}', [S(40, 300)], spread=s) for s in ('first', 'last', 'rising')]

# grouped kernels: grouped lengths around the 32-key tile and the 96-query workgroup (64 for the two-wave kernel) x the three true
# lengths that pad to them (3 Tg - 1, 3 Tg - 2: zero rows in q / k / v and zero positional rows in the last grouped position)
G_EDGES = [grouped(f'g{Tg}_t{3 * Tg - cut}', Tg, 3 * Tg - cut) for Tg in (1, 32, 33, 95, 96, 97) for cut in (0, 1, 2)]
G_MASKS = [
    grouped('g_pad', 97, 290, klens=(0, 33, 64), masked=97),            # no visible key | one above a tile | a whole pair
    grouped('g_pad_odd', 97, 289, klens=(1, 32, 65)),
    grouped('g_chunk', 70, 209, chunk=16),                              # grouped query i sees keys 3 j < 16 ((3 i) // 16 + 1)
    grouped('g_chunk_pad', 70, 210, klens=(70, 30), chunk=16),
]
G_SPREADS = [grouped(f'g_spread_{s}', 120, 360, spread=s) for s in ('first', 'last', 'rising')]     # four tiles, two workgroups
# enough workgroups (2 x 4 heads x 12 sequences >= key 28's 48) for the default switches to pick the tiled kernel
DEFAULT_TILED = plain('default_tiled', [S(130, 70)] * 12)

PLAIN_CASES = NK_EDGES + NQ_EDGES + LAYOUTS + PADS + CHUNKS + SPREADS
GROUPED_CASES = G_EDGES + G_MASKS + G_SPREADS


# ---- operands ------------------------------------------------------------------------------------------------------------------
def spread_profile(kind, nk, gen):
    """the target score t_j of key j (before the per-query modulation): about +-40, the largest three within 1 of each other"""
    ntile = -(-nk // 32)
    tile = torch.arange(nk) // 32
    if kind == 'rising':
        return -40.0 + 80.0 * tile / max(1, ntile - 1) - 1.5 * torch.rand(nk, generator=gen)
    t = -40.0 + 70.0 * torch.rand(nk, generator=gen)
    top = (1, 9, 30) if kind == 'first' else (nk - 1, nk - 5, nk - 12)
    for j, val in zip(top, (40.0, 39.5, 39.2)):
        t[j] = val
    return t


def operands(case, s, gen):
    """float32 q [nq, H, dk], k, v, p [nk, H, dk] of one sequence in the kernel's own head layout (grouped: dk = 192)"""
    H, dk = case.heads, DK * case.group
    r = lambda *shape: torch.randn(*shape, generator=gen)
    q, k, v, p = r(s['nq'], H, dk), r(s['nk'], H, dk), r(s['nk'], H, dk), r(s['nk'], H, dk)
    if case.spread:
        # (q + u) . k_j / sqrt(dk) = t_j (1 + delta_i) + noise with u of norm 2 sqrt(dk) along which the keys are laid out:
        # delta_i = q_i . u / |u|^2 ~ N(0, 1 / (4 dk)) moves the whole row of a query, the order of the keys stays
        u = 2.0 * torch.sign(r(H, dk))
        t = spread_profile(case.spread, s['nk'], gen)
        k = 0.05 * k + t[:, None, None] * math.sqrt(dk) * u[None] / (u * u).sum(-1, keepdim=True)[None]
        p = 0.1 * p
        return q, k, v, p, u
    return q, k, v, p, None


@functools.lru_cache(maxsize=None)
def prepare(name):
    """host buffers, descriptors and the two references of a case, built once and shared by the kernels that run it"""
    case = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 17)
    H, g = case.heads, case.group
    dk, d = DK * g, case.heads * DK                       # d: floats of a frame (grouped: a grouped row is 3 frames)
    bias_u, bias_v = torch.randn(H, dk, generator=gen), torch.randn(H, dk, generator=gen)
    ops = []
    for s in case.seqs:
        q, k, v, p, u = operands(case, s, gen)
        if u is not None:
            bias_u = u
        if g == 3:          # the operation zero-pads frames t_true .. 3 Tg - 1: q, k, v are zero there and P counts as zero
            for t in (q, k, v, p):
                t.view(-1, d)[case.t_true:] = 0.0
        k[s['klen']:] = BIG * torch.sign(torch.randn(k[s['klen']:].shape, generator=gen))
        v[s['klen']:] = BIG * torch.sign(torch.randn(v[s['klen']:].shape, generator=gen))
        ops.append((q, k, v, p))

    # ---- references: float64 truth and the same function in float32 on the CPU ---------------------------------------------
    y64, y32, masked = [], [], 0
    for s, (q, k, v, p) in zip(case.seqs, ops):
        for dt, dst in ((torch.float64, y64), (torch.float32, y32)):
            a = [t.to(dt) for t in (q, k, v, p, bias_u, bias_v)]
            if g == 3:
                T = case.t_true
                y = ar.grouped_attention(*(t.reshape(-1, d)[:T] for t in a[:4]), a[4], a[5], H, s['klen'], case.chunk, 3)
            else:
                y = ar.attention(*a, s['klen'], case.chunk, case.stride, s['q_abs0'])
            dst.append(y)
        vis = ar.visible(s['nq'], s['nk'], s['klen'], case.chunk, case.stride, 0 if g == 3 else s['q_abs0'])
        masked += int((~vis.any(1)).sum())
        assert torch.isfinite(y64[-1]).all() and torch.isfinite(y32[-1]).all(), name
        assert (y64[-1][~vis.any(1)] == 0).all(), name
        if case.spread:
            a = [t.double() for t in (q, k, p, bias_u, bias_v)]
            sc = (torch.einsum('ihd,jhd->hij', a[0] + a[3], a[1]) + torch.einsum('ihd,jhd->hij', a[0] + a[4], a[2])) / math.sqrt(dk)
            assert sc.amax(-1).median() > 35 and sc.amin(-1).median() < -35, (name, sc.amax(-1).median(), sc.amin(-1).median())
            prob = torch.softmax(sc, -1)
            assert ((prob > 1e-3).sum(-1) >= 2).all(), (name, 'a one-hot row')
            tile = prob.argmax(-1) // 32
            want = 0 if case.spread == 'first' else (s['nk'] - 1) // 32
            assert (tile == want).all(), (name, 'row maximum outside the intended tile')
    assert masked == case.masked, (name, masked, case.masked)

    # ---- device layouts: everything the formula does not name is NaN ---------------------------------------------------------
    nan = lambda rows, cols: torch.full((rows + TAIL, cols), float('nan'))
    fr = g                                                # frames per (grouped) row
    lay, descs = case.layout, []
    if lay in ('dense', 'planar'):
        qs, ks, cols = d * fr, d * fr, {'q': 0, 'k': 0, 'v': 0}
        rows_q = sum(s['nq'] + GUARD for s in case.seqs)
        rows_k = sum(s['nk'] + GUARD for s in case.seqs)
        bufs = {'q': nan(rows_q, qs), 'k': nan(rows_k, ks), 'v': nan(rows_k, ks)}
    elif lay == 'qkv3':
        qs, ks, cols = 3 * d, 3 * d, {'q': 0, 'k': d, 'v': 2 * d}
        rows = sum(max(s['nq'], s['nk']) + GUARD for s in case.seqs)
        bufs = {'q': nan(rows, qs)}
        bufs['k'] = bufs['v'] = bufs['q']
    else:
        assert lay == 'kv2'
        qs, ks, cols = 3 * d, 2 * d, {'q': 0, 'k': 0, 'v': d}
        bufs = {'q': nan(sum(s['nq'] + GUARD for s in case.seqs), qs), 'k': nan(sum(s['nk'] + GUARD for s in case.seqs), ks)}
        bufs['v'] = bufs['k']
    w = d * fr                                            # floats of an output row
    out_rows = sum(s['nq'] + GUARD for s in case.seqs)
    row = {'q': 0, 'k': 0, 'v': 0, 'out': 0}
    n_pos = 0
    for s, (q, k, v, p) in zip(case.seqs, ops):
        e = {}
        for key, t, n in (('q', q, s['nq']), ('k', k, s['nk']), ('v', v, s['nk'])):
            r0 = row['q'] if lay == 'qkv3' else row['k' if (lay == 'kv2' and key == 'v') else key]
            bufs[key][r0:r0 + n, cols[key]:cols[key] + w] = t.reshape(n, w)
            e[key + '_off'] = r0 * bufs[key].shape[1] + cols[key]
        e['out_off'] = row['out'] * w
        if lay == 'qkv3':
            row['q'] += max(s['nq'], s['nk']) + GUARD
        else:
            row['q'] += s['nq'] + GUARD
            row['k'] += s['nk'] + GUARD
            row['v'] = row['k']
        e['out_row'] = row['out']
        row['out'] += s['nq'] + GUARD
        # positional rows: key 0 sits at the position of the first key of the window the queries end, at the layer's rate
        pos0 = max(n_pos, case.stride * max(0, s['q_abs0'] + s['nq'] - s['nk'])) if g == 1 else n_pos
        last = pos0 + (case.stride * (s['nk'] - 1) if g == 1 else case.t_true - 1)
        n_pos = last + 1 + GUARD
        e.update(nq=s['nq'], nk=s['nk'], klen=s['klen'], pos0=pos0, q_abs0=s['q_abs0'])
        descs.append(e)
    ptab = nan(n_pos + TAIL * (case.stride - 1), d)
    for e, (q, k, v, p) in zip(descs, ops):
        if g == 1:
            ptab[e['pos0']:e['pos0'] + case.stride * (e['nk'] - 1) + 1:case.stride] = p.reshape(e['nk'], d)
        else:
            ptab[e['pos0']:e['pos0'] + case.t_true] = p.reshape(-1, d)[:case.t_true]
    return dict(case=case, bufs=bufs, ptab=ptab, u=bias_u.reshape(-1).contiguous(), v=bias_v.reshape(-1).contiguous(), descs=descs,
                q_stride=qs, kv_stride=ks, w=w, out_rows=out_rows, y64=torch.cat(y64), y32=torch.cat(y32),
                zero_rows=torch.cat([~ar.visible(s['nq'], s['nk'], s['klen'], case.chunk, case.stride,
                                                 0 if g == 3 else s['q_abs0']).any(1) for s in case.seqs]))


# ---- one case under one kernel ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def eng():
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    e = HipEngine(synthetic.conformer_state_dict(0, 512, num_blocks=1),
                  encoder_conf={'num_blocks': 1, 'cnn_module_norm': 'layer_norm', 'input_layer': 'conv2d'}, vocab_size=512,
                  streaming=True, use_model='conformer')
    yield e
    e.close()


def launch(eng, prep, keys, times=2):
    """``times`` launches of a case under the switches ``keys``, each into a fresh sentinel-filled ``out``; returns them on the host"""
    from masr_amd._lib import debug_keys
    case = prep['case']
    dev = {}
    for key, t in prep['bufs'].items():                   # (the interleaved layouts share one buffer: upload it once)
        dev[key] = next((dev[o] for o in dev if prep['bufs'][o] is t), None)
        if dev[key] is None:
            dev[key] = t.cuda()
    ptab, u, v = prep['ptab'].cuda(), prep['u'].cuda(), prep['v'].cuda()
    outs = []
    with debug_keys(eng, keys):
        for _ in range(times):
            out = torch.full((prep['out_rows'], prep['w']), SENT, device='cuda')
            eng.op_attention(dev['q'], dev['k'], dev['v'], out, ptab, u, v, prep['descs'], case.heads, prep['q_stride'],
                             prep['kv_stride'], chunk_size=case.chunk, pos_stride=case.stride, group=case.group, t_true=case.t_true)
            outs.append(out.cpu())
    return outs


def settle(name, prep, outs):
    out = outs[0]
    live = torch.zeros(prep['out_rows'], dtype=torch.bool)
    for e in prep['descs']:
        live[e['out_row']:e['out_row'] + e['nq']] = True
    assert (out[~live] == SENT).all(), f'{name}: rows at or beyond nq were written'
    y = out[live]
    assert not (y == SENT).any(), f'{name}: a row below nq was not written in full'
    budget.check(name, prep['y64'], prep['y32'], y)        # (a NaN -- a row outside the operands read, or weighed -- is over budget)
    assert (y[prep['zero_rows']] == 0.0).all(), f'{name}: a query without a visible key must give exact zeros'
    for other in outs[1:]:
        assert torch.equal(out, other), f'{name}: a second identical call differs'


@pytest.mark.parametrize('kernel', list(KERNELS))
@pytest.mark.parametrize('name', PLAIN_CASES)
def test_plain_kernels(eng, name, kernel):
    prep = prepare(name)
    settle(f'{name} {kernel}', prep, launch(eng, prep, KERNELS[kernel]))


@pytest.mark.parametrize('kernel', list(GROUPED_KERNELS))
@pytest.mark.parametrize('name', GROUPED_CASES)
def test_grouped_kernels(eng, name, kernel):
    prep = prepare(name)
    settle(f'{name} {kernel}', prep, launch(eng, prep, GROUPED_KERNELS[kernel]))


def test_default_switches(eng):
    """what production launches: the key-split kernel when no sequence has more than 32 queries (or the launch is small), the
    folded tiled kernel otherwise, the folded grouped kernel -- bit-identical to the same case under the explicit switches; and
    every call is one attention launch of the profile (masr_profile_select kind 4)"""
    eng.profile_select(4)
    eng.profile_read()
    n = 0
    for name, same_as in (('nq16', KERNELS['key_split']), ('nk289', KERNELS['key_split']), (DEFAULT_TILED, KERNELS['tiled_fold']),
                          ('g97_t290', GROUPED_KERNELS['grouped_fold'])):
        prep = prepare(name)
        got = launch(eng, prep, {}, times=1)[0]
        settle(f'{name} default', prep, [got])
        assert torch.equal(got, launch(eng, prep, same_as, times=1)[0]), name
        n += 2
    launches = eng.profile_read()[1]
    eng.profile_select(0)
    assert launches == n, (launches, n)
