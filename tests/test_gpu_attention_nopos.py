"""GPU: the plain attention kernels of masr_amd/csrc/attention.hip -- attention_kernel<0, 0> and attention_fewq_kernel<0>, the
instantiations with the positional term compiled out (pos_enc_layer_type abs_pos / no_pos) -- one launch at a time through
``HipEngine.op_attention(..., positional=False)`` (masr_op_attention_plain -> launch_attention, the launcher the encoder calls),
against tests/attention_plain_ref.py in float64 under the budget rule of tests/budget.py (C = 8): the tolerance rule, the guards
and the edges of tests/test_gpu_attention_op.py.

    tiled       attention_kernel<0, 0>       key 7 = 0                  128 queries x (even | odd) 32-key tiles per workgroup
    key_split   attention_fewq_kernel<0>     key 28 raised (and the default when no sequence has more than 32 queries)

K and V are NaN wherever the formula does not name a row (GUARD rows behind the last key row of every sequence, the q rows from nq
on, the columns of the interleaved layouts that belong to no operand); the padded key rows klen <= j < nk hold finite values of
magnitude 1e3.  ``out`` is filled with a sentinel: the rows below nq must be written in full, every other row must keep it.  A
query without a visible key must give exact zeros, and a second identical call the same bits."""
import collections
import functools

import pytest
import torch

from tests import attention_plain_ref as pr
from tests import attention_ref as ar
from tests import budget

pytestmark = pytest.mark.gpu

GUARD, TAIL, SENT, BIG, DK = 4, 64, -777.25, 1.0e3, 64
KERNELS = {'tiled': {'attention_fewq': 0}, 'key_split': {'attention_fewq': 1, 'attention_fewq_wgs': 1 << 30}}

Case = collections.namedtuple('Case', 'name seqs heads layout chunk stride masked')
CASES = {}


def S(nq, nk, klen=None, q_abs0=0):
    return dict(nq=nq, nk=nk, klen=nk if klen is None else klen, q_abs0=q_abs0)


def case(name, seqs, heads=4, layout='dense', chunk=0, stride=1, masked=0):
    assert name not in CASES
    CASES[name] = Case(name, seqs, heads, layout, chunk, stride, masked)
    return name


EDGES = (1, 15, 16, 17, 100)
# query and key counts around the 16-frame chunk, the 32-key tile and beyond a tile pair (100 keys: two pairs, the last tile of 4)
NQ_NK = [case(f'nq{nq}_nk{nk}', [S(nq, nk)]) for nq in EDGES for nk in EDGES]
# klen shorter than nk (three sequences per launch); klen 0 = a sequence whose every row is fully masked; klen 20 of 64 leaves the
# odd tile of the pair (tiled kernel) and waves 1 .. 7 (key split) without a visible key
PADS = [case('pad', [S(17, 64, 20), S(17, 100, 0), S(40, 65, 1)], masked=17),
        case('pad_tile_edge', [S(33, 96, 31), S(33, 96, 32), S(33, 96, 33)]),
        case('pad_h8_qkv3', [S(33, 64, 20), S(33, 96, 0), S(40, 65, 33)], heads=8, layout='qkv3', masked=33)]
# the decoding_chunk_size mask (chunk_size 16): limits inside and at the edge of a tile, with and without a pad mask on top
CHUNKS = [case('chunk16', [S(70, 70)], chunk=16),
          case('chunk16_pad', [S(70, 70, 41), S(33, 40, 40), S(16, 16)], chunk=16),
          case('chunk16_s2', [S(70, 70)], chunk=16, stride=2),
          case('chunk16_q16', [S(20, 60, q_abs0=16)], chunk=16)]
# a streaming descriptor with cached keys: 16 new queries at offset q_abs0 against a k | v cache in rows of 2 d that already holds
# q_abs0 (or the last 16) keys, q in rows of 3 d; two streams of different history in one launch
STREAMS = [case(f'stream_h{h}', [S(16, 48, q_abs0=32), S(16, 16), S(16, 32, q_abs0=48)], heads=h, layout='kv2') for h in (4, 8)]
STREAMS.append(case('stream_long', [S(16, 272, q_abs0=256)], layout='kv2'))               # 9 key tiles: the key split's second round
HEADS8 = [case('h8_dense', [S(33, 97), S(16, 40)], heads=8), case('h8_kv2', [S(17, 100)], heads=8, layout='kv2')]
# enough workgroups (2 x 4 heads x 12 sequences >= key 28's 48) for the default switches to pick the tiled kernel
DEFAULT_TILED = case('default_tiled', [S(130, 70)] * 12)
ALL = NQ_NK + PADS + CHUNKS + STREAMS + HEADS8


@functools.lru_cache(maxsize=None)
def prepare(name):
    """host buffers, descriptors and the two references of a case, built once and shared by the kernels that run it"""
    c = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 29)
    H, d = c.heads, c.heads * DK
    ops, y64, y32, zero, masked = [], [], [], [], 0
    for s in c.seqs:
        q, k, v = (torch.randn(n, H, DK, generator=gen) for n in (s['nq'], s['nk'], s['nk']))
        k[s['klen']:] = BIG * torch.sign(torch.randn(k[s['klen']:].shape, generator=gen))
        v[s['klen']:] = BIG * torch.sign(torch.randn(v[s['klen']:].shape, generator=gen))
        ops.append((q, k, v))
        for dt, dst in ((torch.float64, y64), (torch.float32, y32)):
            dst.append(pr.attention(q.to(dt), k.to(dt), v.to(dt), s['klen'], c.chunk, c.stride, s['q_abs0']))
        vis = ar.visible(s['nq'], s['nk'], s['klen'], c.chunk, c.stride, s['q_abs0'])
        zero.append(~vis.any(1))
        masked += int(zero[-1].sum())
        assert torch.isfinite(y64[-1]).all() and torch.isfinite(y32[-1]).all() and (y64[-1][zero[-1]] == 0).all(), name
    assert masked == c.masked, (name, masked, c.masked)

    nan = lambda rows, cols: torch.full((rows + TAIL, cols), float('nan'))
    lay = c.layout
    if lay == 'dense':
        qs, ks, cols = d, d, {'q': 0, 'k': 0, 'v': 0}
        bufs = {'q': nan(sum(s['nq'] + GUARD for s in c.seqs), qs), 'k': nan(sum(s['nk'] + GUARD for s in c.seqs), ks)}
        bufs['v'] = nan(bufs['k'].shape[0] - TAIL, ks)
    elif lay == 'qkv3':
        qs, ks, cols = 3 * d, 3 * d, {'q': 0, 'k': d, 'v': 2 * d}
        bufs = {'q': nan(sum(max(s['nq'], s['nk']) + GUARD for s in c.seqs), qs)}
        bufs['k'] = bufs['v'] = bufs['q']
    else:
        assert lay == 'kv2'
        qs, ks, cols = 3 * d, 2 * d, {'q': 0, 'k': 0, 'v': d}
        bufs = {'q': nan(sum(s['nq'] + GUARD for s in c.seqs), qs), 'k': nan(sum(s['nk'] + GUARD for s in c.seqs), ks)}
        bufs['v'] = bufs['k']
    row = {'q': 0, 'k': 0, 'out': 0}
    descs = []
    for s, (q, k, v) in zip(c.seqs, ops):
        e = {}
        for key, t, n in (('q', q, s['nq']), ('k', k, s['nk']), ('v', v, s['nk'])):
            r0 = row['q'] if (lay == 'qkv3' or key == 'q') else row['k']
            bufs[key][r0:r0 + n, cols[key]:cols[key] + d] = t.reshape(n, d)
            e[key + '_off'] = r0 * bufs[key].shape[1] + cols[key]
        e.update(out_off=row['out'] * d, out_row=row['out'], nq=s['nq'], nk=s['nk'], klen=s['klen'], pos0=0, q_abs0=s['q_abs0'])
        row['q'] += (max(s['nq'], s['nk']) if lay == 'qkv3' else s['nq']) + GUARD
        row['k'] += s['nk'] + GUARD
        row['out'] += s['nq'] + GUARD
        descs.append(e)
    return dict(case=c, bufs=bufs, descs=descs, q_stride=qs, kv_stride=ks, w=d, out_rows=row['out'], y64=torch.cat(y64),
                y32=torch.cat(y32), zero_rows=torch.cat(zero))


@pytest.fixture(scope='module')
def eng():
    """an abs_pos engine: it owns no positional tables at all"""
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    e = HipEngine(synthetic.conformer_state_dict(0, 50, num_blocks=1, pos_enc_layer_type='abs_pos'),
                  encoder_conf={'num_blocks': 1, 'pos_enc_layer_type': 'abs_pos'}, vocab_size=50, streaming=True, use_model='conformer')
    yield e
    e.close()


def launch(eng, prep, keys, times=2):
    from masr_amd._lib import debug_keys
    c = prep['case']
    dev = {}
    for key, t in prep['bufs'].items():                   # (the interleaved layouts share one buffer: upload it once)
        dev[key] = next((dev[o] for o in dev if prep['bufs'][o] is t), None)
        if dev[key] is None:
            dev[key] = t.cuda()
    outs = []
    with debug_keys(eng, keys):
        for _ in range(times):
            out = torch.full((prep['out_rows'], prep['w']), SENT, device='cuda')
            eng.op_attention(dev['q'], dev['k'], dev['v'], out, None, None, None, prep['descs'], c.heads, prep['q_stride'],
                             prep['kv_stride'], chunk_size=c.chunk, pos_stride=c.stride, positional=False)
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


def test_cases_cover_the_named_edges():
    """(no launch) the conditions on the inputs: every case builds, with finite references and the stated number of masked rows"""
    for name in ALL + [DEFAULT_TILED]:
        prepare(name)
    assert {(s['nq'], s['nk']) for n in NQ_NK for s in CASES[n].seqs} == {(a, b) for a in EDGES for b in EDGES}
    assert any(s['klen'] < s['nk'] for n in PADS for s in CASES[n].seqs) and any(CASES[n].masked for n in PADS)
    assert {CASES[n].heads for n in ALL} == {4, 8}


@pytest.mark.parametrize('kernel', list(KERNELS))
@pytest.mark.parametrize('name', ALL)
def test_plain_kernels(eng, name, kernel):
    prep = prepare(name)
    settle(f'{name} {kernel}', prep, launch(eng, prep, KERNELS[kernel]))


def test_default_switches_and_the_fold_switch(eng):
    """what production launches: the key-split kernel when no sequence has more than 32 queries (or the launch is small), the tiled
    kernel otherwise -- bit-identical to the same case under the explicit switches; key 14 (the fold of the positional term) has
    nothing to act on; every call is one attention launch of the profile (masr_profile_select kind 4)"""
    eng.profile_select(4)
    eng.profile_read()
    n = 0
    for name, same_as in (('nq16_nk100', KERNELS['key_split']), ('stream_h4', KERNELS['key_split']), (DEFAULT_TILED, KERNELS['tiled'])):
        prep = prepare(name)
        got = launch(eng, prep, {}, times=1)[0]
        settle(f'{name} default', prep, [got])
        assert torch.equal(got, launch(eng, prep, same_as, times=1)[0]), name
        assert torch.equal(got, launch(eng, prep, dict(same_as, attention_fold=0), times=1)[0]), name
        n += 3
    launches = eng.profile_read()[1]
    eng.profile_select(0)
    assert launches == n, (launches, n)


def test_refusals_keep_the_entry_points_name(eng):
    from masr_amd._lib import MasrError
    prep = prepare('nq16_nk16')
    q = prep['bufs']['q'].cuda()
    out = torch.full((prep['out_rows'], prep['w']), SENT, device='cuda')
    with pytest.raises(MasrError, match='masr_op_attention.*heads'):
        eng.op_attention(q, q, q, out, None, None, None, prep['descs'], 5, 256, 256, positional=False)
    bad = [dict(prep['descs'][0], klen=17)]
    with pytest.raises(MasrError, match='masr_op_attention.*klen'):
        eng.op_attention(q, q, q, out, None, None, None, bad, 4, 256, 256, positional=False)
    assert (out == SENT).all()
