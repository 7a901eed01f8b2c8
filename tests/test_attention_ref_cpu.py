"""CPU: tests/attention_ref.py (the float64 truth of tests/test_gpu_attention_op.py) against the attention of the oracles, in
float64 on small cases -- the masks are built the way oracle/conformer.py and oracle/efficient_conformer.py build them (pad mask
& subsequent-chunk mask at the frame rate, rows and columns ::stride after a stride layer), never with the helper's own mask.
Also the argument refusals of masr_op_attention, all of which come before the engine is touched."""
import ctypes as C

import pytest
import torch

from oracle import conformer as oc
from oracle import efficient_conformer as oe
from tests import attention_ref as ar

H, DK, D = 4, 64, 256
P = 'a'


def weights(seed, grouped=False):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sd = {f'{P}.linear_{n}.weight': r(D, D) / 16 for n in 'qkv'}
    sd.update({f'{P}.linear_{n}.bias': r(D) / 4 for n in 'qkv'})
    sd[f'{P}.linear_pos.weight'] = r(D, D) / 16
    sd[f'{P}.pos_bias_u'] = r(H, 3 * DK if grouped else DK)
    sd[f'{P}.pos_bias_v'] = r(H, 3 * DK if grouped else DK)
    sd[f'{P}.linear_out.weight'] = torch.eye(D, dtype=torch.float64)          # the context itself comes out
    sd[f'{P}.linear_out.bias'] = torch.zeros(D, dtype=torch.float64)
    return sd, r


def projections(sd, x, pos):
    lin = lambda n, t, b=True: torch.nn.functional.linear(t, sd[f'{P}.linear_{n}.weight'], sd[f'{P}.linear_{n}.bias'] if b else None)
    return lin('q', x), lin('k', x), lin('v', x), lin('pos', pos, False)


def frame_mask(T, length, chunk):
    idx = torch.arange(T)
    pad = idx < length
    ch = idx[None, :] < ((idx[:, None] // chunk + 1) * chunk) if chunk > 0 else torch.ones(T, T, dtype=torch.bool)
    return pad[None, :] & ch                                                 # [T, T], as encoder_full builds att_mask


@pytest.mark.parametrize('T,length,chunk,stride', [(23, 23, 0, 1), (23, 19, 4, 1), (23, 19, 5, 2), (23, 0, 0, 1), (37, 30, 16, 2)])
def test_plain_form_matches_conformer_oracle(T, length, chunk, stride):
    sd, r = weights(1)
    x, pos = r(1, T, D), r(1, T, D)
    mask = frame_mask(T, length, chunk)[::stride, ::stride]
    xs, ps = x[:, ::stride], pos[:, ::stride]
    want, _ = oc._attention(sd, P, xs, ps, mask[None], H)
    q, k, v, p = (t[0].view(-1, H, DK) for t in projections(sd, x, pos))
    n = xs.shape[1]
    got = ar.attention(q[::stride], k[::stride], v[::stride], p[::stride], sd[f'{P}.pos_bias_u'], sd[f'{P}.pos_bias_v'],
                       klen=-(-length // stride), chunk_size=chunk, pos_stride=stride)
    assert got.shape == (n, D) and got.dtype == torch.float64
    assert torch.equal(ar.visible(n, n, -(-length // stride), chunk, stride), mask)
    assert (got - want[0]).abs().max().item() < 1e-12
    if length == 0:
        assert got.abs().max().item() == 0.0


def test_query_offset_matches_conformer_oracle():
    """queries 16 .. 22 of a 23-frame sequence against all its keys: q_abs0 = 16 (a chunk step behind a key cache)"""
    T, q0, chunk = 23, 16, 4
    sd, r = weights(2)
    x, pos = r(1, T, D), r(1, T, D)
    want, _ = oc._attention(sd, P, x, pos, frame_mask(T, T, chunk)[None], H)
    q, k, v, p = (t[0].view(-1, H, DK) for t in projections(sd, x, pos))
    got = ar.attention(q[q0:], k, v, p, sd[f'{P}.pos_bias_u'], sd[f'{P}.pos_bias_v'], klen=T, chunk_size=chunk, q_abs0=q0)
    assert (got - want[0, q0:]).abs().max().item() < 1e-12
    wrong = ar.attention(q[q0:], k, v, p, sd[f'{P}.pos_bias_u'], sd[f'{P}.pos_bias_v'], klen=T, chunk_size=chunk, q_abs0=0)
    assert (wrong - want[0, q0:]).abs().max().item() > 1e-3               # the offset matters in this case


@pytest.mark.parametrize('T,length,chunk', [(21, 21, 0), (20, 17, 0), (19, 19, 4), (20, 16, 5), (20, 0, 0)])
def test_grouped_form_matches_efficient_conformer_oracle(T, length, chunk):
    sd, r = weights(3, grouped=True)
    x, pos = r(1, T, D), r(1, T, D)
    pad = torch.arange(T) < length
    key_mask = frame_mask(T, length, chunk)[None] if chunk > 0 else pad[None]
    want = oe._grouped_attention(sd, P, x, pos, key_mask, H, 3)
    q, k, v, p = (t[0] for t in projections(sd, x, pos))
    got = ar.grouped_attention(q, k, v, p, sd[f'{P}.pos_bias_u'], sd[f'{P}.pos_bias_v'], H, klen=-(-length // 3), chunk_size=chunk)
    Tg = -(-T // 3)
    assert got.shape == (Tg, 3 * D)
    assert (got.reshape(-1, D)[:T] - want[0]).abs().max().item() < 1e-12
    if length == 0:
        assert got.abs().max().item() == 0.0


def test_float32_evaluation_is_close_to_float64():
    sd, r = weights(4)
    x, pos = r(1, 40, D), r(1, 40, D)
    q, k, v, p = (t[0].view(-1, H, DK) for t in projections(sd, x, pos))
    u, vb = sd[f'{P}.pos_bias_u'], sd[f'{P}.pos_bias_v']
    y64 = ar.attention(q, k, v, p, u, vb, klen=33, chunk_size=16)
    y32 = ar.attention(*(t.float() for t in (q, k, v, p, u, vb)), klen=33, chunk_size=16)
    assert y32.dtype == torch.float32
    assert (y32.double() - y64).abs().max().item() < 1e-5


def test_cases_of_the_gpu_module_hold_their_conditions():
    """every case of tests/test_gpu_attention_op.py builds on the CPU: finite float64 and float32 references, the stated number
    of fully masked query rows, weighty wide-spread rows (the asserts of its ``prepare``); every row has a reference"""
    from tests import test_gpu_attention_op as g
    assert set(g.PLAIN_CASES + g.GROUPED_CASES + [g.DEFAULT_TILED]) == set(g.CASES)
    for name, case in g.CASES.items():
        prep = g.prepare(name)
        assert prep['y64'].shape == prep['y32'].shape == (sum(s['nq'] for s in case.seqs), prep['w']), name
        assert int(prep['zero_rows'].sum()) == case.masked, name
        for buf in list(prep['bufs'].values()) + [prep['ptab']]:
            assert torch.isnan(buf[-g.GUARD:]).all(), name                     # the guard rows are there


# ---- masr_op_attention refuses bad arguments without a device ---------------------------------------------------------------
GOOD = dict(n_pos=64, nseq=1, nq=[8], nk=[8], klen=[8], pos0=[0], q_abs0=[0], off=[0], heads=4, q_stride=256, kv_stride=256,
            chunk_size=0, pos_stride=1, group=1, t_true=0, ptr=4096)


def call(**change):
    from masr_amd import _lib
    a = dict(GOOD, **change)
    n = max(1, len(a['nq']))
    i32 = lambda v: (C.c_int32 * n)(*v)
    i64 = lambda v: (C.c_int64 * n)(*v)
    ptr = lambda name: C.c_void_p(0 if a.get('null') == name else a['ptr'])
    arr = lambda name, v: None if a.get('null') == name else v
    rc = _lib.lib().masr_op_attention(
        None, ptr('q'), ptr('k'), ptr('v'), ptr('out'), ptr('ptab'), a['n_pos'], ptr('u'), ptr('vb'), a['nseq'],
        arr('q_off', i64(a['off'])), i64(a.get('k_off', a['off'])), i64(a['off']), i64(a['off']), i32(a['nq']), arr('nk', i32(a['nk'])),
        i32(a['klen']), i32(a['pos0']), i32(a['q_abs0']), a['heads'], a['q_stride'], a['kv_stride'], a['chunk_size'],
        a['pos_stride'], a['group'], a['t_true'], None)
    return rc, _lib.lib().masr_last_error().decode()


@pytest.mark.parametrize('change,word', [
    ({'null': 'q'}, 'null argument'), ({'null': 'ptab'}, 'null argument'), ({'null': 'vb'}, 'null argument'),
    ({'null': 'q_off'}, 'null argument'), ({'null': 'nk'}, 'null argument'),
    ({'nseq': 0}, 'nseq'), ({'nseq': -1}, 'nseq'),
    ({'heads': 2}, 'heads'), ({'heads': 6}, 'heads'), ({'heads': 16}, 'heads'),
    ({'group': 2}, 'group'), ({'group': 0}, 'group'),
    ({'nq': [-1]}, 'negative'), ({'nk': [-1], 'klen': [-1]}, 'negative'), ({'klen': [-1]}, 'negative'),
    ({'pos0': [-1]}, 'negative'), ({'q_abs0': [-1]}, 'negative'), ({'off': [-4]}, 'negative'),
    ({'klen': [9]}, 'klen > nk'),
    ({'q_stride': 252}, 'stride'), ({'kv_stride': 255}, 'stride'), ({'heads': 8}, 'stride'),
    ({'q_stride': 258}, 'multiples of 4'), ({'k_off': [2]}, 'multiples of 4'), ({'ptr': 4104}, '16-byte'),
    ({'chunk_size': -1}, 'chunk_size'), ({'pos_stride': 0}, 'pos_stride'),
    ({'n_pos': 8, 'pos0': [1]}, 'positional table'), ({'n_pos': 14, 'pos_stride': 2}, 'positional table'),
    ({'group': 3}, 'grouped'), ({'group': 3, 'q_stride': 768, 'kv_stride': 768, 't_true': 24, 'n_pos': 23}, 'positional table'),
])
def test_op_attention_refuses(built_lib, change, word):
    rc, msg = call(**change)
    assert rc != 0 and 'masr_op_attention' in msg and word in msg, (rc, msg)


@pytest.mark.parametrize('change', [{}, {'heads': 8, 'q_stride': 1536, 'kv_stride': 1024}, {'n_pos': 15, 'pos_stride': 2, 'klen': [0]},
                                    {'group': 3, 'q_stride': 768, 'kv_stride': 768, 't_true': 24, 'n_pos': 24}])
def test_op_attention_accepts_up_to_the_engine(built_lib, change):
    """well-formed arguments pass every refusal; without an engine the call then stops at the handle, before any device work"""
    rc, msg = call(**change)
    assert rc != 0 and msg == 'null engine', (rc, msg)
