"""Layer layouts off the shipped ones (Squeezeformer reduce_idx / recover_idx, Efficient Conformer stride_layer_idx and leading
group_layer_idx), the parts that need no GPU: the oracle against the committed fixture tests/golden/layouts_v50.npz at every accepted
layout, in float32 and float64, full context and chunked; what the reference itself does with every layout the engine refuses; the
refusals of the configuration check and of masr_create, by name; the fixture against its own recipe; and, for the seeds of
tests/test_gpu_layouts.py, that the float32 oracle leaves at most 2 % of the valid frames without a decided argmax."""
import ctypes
import os

import numpy as np
import pytest
import torch

from masr_amd import _lib
from masr_amd.engine import _layer_layout, _validate_encoder_conf
from oracle import f64, shims
from tests import budget
from tools import make_layout_golden as tool

IDS = [tool.name_of(l) for l in tool.LAYOUTS]


@pytest.fixture(scope='module')
def golden():
    return np.load(tool.OUT)


# ---- the oracle against the fixture ----------------------------------------------------------------------------------------------
# float32: two float32 evaluations of the same probabilities, the recorded one of the modules and the restatement's on whatever CPU,
# BLAS build and thread count this machine has (float32 matmuls are not bit-stable across those): each sits a few 1e-6 from the
# float64 one, so they are within 1e-5 of each other, 100 x under the 1e-3 parity bound (the rule of test_conv_kernel_cpu.py and
# test_wide_cpu.py for a record recomputed on another machine).  float64: the distance is the reference's own float32 error, bounded
# like the recorded float64 distances of tests/test_activation_cpu.py (< 1e-4, ten times under the 1e-3 parity bound)
TOL = {torch.float32: 1e-5, torch.float64: 1e-4}


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('layout', tool.LAYOUTS, ids=IDS)
def test_oracle_reproduces_the_fixture(golden, layout, dtype):
    feats, lens = tool.ragged_batch(tool.T_BATCH[0])
    name = tool.name_of(layout)
    for streaming in (True, False):
        sd = tool.state_dict(layout, streaming)
        got = f64.forward(layout[0], sd, feats, lens, dtype, **tool.oracle_kw(layout, streaming))['probs']
        want = golden[f'{name}_{"s" if streaming else "n"}_b3']
        assert got.dtype == dtype and tuple(got.shape) == want.shape == (3, tool.contract_frames(layout), tool.V)
        diff = float(np.abs(budget.as64(got) - want).max())
        print(f'{name} streaming={streaming} {dtype}: full {diff:.2e}')
        assert diff < TOL[dtype], (name, streaming, diff)
    got = f64.chunk_run(layout[0], tool.state_dict(layout, True), tool.chunked_input(), tool.CHUNKS, dtype, required_cache_size=-1,
                        **tool.oracle_kw(layout))[0]
    want = golden[f'{name}_s_chunks']
    assert got.dtype == dtype and tuple(got.shape) == want.shape
    diff = float(np.abs(budget.as64(got) - want).max())
    print(f'{name} {dtype}: chunks {diff:.2e}')
    assert diff < TOL[dtype], (name, diff)


def test_layouts_are_different_functions(golden):
    """every layout is its own model: no two records of one family agree (a layout keyword that is dropped on the way would show)"""
    for fam in (tool.EFFICIENT, tool.SQUEEZEFORMER):
        for i, a in enumerate(fam):
            for b in fam[:i]:
                for key in ('_s_b3', '_n_b3', '_s_chunks'):
                    assert np.abs(golden[tool.name_of(a) + key] - golden[tool.name_of(b) + key]).max() > 1e-3, (a, b, key)


def test_squeezeformer_chunk_oracle_reads_null_like_the_full_one():
    """recover_idx: null keeps half rate to the end in both entry points of the oracle (the reference's time_reduce = 'normal');
    reduce_idx: null ignores recover_idx in both"""
    from oracle import squeezeformer as osq
    sd = tool.state_dict(('squeezeformer', 4, 2, None))
    x = tool.chunked_input()[:1, :67]
    z = torch.zeros(0, 0, 0, 0)
    with torch.no_grad():
        for c in (None, 4):
            assert osq.encoder_full(sd, x, torch.tensor([67]), reduce_idx=2, recover_idx=c, causal=True).shape[1] == 8
            p, att, _ = osq.get_encoder_out_chunk(sd, x, 0, -1, z, z, reduce_idx=2, recover_idx=c)
            assert p.shape[1] == 8 and att.shape[2] == 16
        full = osq.encoder_full(sd, x, torch.tensor([67]), reduce_idx=None, recover_idx=3, causal=True)
        assert torch.equal(full, osq.encoder_full(sd, x, torch.tensor([67]), reduce_idx=None, recover_idx=None, causal=True))
        a = osq.get_encoder_out_chunk(sd, x, 0, -1, z, z, reduce_idx=None, recover_idx=3)
        b = osq.get_encoder_out_chunk(sd, x, 0, -1, z, z, reduce_idx=None, recover_idx=None)
        assert all(torch.equal(u, v) for u, v in zip(a, b)) and a[0].shape[1] == 16


# ---- what the reference does with the refused layouts ------------------------------------------------------------------------------
def test_refused_layouts_in_the_reference(golden):
    """the recorded outcome of the reference for every refused layout.  REFUSED: its constructor or forward raises, or its frame count
    is one the engine's contract excludes.  REFUSED_BUT_RUNS: it runs at the contract's rate (an index that names no layer is ignored;
    grouped attention behind the stride layer works there) -- refused by the engine all the same, and recorded as what it is."""
    rec = dict(line.split('|') for line in golden['refused'].tolist())
    assert list(rec) == [tool.name_of(l) for l in tool.REFUSED + tool.REFUSED_BUT_RUNS]
    for layout in tool.REFUSED:
        got = rec[tool.name_of(layout)]
        assert got == 'error' or (got.startswith('frames ') and int(got.split()[1]) != tool.contract_frames(layout)), (layout, got)
    for layout in tool.REFUSED_BUT_RUNS:
        assert rec[tool.name_of(layout)] == f'frames {tool.contract_frames(layout)}', layout
    # the oracle behaves the same way (where the reference checkout is absent it is what the recipe runs)
    with torch.no_grad():
        for layout in tool.REFUSED + tool.REFUSED_BUT_RUNS:
            assert tool.outcome(layout) == rec[tool.name_of(layout)], layout


# ---- the configuration check -----------------------------------------------------------------------------------------------------
def test_validate_accepts_every_layout_of_the_fixture_and_the_shipped_ones():
    for layout in tool.LAYOUTS:
        fam, L, a, b = layout
        _validate_encoder_conf(fam, tool.encoder_conf(layout), tool.state_dict(layout), True)
        assert _layer_layout(fam, tool.encoder_conf(layout)) == (-1 if a is None else a, -1 if b is None else b)
    assert _layer_layout('squeezeformer', {}) == (5, 11) and _layer_layout('efficient_conformer', {}) == (3, 4)
    assert _layer_layout('squeezeformer', {'num_blocks': 2, 'reduce_idx': None, 'recover_idx': None}) == (-1, -1)
    assert _layer_layout('efficient_conformer', {'num_blocks': 4, 'efficient_conf': {'stride_layer_idx': 2, 'group_layer_idx': []}}) == (2, 0)


KEY = {'s': 'stride_layer_idx', 'g': 'group_layer_idx', 'r': 'reduce_idx', 'c': 'recover_idx'}
# (layout, the YAML key the refusal names)
REFUSALS = [(('efficient_conformer', 4, -1, 0), 's'), (('efficient_conformer', 4, 4, 4), 's'), (('efficient_conformer', 4, 5, 0), 's'),
            (('efficient_conformer', 4, 1, 3), 'g'), (('efficient_conformer', 4, 0, 2), 'g'),
            (('squeezeformer', 4, -2, 3), 'r'), (('squeezeformer', 4, 4, 5), 'r'), (('squeezeformer', 4, 7, 9), 'r'),
            (('squeezeformer', 4, 2, 1), 'c'), (('squeezeformer', 4, 3, 0), 'c'), (('squeezeformer', 4, 2, None), 'c'),
            (('squeezeformer', 4, 2, 4), 'c')]


def test_every_refused_layout_of_the_fixture_has_a_refusal_test():
    assert sorted(map(str, (l for l, _ in REFUSALS))) == sorted(map(str, tool.REFUSED + tool.REFUSED_BUT_RUNS))


@pytest.mark.parametrize('layout,key', REFUSALS, ids=[tool.name_of(l) for l, _ in REFUSALS])
def test_validate_refuses_by_name(layout, key):
    with pytest.raises(_lib.MasrError) as ei:
        _validate_encoder_conf(layout[0], tool.encoder_conf(layout), None, True)
    msg = str(ei.value)
    assert KEY[key] in msg and layout[0] in msg and repr({'s': layout[2], 'g': list(range(layout[3] or 0)), 'r': layout[2],
                                                           'c': layout[3]}[key]) in msg, msg


def test_validate_refuses_what_has_no_index_form():
    """a grouped layer that is not a leading one (a negative entry included), two stride layers, a value that is no integer"""
    for groups in ([-1], [1], [0, 2]):
        with pytest.raises(_lib.MasrError, match='group_layer_idx'):
            _layer_layout('efficient_conformer', {'num_blocks': 4, 'efficient_conf': {'stride_layer_idx': [3], 'group_layer_idx': groups}})
    with pytest.raises(_lib.MasrError, match='stride_layer_idx'):
        _layer_layout('efficient_conformer', {'num_blocks': 4, 'efficient_conf': {'stride_layer_idx': [1, 3], 'stride': [2, 2]}})
    for key, v in (('reduce_idx', 1.0), ('recover_idx', '3'), ('reduce_idx', True)):
        with pytest.raises(_lib.MasrError, match=key):
            _layer_layout('squeezeformer', dict({'num_blocks': 4, 'reduce_idx': 1, 'recover_idx': 3}, **{key: v}))


# ---- masr_create -------------------------------------------------------------------------------------------------------------------
def _create(layout, causal=1):
    """masr_create with the configuration the facade would pass -> (return code, handle value, message)"""
    fam, L, a, b = layout
    kind = 1 if fam == 'squeezeformer' else 2
    cfg = _lib.MasrConfig(model_kind=kind, d_model=256, heads=4, d_ff=2048, num_blocks=L, cnn_kernel=31 if kind == 1 else 15, n_mels=80,
                          vocab_size=50, causal=causal, max_pos=5000, device_id=0)
    cfg.reserved[0], cfg.reserved[1] = (-1 if a is None else a), (-1 if b is None else b)
    if kind == 2:
        cfg.reserved[2] = 3
    h = ctypes.c_void_p()
    rc = _lib.lib().masr_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = _lib.lib().masr_last_error().decode()
    value = h.value
    if rc == 0:                       # (a machine with a GPU: the engine exists)
        _lib.lib().masr_destroy(h)
    return rc, value, msg


@pytest.mark.parametrize('layout', tool.LAYOUTS + [('squeezeformer', 12, 5, 11), ('efficient_conformer', 12, 3, 4),
                                                   ('squeezeformer', 2, None, None), ('squeezeformer', 4, None, -7)],
                         ids=lambda l: tool.name_of(l))
def test_masr_create_gets_past_the_layout_check(built_lib, layout):
    """fails only for want of a device here (or succeeds where there is one)"""
    rc, _, msg = _create(layout)
    assert rc == 0 or not any(k in msg for k in KEY.values()), msg
    if rc:
        assert 'hip' in msg.lower() or 'device' in msg.lower(), msg


# (the C level also takes what no YAML can say: a negative NUMBER of grouped layers)
C_REFUSALS = REFUSALS + [(('efficient_conformer', 4, 3, -1), 'g'), (('efficient_conformer', 4, 3, 5), 'g')]


@pytest.mark.parametrize('layout,key', C_REFUSALS, ids=[tool.name_of(l) for l, _ in C_REFUSALS])
def test_masr_create_refuses_by_name(built_lib, layout, key):
    """before any allocation: no handle comes back, and the message names the YAML key, the slot and the value"""
    rc, value, msg = _create(layout)
    assert rc != 0 and not value
    slot = 'reserved[0]' if key in 'sr' else 'reserved[1]'
    given = layout[2] if key in 'sr' else (-1 if layout[3] is None else layout[3])
    assert KEY[key] in msg and slot in msg and f'= {given}' in msg and layout[0] in msg, msg
    assert 'hip' not in msg.lower().replace('masr_hip', ''), msg


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def test_fixture_equals_its_recipe(golden):
    """the committed file, recomputed from its seeds: through the live reference where it exists, else through the oracle (which
    test_oracle_reproduces_the_fixture holds to it)"""
    import tempfile
    assert os.path.getsize(tool.OUT) <= tool.LIMIT == 1 << 20
    live = shims.reference_available()
    keep = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        if live:
            with tempfile.TemporaryDirectory() as tmp:
                got = tool.record(tmp)
        else:
            got = tool.record()
    finally:
        torch.set_num_threads(keep)
    assert sorted(got) == sorted(golden.files)
    assert got['refused'].tolist() == golden['refused'].tolist()
    for k in golden.files:
        if k == 'refused':
            continue
        assert got[k].shape == golden[k].shape and got[k].dtype == golden[k].dtype == np.float32, k
        diff = float(np.abs(got[k] - golden[k]).max())
        if live:          # the recipe itself, on the kind of machine that recorded the file: the same bits
            assert np.array_equal(got[k], golden[k]), (k, diff)
        else:
            # two float32 evaluations of probabilities on different CPUs / BLAS builds: each sits a few 1e-6 from the float64 one, so
            # they are within 1e-5 of each other, 100 x under the 1e-3 parity bound (the rule of test_conv_kernel_cpu.py)
            assert diff < 1e-5, (k, diff)


# ---- the seeds of the GPU module -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', tool.LAYOUTS, ids=IDS)
def test_oracle_argmax_is_decided_on_the_gpu_modules_batches(layout):
    """tests/test_gpu_layouts.py judges the argmax where budget.argmax_margin decides it and allows 2 % of the valid frames to stay
    undecided: the float32 oracle's own run has to stay within that cap for these seeds before the GPU is asked"""
    rate = 8 if layout[0] == 'efficient_conformer' else 4
    for T in tool.T_BATCH:
        feats, lens = tool.ragged_batch(T)
        assert int(lens[0]) == T
        for streaming in (True, False):
            r32, r64 = f64.both(layout[0], tool.state_dict(layout, streaming), feats, lens, **tool.oracle_kw(layout, streaming))
            mask = budget.valid_mask(r64['probs'].shape, lens, rate)
            e_ref = np.abs(budget.as64(r32['probs']) - budget.as64(r64['probs']))[mask].max()
            decided = budget.argmax_margin(r64['probs'], e_ref) & mask
            undecided = 1 - decided[mask].mean()
            print(f'{tool.name_of(layout)} T={T} streaming={streaming}: e_ref {e_ref:.2e}, undecided {undecided:.3f}')
            assert undecided <= 0.02, (layout, T, streaming, undecided)
            same = budget.as64(r32['probs']).argmax(-1)[decided] == budget.as64(r64['probs']).argmax(-1)[decided]
            assert same.all()
