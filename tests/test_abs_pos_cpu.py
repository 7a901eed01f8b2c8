"""pos_enc_layer_type abs_pos / no_pos for the Conformer, the parts that need no GPU: what the configuration check and masr_create
admit and refuse, by name; the synthetic checkpoints; the committed fixture tests/golden/conformer_abs_pos_v50.npz against its own
recipe; and the fixture's float32 record under the budget rule against its float64 record (the rule is satisfiable by the
reference alone on these inputs)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from masr_amd import _lib
from masr_amd.engine import POS_ENC_LAYER_TYPES, REL_POS_KEYS, _validate_encoder_conf
from masr_amd.utils import synthetic
from tests import budget
from tests.test_wide_cpu import PARENT_DIGEST, _digest
from tools import make_abs_pos_golden as tool

FAMILY = {0: 'conformer', 1: 'squeezeformer', 2: 'efficient_conformer'}


def _sd(mode='rel_pos', **kw):
    return synthetic.conformer_state_dict(0, 16, num_blocks=1, pos_enc_layer_type=mode, **kw)


# ---- _validate_encoder_conf ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['abs_pos', 'no_pos'])
@pytest.mark.parametrize('width,heads', [(256, 4), (512, 8)])
@pytest.mark.parametrize('streaming', [True, False])
def test_validate_accepts_the_plain_modes_for_the_conformer(mode, width, heads, streaming):
    conf = {'output_size': width, 'attention_heads': heads, 'pos_enc_layer_type': mode}
    _validate_encoder_conf('conformer', conf, None, streaming)
    _validate_encoder_conf('conformer', conf, _sd(mode, d=width, heads=heads), streaming)


def test_slot_values():
    assert POS_ENC_LAYER_TYPES == {'rel_pos': 0, 'abs_pos': 1, 'no_pos': 2}


@pytest.mark.parametrize('family', ['squeezeformer', 'efficient_conformer'])
@pytest.mark.parametrize('mode', ['abs_pos', 'no_pos'])
def test_validate_refuses_the_plain_modes_for_the_other_families_by_key_and_family(family, mode):
    with pytest.raises(_lib.MasrError) as ei:
        _validate_encoder_conf(family, {'pos_enc_layer_type': mode}, None)
    msg = str(ei.value)
    assert 'pos_enc_layer_type' in msg and family in msg and mode in msg and 'rel_pos' in msg, msg
    _validate_encoder_conf(family, {'pos_enc_layer_type': 'rel_pos'}, None)


@pytest.mark.parametrize('value', ['rel_pos_v2', 'abs', None, 1])
def test_validate_refuses_an_unknown_value(value):
    with pytest.raises(_lib.MasrError, match='pos_enc_layer_type'):
        _validate_encoder_conf('conformer', {'pos_enc_layer_type': value}, None)


def test_validate_refuses_a_rel_pos_config_on_a_plain_checkpoint_by_key():
    for mode in ('abs_pos', 'no_pos'):
        with pytest.raises(_lib.MasrError) as ei:
            _validate_encoder_conf('conformer', {'pos_enc_layer_type': 'rel_pos'}, _sd(mode))
        msg = str(ei.value)
        assert 'pos_enc_layer_type' in msg and 'rel_pos' in msg and 'has no' in msg, msg
        assert any(k in msg for k in REL_POS_KEYS), msg
    with pytest.raises(_lib.MasrError, match='pos_enc_layer_type'):            # the default is rel_pos
        _validate_encoder_conf('conformer', {}, _sd('abs_pos'))
    sd = _sd()                                   # one of the three missing is a disagreement too, named by that key
    del sd['encoder.encoders.0.self_attn.pos_bias_u']
    with pytest.raises(_lib.MasrError, match='pos_bias_u'):
        _validate_encoder_conf('conformer', {}, sd)


@pytest.mark.parametrize('mode', ['abs_pos', 'no_pos'])
def test_validate_refuses_a_plain_config_on_a_rel_pos_checkpoint_by_key(mode):
    with pytest.raises(_lib.MasrError) as ei:
        _validate_encoder_conf('conformer', {'pos_enc_layer_type': mode}, _sd())
    msg = str(ei.value)
    assert 'pos_enc_layer_type' in msg and mode in msg and 'holds' in msg and any(k in msg for k in REL_POS_KEYS), msg


# ---- masr_create -------------------------------------------------------------------------------------------------------------------
def _create(kind, width, heads, pos):
    cfg = _lib.MasrConfig(model_kind=kind, d_model=width, heads=heads, d_ff=2048, num_blocks=2, cnn_kernel=31 if kind == 1 else 15,
                          n_mels=80, vocab_size=50, causal=1, max_pos=5000, device_id=0)
    if kind == 1:
        cfg.reserved[0], cfg.reserved[1] = -1, -1
    cfg.reserved[2] = pos
    h = ctypes.c_void_p()
    rc = _lib.lib().masr_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = _lib.lib().masr_last_error().decode()
    if rc == 0:                       # (a machine with a GPU: the engine exists)
        _lib.lib().masr_destroy(h)
    return rc, msg


@pytest.mark.parametrize('pos', [0, 1, 2])
@pytest.mark.parametrize('width,heads', [(256, 4), (512, 8)])
def test_masr_create_gets_past_the_pos_enc_check(built_lib, pos, width, heads):
    """values 0, 1, 2 fail only for want of a device here (or succeed where there is one)"""
    rc, msg = _create(0, width, heads, pos)
    assert rc == 0 or 'pos_enc_layer_type' not in msg, msg
    if rc:
        assert 'hip' in msg.lower() or 'device' in msg.lower(), msg


@pytest.mark.parametrize('pos', [3, -1])
def test_masr_create_refuses_other_values_by_name(built_lib, pos):
    rc, msg = _create(0, 256, 4, pos)
    assert rc != 0 and 'pos_enc_layer_type' in msg and 'reserved[2]' in msg and str(pos) in msg, msg
    assert 'rel_pos' in msg and 'abs_pos' in msg and 'no_pos' in msg, msg


def test_masr_create_refuses_a_plain_mode_for_the_squeezeformer_by_name(built_lib):
    rc, msg = _create(1, 256, 4, 1)
    assert rc != 0 and 'pos_enc_layer_type' in msg and 'squeezeformer' in msg and 'rel_pos' in msg, msg
    rc, msg = _create(1, 256, 4, 0)
    assert rc == 0 or 'pos_enc_layer_type' not in msg, msg


# ---- synthetic checkpoints ---------------------------------------------------------------------------------------------------------
def test_synthetic_default_is_unchanged_and_the_plain_dicts_lack_exactly_the_three_tensors():
    rel = _sd()
    assert _digest(rel) == PARENT_DIGEST == _digest(synthetic.conformer_state_dict(0, 16, num_blocks=1))
    for mode in ('abs_pos', 'no_pos'):
        plain = synthetic.conformer_state_dict(0, 16, num_blocks=2, pos_enc_layer_type=mode)
        full = synthetic.conformer_state_dict(0, 16, num_blocks=2)
        gone = sorted(set(full) - set(plain))
        assert gone == sorted(f'encoder.encoders.{i}.{k}' for i in range(2) for k in REL_POS_KEYS), gone
        assert not set(plain) - set(full)
        assert all(torch.equal(plain[k], full[k]) for k in plain)
    with pytest.raises(AssertionError):
        synthetic.conformer_state_dict(0, 16, num_blocks=1, pos_enc_layer_type='sinusoid')


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def z():
    return np.load(tool.OUT)


def test_fixture_holds_every_case(z):
    assert os.path.getsize(tool.OUT) <= tool.LIMIT
    want = set()
    for mode, width, streaming in tool.builds():
        k = tool.prefix(mode, width, streaming)
        names = ['b3_probs', 'b3_enc'] + ([f'single_probs_{T}' for T in tool.SINGLE_T] if width == 256 else [])
        if streaming:
            names += [f'chunk_probs_{r}' for r in tool.CACHE_SIZES]
            want |= {k + f'chunk_{c}_{r}' for c in ('att', 'cnn') for r in tool.CACHE_SIZES}
        want |= {k + n for n in names} | {k + n + tool.D64 for n in names}
    assert set(z.files) == want
    assert tool.builds() == [('abs', 256, True), ('abs', 256, False), ('no', 256, True), ('no', 256, False), ('abs', 512, True),
                             ('abs', 512, False)]
    assert z['abs_256_s_b3_probs'].shape == (3, 32, 50) and z['abs_256_s_single_probs_403'].shape == (1, 100, 50)
    assert z['abs_256_s_chunk_probs_16'].shape == (3, 16, 50)
    assert z['abs_256_s_chunk_att_-1'].shape == (2, 4, 48, 16) and z['abs_512_s_chunk_att_16'].shape == (2, 8, 16, 16)
    assert z['no_256_s_chunk_cnn_-1'].shape == (2, 1, 64, 14) and z['abs_512_s_chunk_cnn_16'].shape == (2, 1, 128, 14)
    # the two modes are different functions of the same weights, and the offset matters to abs_pos
    assert np.abs(z['abs_256_s_b3_probs'] - z['no_256_s_b3_probs']).max() > 1e-2


def test_fixture_equals_its_recipe(z):
    """the committed file, recomputed from its seeds through the live reference modules"""
    import tempfile
    from oracle import shims
    if not shims.reference_available():
        pytest.skip('the reference checkout is not on this machine, and oracle/ has no abs_pos / no_pos restatement to recompute '
                    'the records with: the fixture can only be re-recorded where the reference is')
    keep = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        with tempfile.TemporaryDirectory() as tmp:
            got = tool.record(tmp)
    finally:
        torch.set_num_threads(keep)
    assert sorted(got) == sorted(z.files)
    for k in z.files:
        assert got[k].shape == z[k].shape and got[k].dtype == z[k].dtype == np.float32, k
        # the recipe itself, on the kind of machine that recorded the file: the same bits
        assert np.array_equal(got[k], z[k]), (k, float(np.abs(got[k] - z[k]).max()))


def _budget_cases():
    for mode, width, streaming in tool.builds():
        k = tool.prefix(mode, width, streaming)
        yield k + 'b3_probs', tool.LENS
        yield k + 'b3_enc', tool.LENS
        if width == 256:
            for T in tool.SINGLE_T:
                yield k + f'single_probs_{T}', None
        if streaming:
            for r in tool.CACHE_SIZES:
                yield k + f'chunk_probs_{r}', None


@pytest.mark.parametrize('key,lens', list(_budget_cases()))
def test_float32_record_holds_the_budget_against_the_float64_record(z, key, lens):
    """yardstick and candidate are both the reference's float32 output: ratios 1.0 by construction, and the float64 record is a
    usable truth (finite, a reference error above zero and far under the 1e-3 parity bound)"""
    y32, y64 = z[key], tool.truth(z, key)
    assert y64.dtype == np.float64 and np.isfinite(y64).all()
    mask = budget.valid_mask(y32.shape, lens) if lens else None
    f = budget.check(key, y64, y32, y32, mask)
    assert 0 < f['max_ref'] < 1e-4, f
    assert f['ratio_max'] <= 1.0 and f['ratio_rms'] <= 1.0, f
