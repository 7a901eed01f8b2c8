"""encoder_conf.activation_type for the Conformer, the parts that need no GPU: what the configuration check, masr_create and
masr_op_gemm admit and refuse, by name; the helper tests/activation_ref.py against oracle.conformer (swish, bit for bit) and
against the live reference model built with each activation; and the committed fixture
tests/golden/conformer_activation_v50.npz against its own recipe."""
import ctypes
import os

import numpy as np
import pytest
import torch

from masr_amd import _lib
from masr_amd.engine import ACTIVATION_TYPES, _validate_encoder_conf
from masr_amd.utils import synthetic
from oracle import conformer as oc
from oracle import f64, shims
from tests import activation_ref as ar
from tools import make_activation_golden as tool

SIX = ('swish', 'relu', 'gelu', 'tanh', 'hardtanh', 'selu')
CHUNKS = [(0, 67), (64, 67), (128, 67)]


# ---- _validate_encoder_conf ------------------------------------------------------------------------------------------------------
def test_slot_values():
    assert ACTIVATION_TYPES == {'swish': 0, 'relu': 1, 'gelu': 2, 'tanh': 3, 'hardtanh': 4, 'selu': 5}
    assert tuple(ACTIVATION_TYPES) == SIX and tool.ACTS == ar.NEW == SIX[1:]


@pytest.mark.parametrize('act', SIX)
@pytest.mark.parametrize('width,heads', [(256, 4), (512, 8)])
@pytest.mark.parametrize('streaming', [True, False])
def test_validate_accepts_the_six_for_the_conformer(act, width, heads, streaming):
    conf = {'output_size': width, 'attention_heads': heads, 'activation_type': act}
    _validate_encoder_conf('conformer', conf, None, streaming)
    _validate_encoder_conf('conformer', conf, synthetic.conformer_state_dict(0, 16, d=width, heads=heads, num_blocks=1), streaming)


@pytest.mark.parametrize('value', ['mish', None, 3])
def test_validate_refuses_an_unknown_value_by_key(value):
    with pytest.raises(_lib.MasrError, match='activation_type') as ei:
        _validate_encoder_conf('conformer', {'activation_type': value}, None)
    assert repr(value) in str(ei.value)


@pytest.mark.parametrize('family', ['squeezeformer', 'efficient_conformer'])
@pytest.mark.parametrize('act', SIX[1:])
def test_validate_refuses_the_new_values_for_the_other_families_by_key_and_family(family, act):
    with pytest.raises(_lib.MasrError) as ei:
        _validate_encoder_conf(family, {'activation_type': act}, None)
    msg = str(ei.value)
    assert 'activation_type' in msg and family in msg and act in msg and 'swish' in msg, msg
    _validate_encoder_conf(family, {'activation_type': 'swish'}, None)


@pytest.mark.parametrize('act', SIX[1:])
def test_validate_refuses_the_new_values_with_batch_norm_by_both_keys(act):
    with pytest.raises(_lib.MasrError) as ei:
        _validate_encoder_conf('conformer', {'activation_type': act, 'cnn_module_norm': 'batch_norm'}, None)
    msg = str(ei.value)
    assert 'activation_type' in msg and 'cnn_module_norm' in msg and 'batch_norm' in msg and act in msg, msg


def test_validate_still_accepts_batch_norm_with_swish():
    sd = synthetic.conformer_state_dict(0, 16, num_blocks=1, cnn_module_norm='batch_norm')
    _validate_encoder_conf('conformer', {'cnn_module_norm': 'batch_norm'}, sd, True)
    _validate_encoder_conf('conformer', {'cnn_module_norm': 'batch_norm', 'activation_type': 'swish'}, sd, True)


# ---- masr_create / masr_op_gemm --------------------------------------------------------------------------------------------------
def _create(act, norm=0, width=256, heads=4):
    cfg = _lib.MasrConfig(model_kind=0, d_model=width, heads=heads, d_ff=2048, num_blocks=2, cnn_kernel=15, n_mels=80, vocab_size=50,
                          causal=1, max_pos=5000, device_id=0)
    cfg.reserved[0], cfg.reserved[4] = norm, act
    h = ctypes.c_void_p()
    rc = _lib.lib().masr_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = _lib.lib().masr_last_error().decode()
    if rc == 0:                       # (a machine with a GPU: the engine exists)
        _lib.lib().masr_destroy(h)
    return rc, msg


@pytest.mark.parametrize('act', range(6))
@pytest.mark.parametrize('width,heads', [(256, 4), (512, 8)])
def test_masr_create_gets_past_the_activation_check(built_lib, act, width, heads):
    """values 0 .. 5 fail only for want of a device here (or succeed where there is one)"""
    rc, msg = _create(act, width=width, heads=heads)
    assert rc == 0 or 'activation_type' not in msg, msg
    if rc:
        assert 'hip' in msg.lower() or 'device' in msg.lower(), msg


@pytest.mark.parametrize('act', [6, -1])
def test_masr_create_refuses_other_values_by_name(built_lib, act):
    rc, msg = _create(act)
    assert rc != 0 and 'activation_type' in msg and 'reserved[4]' in msg and str(act) in msg, msg
    assert all(name in msg for name in SIX), msg


def test_masr_create_refuses_an_activation_with_batch_norm(built_lib):
    rc, msg = _create(2, norm=1)
    assert rc != 0 and 'activation_type' in msg and 'batch_norm' in msg, msg
    rc, msg = _create(0, norm=1)                         # swish with batch_norm stays accepted
    assert rc == 0 or 'activation_type' not in msg, msg


@pytest.mark.parametrize('act', [8, -1])
def test_masr_op_gemm_refuses_an_unknown_act_before_the_engine_is_touched(built_lib, act):
    """no engine, no device: the refusal names the argument and the value"""
    rc = _lib.lib().masr_op_gemm(None, None, None, None, None, None, 1, 64, 32, act, ctypes.c_float(1.0), None)
    msg = _lib.lib().masr_last_error().decode()
    assert rc != 0 and 'masr_op_gemm' in msg and 'act' in msg and str(act) in msg, msg
    rc = _lib.lib().masr_op_gemm(None, None, None, None, None, None, 1, 64, 32, 6, ctypes.c_float(1.0), None)
    assert rc != 0 and 'null engine' in _lib.lib().masr_last_error().decode()          # a known value goes on to the engine


# ---- the helper ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('streaming', [True, False], ids=['s', 'n'])
def test_helper_with_swish_is_the_oracle_bit_for_bit(dtype, streaming):
    sd = f64.cast_state_dict(tool.state_dict(256), dtype)
    feats, lens = tool.ragged_inputs()
    feats = feats.to(dtype)
    with torch.no_grad():
        for chunk in (-1, 16):
            want = oc.encoder_full(sd, feats, lens, chunk, streaming=streaming)
            assert torch.equal(ar.encoder_full(sd, feats, lens, 'swish', chunk, streaming=streaming), want)
        assert torch.equal(ar.get_encoder_out(sd, feats, lens, 'swish', streaming=streaming),
                           oc.get_encoder_out(sd, feats, lens, streaming=streaming))
    assert want.dtype == dtype


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_helper_chunk_runner_with_swish_is_the_oracle_bit_for_bit(dtype):
    sd, x = tool.state_dict(256), tool.single_inputs()[403]
    for rcs in (-1, 16):
        want = f64.chunk_run('conformer', sd, x, CHUNKS, dtype, required_cache_size=rcs)
        got = ar.chunk_run(sd, x, CHUNKS, 'swish', dtype, required_cache_size=rcs)
        assert all(torch.equal(g, w) and g.dtype == dtype for g, w in zip(got, want))


def test_helper_activations_are_torch_defaults():
    x = torch.linspace(-8, 8, 4001, dtype=torch.float64)
    assert torch.equal(ar.ACTS['gelu'](x), 0.5 * x * (1 + torch.erf(x / 2 ** 0.5))) or \
        (ar.ACTS['gelu'](x) - 0.5 * x * (1 + torch.erf(x / 2 ** 0.5))).abs().max() < 1e-15
    assert torch.equal(ar.ACTS['hardtanh'](x), x.clamp(-1, 1))
    selu = 1.0507009873554805 * torch.where(x > 0, x, 1.6732632423543772 * torch.expm1(x))
    assert (ar.ACTS['selu'](x) - selu).abs().max() < 1e-15
    assert torch.equal(ar.ACTS['swish'](x), torch.nn.functional.silu(x))


@pytest.mark.parametrize('act', SIX[1:])
def test_helper_equals_the_live_reference(act, tmp_path):
    """the reference model built with the activation, against the restatement: the tolerances of the Conformer encoder pins of
    tests/test_oracle_golden.py (encoder rows 2e-5, probabilities 2e-6)"""
    if not shims.reference_available():
        pytest.skip('the reference checkout is not on this machine')
    sd, x = tool.state_dict(256), tool.single_inputs()[403]
    feats, lens = tool.ragged_inputs()
    with torch.no_grad():
        for streaming in (True, False):
            m = tool.model(act, 256, streaming, str(tmp_path))
            np.testing.assert_allclose(ar.encoder_full(sd, feats, lens, act, streaming=streaming).numpy(),
                                       m.encoder(feats, lens, -1, -1)[0].numpy(), atol=2e-5)
            np.testing.assert_allclose(ar.get_encoder_out(sd, feats, lens, act, streaming=streaming).numpy(),
                                       m.get_encoder_out(feats, lens).numpy(), atol=2e-6)
        m = tool.model(act, 256, True, str(tmp_path))
        np.testing.assert_allclose(ar.encoder_full(sd, feats, lens, act, 16).numpy(), m.encoder(feats, lens, 16, -1)[0].numpy(),
                                   atol=2e-5)
        att, cnn, off = torch.zeros(0, 0, 0, 0), torch.zeros(0, 0, 0, 0), 0
        mine = ar.chunk_run(sd, x, CHUNKS, act, required_cache_size=16)
        outs = []
        for cur, n in CHUNKS:
            p, att, cnn = m.get_encoder_out_chunk(x[:1, cur:cur + n], off, 16, att, cnn)
            off += p.shape[1]
            outs.append(p[0])
        np.testing.assert_allclose(mine[0].numpy(), torch.cat(outs).numpy(), atol=2e-6)
        np.testing.assert_allclose(mine[1].numpy(), att.numpy(), atol=2e-5)
        np.testing.assert_allclose(mine[2].numpy(), cnn.numpy(), atol=2e-5)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def test_fixture_holds_every_case_under_the_size_limit():
    assert os.path.getsize(tool.OUT) <= tool.LIMIT == 1 << 20
    z = np.load(tool.OUT)
    want = set()
    for b in tool.builds():
        names, d64 = tool.names_of(*b)
        want |= {tool.prefix(*b) + n for n in names} | {tool.prefix(*b) + n + tool.D64 for n in d64}
    assert set(z.files) == want and len(tool.builds()) == 20
    assert z['relu_256_s_b3_probs'].shape == (3, 32, 50) and z['selu_512_n_b3_enc'].shape == (3, 32, 64)
    assert z['gelu_256_s_single_probs_403'].shape == (1, 100, 50) and z['tanh_256_s_single_probs_67'].shape == (1, 16, 50)
    assert 'tanh_256_s_single_probs_403' not in z.files
    # five different functions of one checkpoint
    for a in range(len(tool.ACTS)):
        for b in range(a):
            assert np.abs(z[f'{tool.ACTS[a]}_256_s_b3_probs'] - z[f'{tool.ACTS[b]}_256_s_b3_probs']).max() > 1e-3
    # the float64 distances are reference errors: above zero, far under the 1e-3 parity bound
    for k in z.files:
        assert z[k].dtype == np.float32 and np.isfinite(z[k]).all(), k
        if k.endswith(tool.D64):
            assert 0 < np.abs(z[k]).max() < 1e-4, k


def test_fixture_equals_its_recipe():
    """the committed file, recomputed from its seeds: through the live reference where it exists, else through
    tests/activation_ref.py (which equals the live reference to the pins' tolerance, test_helper_equals_the_live_reference)"""
    import tempfile
    z = np.load(tool.OUT)
    keep = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    live = shims.reference_available()
    try:
        if live:
            with tempfile.TemporaryDirectory() as tmp:
                got = tool.record(tmp)
        else:
            got = tool.record()
    finally:
        torch.set_num_threads(keep)
    assert sorted(got) == sorted(z.files)
    for k in z.files:
        assert got[k].shape == z[k].shape and got[k].dtype == z[k].dtype, k
        diff = float(np.abs(got[k] - z[k]).max())
        if live:          # the recipe itself, on the kind of machine that recorded the file: the same bits
            assert np.array_equal(got[k], z[k]), (k, diff)
        else:
            # the float32 restatement on whatever CPU, BLAS build and thread count this machine has: float32 matmuls are not
            # bit-stable across those.  Two float32 evaluations of these records sit a few 1e-6 from the float64 one (values up to
            # about 5), so two of them -- and two of their float64 distances -- are within 1e-5 of each other, 100 x under the 1e-3
            # parity bound the file serves
            assert diff < 1e-5, (k, diff)
