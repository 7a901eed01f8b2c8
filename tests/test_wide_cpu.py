"""output_size 512 / attention_heads 8 for the Conformer, the parts that need no GPU: which (width, heads) pairs the configuration
check and masr_create admit, by name; the committed fixture tests/golden/conformer_wide_v50.npz against its own recipe; and the
256 defaults of the synthetic checkpoints."""
import ctypes
import hashlib
import inspect
import os

import numpy as np
import pytest
import torch

from masr_amd import _lib
from masr_amd.engine import INPUT_LAYERS, _validate_encoder_conf
from masr_amd.utils import synthetic

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
FAMILY = {0: 'conformer', 1: 'squeezeformer', 2: 'efficient_conformer'}
# sha256 over (key, dtype, shape, bytes) of synthetic.conformer_state_dict(0, 16, num_blocks=1), in key order, computed at the
# commit before the 512 / 8 path existed
PARENT_DIGEST = 'd953380d056f0f20d2bbed9d1d97538ff91e358e15703de6c0c8c1dfbb85813e'


def _conf(kind, width, heads, **more):
    return dict({'encoder_dim' if kind == 1 else 'output_size': width, 'attention_heads': heads}, **more)


def _create(kind, width, heads, norm=0, input_layer=0, d_ff=2048):
    """masr_create with the configuration the facade would pass -> (return code, handle value, message)"""
    cfg = _lib.MasrConfig(model_kind=kind, d_model=width, heads=heads, d_ff=d_ff, num_blocks=2, cnn_kernel=31 if kind == 1 else 15,
                          n_mels=80, vocab_size=50, causal=1, max_pos=5000, device_id=0)
    if kind == 0:
        cfg.reserved[0], cfg.reserved[3] = norm, input_layer
    if kind == 1:
        cfg.reserved[0], cfg.reserved[1] = -1, -1
    if kind == 2:
        cfg.reserved[0], cfg.reserved[1], cfg.reserved[2], cfg.reserved[3], cfg.reserved[4] = 3, 4, 3, input_layer, norm
    h = ctypes.c_void_p()
    rc = _lib.lib().masr_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = _lib.lib().masr_last_error().decode()
    if rc == 0:                       # (a machine with a GPU: the engine exists)
        _lib.lib().masr_destroy(h)
    return rc, msg


def test_validate_accepts_256_for_every_family_and_512_for_the_conformer():
    for kind in FAMILY:
        _validate_encoder_conf(FAMILY[kind], _conf(kind, 256, 4), None)
        _validate_encoder_conf(FAMILY[kind], {}, None)
    _validate_encoder_conf('conformer', _conf(0, 512, 8), None)
    _validate_encoder_conf('conformer', _conf(0, 512, 8, linear_units=384, cnn_module_norm='layer_norm', input_layer='conv2d'), None)


@pytest.mark.parametrize('kind,width,heads', [(0, 512, 4), (0, 384, 6), (0, 256, 8), (1, 512, 8), (2, 512, 8), (1, 384, 6)])
def test_validate_refuses_other_widths_by_name(kind, width, heads):
    with pytest.raises(_lib.MasrError) as ei:
        _validate_encoder_conf(FAMILY[kind], _conf(kind, width, heads), None)
    msg = str(ei.value)
    assert ('encoder_dim' if kind == 1 else 'output_size') in msg and 'attention_heads' in msg
    assert '256 / 4' in msg and '512 / 8' in msg and str(width) in msg, msg


def test_validate_refuses_batch_norm_and_other_input_layers_at_512():
    with pytest.raises(_lib.MasrError, match='cnn_module_norm'):
        _validate_encoder_conf('conformer', _conf(0, 512, 8, cnn_module_norm='batch_norm'), None)
    for il in ('conv2d6', 'conv2d8'):
        with pytest.raises(_lib.MasrError, match='input_layer'):
            _validate_encoder_conf('conformer', _conf(0, 512, 8, input_layer=il), None)
    # both stay accepted at 256
    _validate_encoder_conf('conformer', _conf(0, 256, 4, cnn_module_norm='batch_norm', input_layer='conv2d6'), None)


def test_masr_create_gets_past_the_width_check_at_512(built_lib):
    """(512, 8, Conformer) fails only for want of a device here (or succeeds where there is one); (256, 4) likewise"""
    for width, heads in ((512, 8), (256, 4)):
        rc, msg = _create(0, width, heads)
        assert rc == 0 or ('output_size' not in msg and 'specialised' not in msg and 'd_model' not in msg), msg
        if rc:
            assert 'hip' in msg.lower() or 'device' in msg.lower(), msg


@pytest.mark.parametrize('kind,width,heads', [(0, 512, 4), (0, 384, 6), (1, 512, 8), (2, 512, 8)])
def test_masr_create_refuses_other_widths_by_name(built_lib, kind, width, heads):
    rc, msg = _create(kind, width, heads)
    assert rc != 0
    assert 'output_size' in msg and 'attention_heads' in msg and '256 / 4' in msg and '512 / 8' in msg, msg
    assert f'{width} / {heads}' in msg, msg


def test_masr_create_refuses_batch_norm_and_conv2d6_at_512(built_lib):
    rc, msg = _create(0, 512, 8, norm=1)
    assert rc != 0 and 'cnn_module_norm' in msg and 'batch_norm' in msg, msg
    rc, msg = _create(0, 512, 8, input_layer=INPUT_LAYERS['conv2d6'])
    assert rc != 0 and 'input_layer' in msg and 'conv2d' in msg, msg


@pytest.mark.parametrize('d_ff', [0, -128, 2000])
def test_d_ff_keeps_its_rule_at_512(built_lib, d_ff):
    rc, msg = _create(0, 512, 8, d_ff=d_ff)
    assert rc != 0 and 'd_ff' in msg and 'positive multiple of 128' in msg, msg


def test_fixture_equals_its_recipe():
    """the committed file, recomputed from its seeds: through the live reference where it exists, else through oracle.conformer
    with heads = 8 (which equals the live reference bit for bit on the machine that recorded the file)"""
    import tempfile
    from oracle import shims
    from tools import make_wide_golden as tool
    z = np.load(os.path.join(GOLDEN, 'conformer_wide_v50.npz'))
    assert os.path.getsize(tool.OUT) <= tool.LIMIT
    keep = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        if shims.reference_available():
            with tempfile.TemporaryDirectory() as tmp:
                got = tool.record(tmp)
        else:
            got = tool.record()
    finally:
        torch.set_num_threads(keep)
    assert sorted(got) == sorted(z.files)
    live = shims.reference_available()
    for k in z.files:
        assert got[k].shape == z[k].shape and got[k].dtype == z[k].dtype, k
        diff = float(np.abs(got[k] - z[k]).max())
        if live:          # the recipe itself, on the kind of machine that recorded the file: the same bits
            assert np.array_equal(got[k], z[k]), (k, diff)
        else:
            # the float32 oracle on whatever CPU, BLAS build and thread count this machine has: float32 matmuls are not bit-stable
            # across those.  Two float32 evaluations of these records sit 2e-6 to 3e-6 from the float64 one (values up to 4.8), so
            # two of them are within 1e-5 of each other, 100 x under the 1e-3 parity bound the file serves
            assert diff < 1e-5, (k, diff)
    assert z['s_chunk_att_-1'].shape == (2, 8, 48, 128) and z['s_chunk_att_16'].shape == (2, 8, 16, 128)
    assert z['s_chunk_cnn_-1'].shape == (2, 1, 512, 14)


def _digest(sd):
    h = hashlib.sha256()
    for k in sd:
        a = np.ascontiguousarray(sd[k].numpy())
        h.update(k.encode())
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def test_synthetic_defaults_are_unchanged():
    for fn in (synthetic.conformer_state_dict, synthetic.squeezeformer_state_dict, synthetic.efficient_conformer_state_dict):
        p = inspect.signature(fn).parameters
        assert p['d'].default == 256 and p['heads'].default == 4
    sd = synthetic.conformer_state_dict(0, 16, num_blocks=1)
    assert _digest(sd) == PARENT_DIGEST
    assert sd['encoder.encoders.0.self_attn.pos_bias_u'].shape == (4, 64) and sd['encoder.after_norm.weight'].shape == (256,)
    wide = synthetic.conformer_state_dict(0, 16, d=512, heads=8, num_blocks=1)
    assert wide['encoder.encoders.0.self_attn.pos_bias_u'].shape == (8, 64) and wide['encoder.after_norm.weight'].shape == (512,)
