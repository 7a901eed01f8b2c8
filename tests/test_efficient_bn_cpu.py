"""cnn_module_norm: batch_norm for the Efficient Conformer, the parts that need no GPU: configuration checks, the synthetic
checkpoint, the committed fixture against the live reference, and the eval-mode fold of masr_finalize."""
import hashlib
import os

import numpy as np
import pytest
import torch

from masr_amd import _lib
from masr_amd.engine import _validate_encoder_conf
from masr_amd.utils import synthetic

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
# sha256 over (key, dtype, shape, bytes) of synthetic.efficient_conformer_state_dict(0, 16, num_blocks=1), in key order, computed
# at the commit before the cnn_module_norm argument existed
PARENT_DIGEST = '3cf4d6b1f7bbf39fbfc2a8230e76e29d8e5d8cef0001fba7b502382022cb8b87'


def test_validate_accepts_batch_norm_for_the_efficient_conformer():
    _validate_encoder_conf('efficient_conformer', {'cnn_module_norm': 'batch_norm'}, None)
    _validate_encoder_conf('efficient_conformer', {'cnn_module_norm': 'layer_norm'}, None)
    _validate_encoder_conf('efficient_conformer', {}, None)


def test_validate_refuses_an_unknown_norm_by_name():
    with pytest.raises(_lib.MasrError, match='cnn_module_norm'):
        _validate_encoder_conf('efficient_conformer', {'cnn_module_norm': 'group_norm'}, None)


def test_config_and_checkpoint_must_agree():
    ln = synthetic.efficient_conformer_state_dict(0, 16, num_blocks=1)
    bn = synthetic.efficient_conformer_state_dict(0, 16, num_blocks=1, cnn_module_norm='batch_norm')
    with pytest.raises(_lib.MasrError, match='cnn_module_norm'):
        _validate_encoder_conf('efficient_conformer', {'cnn_module_norm': 'batch_norm'}, ln)
    with pytest.raises(_lib.MasrError, match='cnn_module_norm'):
        _validate_encoder_conf('efficient_conformer', {'cnn_module_norm': 'layer_norm'}, bn)
    # a YAML without the key means layer_norm here (the reference's own default for this family is batch_norm): the message of a
    # BatchNorm checkpoint names the key to add
    with pytest.raises(_lib.MasrError, match='holds BatchNorm statistics'):
        _validate_encoder_conf('efficient_conformer', {}, bn)
    _validate_encoder_conf('efficient_conformer', {'cnn_module_norm': 'batch_norm'}, bn)
    _validate_encoder_conf('efficient_conformer', {}, ln)


def _digest(sd):
    h = hashlib.sha256()
    for k in sd:
        a = np.ascontiguousarray(sd[k].numpy())
        h.update(k.encode())
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def test_default_synthetic_checkpoint_is_unchanged():
    assert _digest(synthetic.efficient_conformer_state_dict(0, 16, num_blocks=1)) == PARENT_DIGEST


def test_batch_norm_synthetic_checkpoint_adds_only_the_statistics():
    ln = synthetic.efficient_conformer_state_dict(0, 16, num_blocks=2)
    bn = synthetic.efficient_conformer_state_dict(0, 16, num_blocks=2, cnn_module_norm='batch_norm')
    extra = sorted(set(bn) - set(ln))
    assert extra == sorted(f'encoder.encoders.{i}.conv_module.norm.{n}' for i in range(2)
                           for n in ('running_mean', 'running_var', 'num_batches_tracked'))
    assert all(torch.equal(ln[k], bn[k]) for k in ln)
    for i in range(2):
        p = f'encoder.encoders.{i}.conv_module.norm.'
        assert bn[p + 'running_mean'].abs().max() > 0.1 and (bn[p + 'running_var'] - 1).abs().max() > 0.1      # not the identity
        assert bn[p + 'running_var'].min() > 0


def test_fixture_equals_the_live_reference():
    """pins the committed file to the reference: the B = 3 record, rebuilt the way tools/make_efficient_bn_golden.py builds it"""
    from oracle import shims
    if not shims.reference_available():
        pytest.skip('the reference checkout is not on this machine')
    import tempfile
    from tools import make_efficient_bn_golden as tool
    z = np.load(os.path.join(GOLDEN, 'efficient_bn_v50.npz'))
    keep = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        with tempfile.TemporaryDirectory() as tmp:
            for streaming, k in ((True, 's_'), (False, 'n_')):
                probs, enc = tool.b3_record(tool.model('efficient_conformer', streaming, tmp)[0])
                assert np.array_equal(probs, z[k + 'b3_probs'])
                assert np.array_equal(enc, z[k + 'b3_enc'])
    finally:
        torch.set_num_threads(keep)
    feats, lens = tool.batch32()
    assert np.array_equal(lens, z['b32_lens']) and np.array_equal(feats[0, 0, :8], z['b32_probe'])
    for T, x in tool.single_inputs().items():
        assert np.array_equal(x, z[f'single_feats_{T}'])


def _fold(w, b, mean, var):
    """masr_finalize's fold (engine_conformer.hip finalize_conformer, `if (e->conv_bn)`), float32 throughout: invstd = 1 / sqrtf(var + 1e-5f), scale = w * invstd,
    shift = fmaf(-mean, scale, b) (one rounding: the product of two float32 is exact in float64)"""
    invstd = (np.float32(1) / np.sqrt(var + np.float32(1e-5))).astype(np.float32)
    scale = (w * invstd).astype(np.float32)
    return scale, (b.astype(np.float64) - mean.astype(np.float64) * scale.astype(np.float64)).astype(np.float32)


def _fold_case():
    sd = synthetic.efficient_conformer_state_dict(0, 16, num_blocks=1, cnn_module_norm='batch_norm')
    p = 'encoder.encoders.0.conv_module.norm.'
    w, b, mean, var = (sd[p + k].numpy() for k in ('weight', 'bias', 'running_mean', 'running_var'))
    x = np.random.default_rng(5).standard_normal((4096, 256)).astype(np.float32)
    ref = torch.nn.functional.batch_norm(*(torch.from_numpy(a) for a in (x, mean, var, w, b)), False, 0.0, 1e-5).numpy()
    scale, shift = _fold(w, b, mean, var)
    assert scale.dtype == shift.dtype == np.float32
    return x, scale, shift, ref


def _apply(x, scale, shift):
    """the kernels' y = fmaf(x, scale, shift): one float32 rounding (float32 products and these sums are held by float64)"""
    return (x.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)


def test_fold_is_the_batch_norm():
    """a loose bound of its own (a few float32 roundings of values of magnitude <= 8), with the multiply and the add rounded
    separately: the fold is the eval-mode BatchNorm however the multiply-add is evaluated"""
    x, scale, shift, ref = _fold_case()
    assert np.abs(x * scale + shift - ref).max() < 8 * 2.0 ** -21


def test_fold_within_the_rounding_of_one_multiply_add():
    """the fold applied the way the kernels apply it, as ONE fused multiply-add per element, against
    torch.nn.functional.batch_norm(training=False), element by element within |x * scale| * 2^-23 * 2 + |shift| * 2^-24.  Where
    x * scale is near zero that is half an ulp of the shift: the fold has to produce the reference's own shift, which is why
    masr_finalize takes the reference's steps (scale = w / sqrt(var + eps) with shift = b - mean * scale in two roundings misses
    this bound on 1 % of the elements, and so does a multiply-add in two roundings on 0.07 %)."""
    x, scale, shift, ref = _fold_case()
    y = _apply(x, scale, shift)
    bound = np.abs(x * scale) * np.float32(2.0 ** -23) * 2 + np.abs(shift) * np.float32(2.0 ** -24)
    diff = np.abs(y - ref)
    print(f'fold vs batch_norm: max abs {diff.max():.3e}, over the bound {(diff > bound).sum()} of {diff.size}')
    assert (diff <= bound).all()
