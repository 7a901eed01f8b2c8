"""encoder_conf.cnn_module_kernel off the shipped values, the parts that need no GPU: what the configuration check and masr_create
accept and refuse, by name; the checkpoint's own tap count against the config; the FFN launch plan (unchanged for head stages of
15 / 7 taps, no fused head for any other count); the committed fixture tests/golden/conv_kernel_v50.npz against its own recipe;
and oracle.squeezeformer.get_encoder_out_chunk at other kernel sizes against the live reference."""
import ctypes
import os

import numpy as np
import pytest
import torch

from masr_amd import _lib
from masr_amd.engine import _validate_encoder_conf
from masr_amd.utils import synthetic
from oracle import shims
from tests import ffn_plan as model

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
KEY = 'encoder.encoders.0.conv_module.depthwise_conv.weight'


def _create(kind, kernel, causal=1):
    """masr_create with the configuration the facade would pass -> (return code, message)"""
    cfg = _lib.MasrConfig(model_kind=kind, d_model=256, heads=4, d_ff=2048, num_blocks=2, cnn_kernel=kernel, n_mels=80, vocab_size=50,
                          causal=causal, max_pos=5000, device_id=0)
    if kind == 1:
        cfg.reserved[0], cfg.reserved[1] = -1, -1
    if kind == 2:                     # (two blocks: the stride layer is the last one and both are grouped, as in the shipped layout)
        cfg.reserved[0], cfg.reserved[1], cfg.reserved[2] = 1, 2, 3
    h = ctypes.c_void_p()
    rc = _lib.lib().masr_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = _lib.lib().masr_last_error().decode()
    if rc == 0:                       # (a machine with a GPU: the engine exists)
        _lib.lib().masr_destroy(h)
    return rc, msg


def test_validate_accepts_the_range_by_build():
    for k in (31, 9, 3):
        _validate_encoder_conf('conformer', {'cnn_module_kernel': k}, None, streaming=False)
    for k in (8, 31):
        _validate_encoder_conf('conformer', {'cnn_module_kernel': k}, None, streaming=True)
    _validate_encoder_conf('squeezeformer', {'cnn_module_kernel': 15}, None, streaming=False)
    _validate_encoder_conf('squeezeformer', {'cnn_module_kernel': 7}, None, streaming=False)
    _validate_encoder_conf('squeezeformer', {'cnn_module_kernel': 8}, None, streaming=True)
    # the build not known: the parity check is skipped; the old three-argument call keeps working
    _validate_encoder_conf('conformer', {'cnn_module_kernel': 8}, None)
    _validate_encoder_conf('efficient_conformer', {'cnn_module_kernel': 15}, None, streaming=True)


@pytest.mark.parametrize('family,k,streaming', [('conformer', 2, True), ('conformer', 33, True), ('conformer', 15.0, True),
                                                ('conformer', '15', True), ('conformer', 8, False), ('conformer', 30, False),
                                                ('squeezeformer', 2, True), ('squeezeformer', 33, False), ('squeezeformer', 8, False),
                                                ('squeezeformer', 31.0, False), ('efficient_conformer', 31, True)])
def test_validate_refuses_by_name(family, k, streaming):
    with pytest.raises(_lib.MasrError) as ei:
        _validate_encoder_conf(family, {'cnn_module_kernel': k}, None, streaming=streaming)
    msg = str(ei.value)
    assert 'cnn_module_kernel' in msg and repr(k) in msg, msg
    assert ('15' if family == 'efficient_conformer' else '3 to 31') in msg, msg


@pytest.mark.parametrize('family', ['conformer', 'squeezeformer'])
def test_checkpoint_and_config_must_agree(family):
    make = synthetic.conformer_state_dict if family == 'conformer' else synthetic.squeezeformer_state_dict
    for have, conf in ((31, 15), (15, 31)):
        sd = make(0, 16, num_blocks=1, kernel=have)
        _validate_encoder_conf(family, {'cnn_module_kernel': have}, sd, streaming=True)
        with pytest.raises(_lib.MasrError) as ei:
            _validate_encoder_conf(family, {'cnn_module_kernel': conf}, sd, streaming=True)
        msg = str(ei.value)
        assert 'cnn_module_kernel' in msg and KEY in msg and str(have) in msg and str(conf) in msg, msg


@pytest.mark.parametrize('kind,kernel,causal', [(0, 31, 1), (0, 8, 1), (0, 31, 0), (0, 3, 0), (1, 15, 1), (1, 15, 0), (1, 8, 1), (2, 15, 1)])
def test_masr_create_gets_past_the_kernel_check(built_lib, kind, kernel, causal):
    """fails only for want of a device here (or succeeds where there is one)"""
    rc, msg = _create(kind, kernel, causal)
    assert rc == 0 or 'cnn_module_kernel' not in msg, msg
    if rc:
        assert 'hip' in msg.lower() or 'device' in msg.lower(), msg


@pytest.mark.parametrize('kind,kernel,causal', [(0, 33, 1), (0, 2, 1), (1, 33, 1), (1, 2, 0), (0, 8, 0), (1, 8, 0), (0, 30, 0), (2, 31, 1),
                                                (2, 7, 1)])
def test_masr_create_refuses_by_name(built_lib, kind, kernel, causal):
    rc, msg = _create(kind, kernel, causal)
    assert rc != 0
    assert 'cnn_module_kernel' in msg and str(kernel) in msg, msg
    assert ('15 only' if kind == 2 else '[3, 31]') in msg, msg


@pytest.mark.parametrize('M', [16, 256, 8192])
def test_plan_is_unchanged_for_15_and_7_and_declines_other_heads(built_lib, M):
    for d_ff in (2048, 384):
        nsplit, cpb, ny = model.plan(d_ff, M)
        for taps in (15, 7):
            for norm in (0, 1):
                p = _lib.ffn_plan(d_ff, M, head_ktaps=taps, head_norm=norm)
                assert (p.nsplit, p.cpb, p.ny) == (nsplit, cpb, ny)
                # ffn_plan.h: the head rides on the full launch of either count; on the d_ff-split launch only with masr_debug_set
                # key 30 (split_head, off by default), and then at 15 taps only
                assert p.head_in_kernel == (1 if nsplit == 1 else 0) and p.split_head == 0, (taps, norm, p)
                assert p.prof == (7 if p.head_in_kernel else 2)
                assert p.kernel == ('ROWS16' if nsplit == 1 else 'PC')
            if nsplit > 1:
                p = _lib.ffn_plan(d_ff, M, {30: 1}, head_ktaps=taps)
                assert p.split_head == p.head_in_kernel == (1 if taps == 15 else 0), (taps, p)
        for taps in (9, 31, 8, 3):
            for keys in (None, {30: 1}):
                p = _lib.ffn_plan(d_ff, M, keys, head_ktaps=taps)
                assert (p.nsplit, p.cpb, p.ny) == (nsplit, cpb, ny)
                assert p.head_in_kernel == 0 and p.split_head == 0 and p.prof == 2, (taps, p)
                assert p.kernel == _lib.ffn_plan(d_ff, M, keys).kernel


def test_fixture_equals_its_recipe():
    """the committed file, recomputed from its seeds: through the live reference where it exists, else through the oracle (which
    the issue's runs and test_oracle_golden.py hold to the live reference)"""
    import tempfile
    from tools import make_conv_kernel_golden as tool
    z = np.load(os.path.join(GOLDEN, 'conv_kernel_v50.npz'))
    assert os.path.getsize(tool.OUT) <= tool.LIMIT
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
    assert sorted(got) == sorted(z.files)
    for k in z.files:
        assert got[k].shape == z[k].shape and got[k].dtype == z[k].dtype, k
        diff = float(np.abs(got[k] - z[k]).max())
        if live:          # the recipe itself, on the kind of machine that recorded the file: the same bits
            assert np.array_equal(got[k], z[k]), (k, diff)
        else:
            # two float32 evaluations of probabilities and normalised cache rows (values up to ~5) on different CPUs / BLAS builds:
            # each sits a few 1e-6 from the float64 one, so they are within 1e-5 of each other, 100 x under the 1e-3 parity bound
            # the file serves (the rule of test_wide_cpu.py)
            assert diff < 1e-5, (k, diff)
    assert z['c8_chunk_cnn_16'].shape == (2, 1, 256, 7) and z['c8_chunk_att_16'].shape == (2, 4, 16, 128)
    assert z['q8_chunk_cnn_-1'].shape == (4, 1, 256, 7)


@pytest.mark.skipif(not shims.reference_available(), reason='the reference checkout is not present')
@pytest.mark.parametrize('K', [15, 8])
def test_squeezeformer_chunk_oracle_matches_the_live_reference(K):
    import tempfile
    from oracle import squeezeformer as osq
    from tools import make_conv_kernel_golden as tool
    sd = tool.squeezeformer_sd(K, True)
    x = tool.single_inputs()[403]
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        m = tool.squeezeformer_model(K, True, tmp)
        ra, rc, oa, oc = (torch.zeros(0, 0, 0, 0) for _ in range(4))
        off = 0
        for cur, n in tool.CHUNKS:
            rp, ra, rc = m.get_encoder_out_chunk(x[:1, cur:cur + n], off, -1, ra, rc)
            op, oa, oc = osq.get_encoder_out_chunk(sd, x[:1, cur:cur + n], off, -1, oa, oc, kernel=K, **tool.SQZ_IDX)
            off += rp.shape[1]
            assert rp.shape == op.shape and ra.shape == oa.shape and rc.shape == oc.shape == (4, 1, 256, K - 1)
            # (float32 restatement against the modules: the bound of test_oracle_golden.py's live comparisons)
            assert (rp - op).abs().max() < 2e-5 and (ra - oa).abs().max() < 2e-5 and (rc - oc).abs().max() < 2e-5, (K, cur)
