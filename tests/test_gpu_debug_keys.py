"""The masr_debug_set switches ARRIVE: a bit-identity test of a switch also passes when the switch reaches nothing, so this one counts
launches (masr_profile_select / masr_profile_read; no timing) with the switches set by name through _lib.debug_keys.

Offline Conformer, d_model 256, two blocks; 3 utterances of 403 / 371 / 290 feature frames -> T' = 100, M = 300 rows = 10 row blocks
of 32: the sequence boundaries (rows 100, 200) fall inside row blocks and the last block holds 12 rows.  By default such a batch runs
the d_ff-split FFN launches (10 < ffn_split_blocks = 192), which carry neither stage; with ffn_split_blocks = 0 every layer runs
one full-d_ff launch with the QKV tail stage (profile kind 6) and one with the conv-module head stage (kind 7): by ffn() and
encode_full_conformer in engine_conformer.hip, one launch of each kind per block with ffn_split_blocks = 0 and none without.  few_rows_path needs
no change: the few-rows layer path is taken below min(rowgemm_small_blocks, ffn_split_blocks) row blocks, which is 0 here."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FFN_TAIL, FFN_HEAD = 6, 7     # masr_profile_select kinds


@pytest.fixture(scope='module')
def setup():
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sd = synthetic.conformer_state_dict(0, 512, num_blocks=2)
    engines = [HipEngine(sd, encoder_conf={'num_blocks': 2}, vocab_size=512, streaming=False) for _ in range(2)]
    T, lens = 403, torch.tensor([403, 371, 290], dtype=torch.int32)
    feats = torch.randn(3, T, 80, generator=torch.Generator().manual_seed(7)) * 3 + 13
    feats = feats * (torch.arange(T)[None, :, None] < lens[:, None, None])
    yield engines, feats.cuda(), lens.cuda()
    for e in engines:
        e.close()


def _launches(eng, kind, feats, lens):
    """(launches of `kind` in one encoder pass, encoder output)"""
    eng.profile_select(kind)
    try:
        eng.profile_read(True)
        out = eng.encode_full(feats, lens, -1).clone()
        torch.cuda.synchronize()
        return eng.profile_read(True)[1], out
    finally:
        eng.profile_select(0)


def test_switches_reach_the_launchers_and_reset_restores_the_defaults(setup):
    from masr_amd._lib import debug_keys
    (eng, _), feats, lens = setup
    n0, before = _launches(eng, FFN_TAIL, feats, lens)
    assert before.shape == (3, 100, 256) and torch.isfinite(before).all()
    assert n0 == 0 and _launches(eng, FFN_HEAD, feats, lens)[0] == 0            # the defaults: d_ff-split launches
    with debug_keys(eng, ffn_split_blocks=0):
        tail, _ = _launches(eng, FFN_TAIL, feats, lens)
        head, _ = _launches(eng, FFN_HEAD, feats, lens)
        print(f'ffn_split_blocks = 0: {tail} launches with the tail stage, {head} with the head stage')
        assert tail > 0 and head > 0
    with debug_keys(eng, ffn_split_blocks=0, no_ffn_tail=1):
        assert _launches(eng, FFN_TAIL, feats, lens)[0] == 0
    with debug_keys(eng, {'ffn_split_blocks': 0, 'no_ffn_head': 1}):
        assert _launches(eng, FFN_HEAD, feats, lens)[0] == 0
    # behind the block nothing is set: ffn_split_blocks is back at 192, the batch runs split, and computes what it did before
    n1, after = _launches(eng, FFN_TAIL, feats, lens)
    assert n1 == 0
    assert torch.equal(after, before)


def test_a_switch_holds_for_every_engine_of_the_process(setup):
    from masr_amd._lib import debug_keys
    (first, second), feats, lens = setup
    assert _launches(second, FFN_TAIL, feats, lens)[0] == 0
    with debug_keys(first, ffn_split_blocks=0):
        assert _launches(second, FFN_TAIL, feats, lens)[0] > 0
    assert _launches(second, FFN_TAIL, feats, lens)[0] == 0


def test_refused_and_unknown_keys_raise(setup):
    from masr_amd import build
    from masr_amd._lib import MasrError, debug_keys
    (eng, _), _, _ = setup
    for keys in ({'no_such_switch': 1}, {3: 1}, {44: 1}) + (() if build.has_experiments() else ({'ffn_dual': 1},)):
        with pytest.raises(MasrError):
            with debug_keys(eng, keys):
                pass
