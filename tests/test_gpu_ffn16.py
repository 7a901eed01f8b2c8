"""The full-d_ff FFN launches run the 16-row kernel (ffn_pc.hip ffn16_kernel, two workgroups per CU) by default; masr_debug_set
key 39 = 0 selects the 32-row kernel.  Every dot product is the same fmaf chain in both (tests/test_gpu_mfma_order.py), so the
encoder output and the CTC probabilities must be BIT-identical with the switch on and off -- for the QKV tail and the conv-module
head (offline Conformer, streaming True and False), the Efficient Conformer (planar QKV tail), ragged batches whose last 16-row
block is partial and whose sequences start inside blocks, and M on both sides of the cut-overs of ffn() in engine_layers.hip.

Full launches (nsplit = 1) need >= 129 32-row blocks: below that ffn() splits d_ff (nsplit = min(d_ff / 128, 256 / blocks) > 1).
The conv-module head rides on the FFN launch from ffn_split_blocks = 192 blocks (masr_debug_set key 13) on."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _both(eng, feats, lens, **keys):
    from masr_amd._lib import debug_keys
    out = {}
    for v in (1, 0, 1):
        with debug_keys(eng, ffn16=v, **keys):
            enc = eng.encode_full(feats, lens, -1).clone()
            out[v] = (enc, eng.ctc_probs(enc).clone())
    torch.cuda.synchronize()
    return out


def _assert_same(out):
    (e1, p1), (e0, p0) = out[1], out[0]
    assert torch.isfinite(e1).all() and float(e1.abs().max()) > 0
    assert torch.equal(e0, e1), (e0 - e1).abs().max().item()
    assert torch.equal(p0, p1), (p0 - p1).abs().max().item()


@pytest.mark.parametrize('kind,streaming', [('conformer', True), ('conformer', False), ('efficient_conformer', True)])
def test_16_row_kernel_is_bit_identical_to_32_row_kernel(kind, streaming):
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    V = 512
    sd = getattr(synthetic, kind + '_state_dict')(0, V)
    eng = HipEngine(sd, vocab_size=V, use_model=kind, streaming=streaming)
    try:
        rng = np.random.default_rng(3)
        lens = rng.integers(60000, 160001, 32).astype(np.int32)
        pcm = synthetic.synthetic_pcm(32, 160000, seed=9)
        for i, l in enumerate(lens):
            pcm[i, l:] = 0
        feats, frames = eng.fbank_batch(torch.from_numpy(pcm).cuda(), torch.from_numpy(lens).cuda())
        _assert_same(_both(eng, feats, frames))
    finally:
        eng.close()


def _feats(nseq, T, lens, seed):
    gen = torch.Generator().manual_seed(seed)
    feats = torch.randn(nseq, T, 80, generator=gen) * 3 + 13
    lens = torch.tensor(lens, dtype=torch.int32)
    feats = feats * (torch.arange(T)[None, :, None] < lens[:, None, None])
    return feats.cuda(), lens.cuda()


def _assert_reaches(M, blocks_from=129):
    assert (M + 31) // 32 >= blocks_from and M % 16 != 0, M


@pytest.mark.parametrize('streaming', [True, False])
def test_ragged_batch_with_partial_blocks(streaming):
    # 9 x 1003 frames -> T' = 250, M = 2250 = 71 32-row blocks: d_ff-split launches by default, so the cut-over is moved out of the
    # way (key 13 = 0: full launches with the QKV tail and the conv-module head).  2250 = 140 x 16 + 10: the last 16-row block is
    # partial; sequences start inside 16-row blocks (250 = 15 x 16 + 10)
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sd = synthetic.conformer_state_dict(0, 512)
    eng = HipEngine(sd, vocab_size=512, streaming=streaming)
    try:
        feats, lens = _feats(9, 1003, [1003, 990, 700, 1003, 512, 333, 1003, 801, 67], 21)
        out = _both(eng, feats, lens, ffn_split_blocks=0)
        assert out[1][0].shape == (9, 250, 256)
        _assert_same(out)
    finally:
        eng.close()


@pytest.mark.parametrize('nseq,T', [(17, 963), (17, 971), (17, 1439), (17, 1447), (33, 995)])
def test_around_the_cut_overs(nseq, T):
    # default cut-overs, 17 sequences (M % 16 != 0 on the full side: partial last block, sequences starting inside blocks):
    #   T = 963  -> T' = 240, M = 4080 = 128 blocks: d_ff split          T = 971  -> T' = 242, M = 4114 = 129 blocks: full, 16-row
    #   T = 1439 -> T' = 359, M = 6103 = 191 blocks: full, head separate  T = 1447 -> T' = 361, M = 6137 = 192 blocks: head fused
    # and 33 x 10 s (T' = 248, M = 8184 = 511 x 16 + 8): a real batch size with a partial last 16-row block
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sd = synthetic.conformer_state_dict(0, 512)
    eng = HipEngine(sd, vocab_size=512, streaming=False)
    try:
        lens = [T - 23 * i for i in range(nseq)]
        feats, n = _feats(nseq, T, lens, 5)
        Tq = (T - 3) // 4
        if T != 963:
            _assert_reaches(nseq * Tq)
        out = _both(eng, feats, n)
        assert out[1][0].shape == (nseq, Tq, 256)
        _assert_same(out)
    finally:
        eng.close()
