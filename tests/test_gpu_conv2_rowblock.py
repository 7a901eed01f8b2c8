"""The offline conv2 (implicit GEMM, N = 256) runs on full-width 64-row blocks with packed weights in registers
(gemm_f32.hip conv2_rows_kernel) wherever launch_gemm would pick 128x128 tiles; masr_debug_set key 40 = 0 selects the 128x128
tiles.  Every output element is the same MFMA chain from zero in both, followed by the same epilogue, so the encoder output and
the CTC probabilities must be BIT-identical with the switch on and off: Conformer, Efficient Conformer and Squeezeformer front-ends,
row counts that are not a multiple of 64, and the Squeezeformer's skipping of row blocks that hold padded frames only (key 38)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F2 = 19     # conv2 output columns for 80 mel bins: ((80 - 1) // 2 - 1) // 2


def _takes_row_blocks(nseq, T):
    # launch_gemm (gemm_f32.hip) runs the 128x128 tiles -- now the row blocks -- above 1 024 tiles, or from 200 tiles on when the
    # last round of 512 workgroups is at least half full (key 33, default 50 %)
    M = nseq * (((T - 1) // 2 - 1) // 2) * F2
    t128 = (M + 127) // 128 * 2
    rounds = (t128 + 511) // 512
    return M, t128 > 1024 or (t128 >= 200 and (t128 - (rounds - 1) * 512) * 100 >= 50 * 512)


def _both(eng, feats, lens, **keys):
    from masr_amd._lib import debug_keys
    out = {}
    for v in (1, 0, 1):
        with debug_keys(eng, conv2_rows=v, **keys):
            enc = eng.encode_full(feats, lens, -1).clone()
            out[v] = (enc, eng.ctc_probs(enc).clone())
    torch.cuda.synchronize()
    return out


def _assert_same(out, valid=None):
    (e1, p1), (e0, p0) = out[1], out[0]
    if valid is not None:
        e1, p1, e0, p0 = (torch.cat([t[i, :n] for i, n in enumerate(valid)]) for t in (e1, p1, e0, p0))
    assert torch.isfinite(e1).all() and float(e1.abs().max()) > 0
    assert torch.equal(e0, e1), (e0 - e1).abs().max().item()
    assert torch.equal(p0, p1), (p0 - p1).abs().max().item()


def _engine(kind):
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sd = getattr(synthetic, kind + '_state_dict')(0, 512)
    return HipEngine(sd, vocab_size=512, use_model=kind, streaming=False)


def _feats(nseq, T, lens, seed):
    gen = torch.Generator().manual_seed(seed)
    feats = torch.randn(nseq, T, 80, generator=gen) * 3 + 13
    lens = torch.tensor(lens, dtype=torch.int32)
    feats = feats * (torch.arange(T)[None, :, None] < lens[:, None, None])
    return feats.cuda(), lens.cuda()


@pytest.mark.parametrize('kind', ['conformer', 'efficient_conformer'])
def test_contract_batch(kind):
    # B = 32 x 10 s of PCM through the feature front-end: M = 32 x 248 x 19 = 150 784 conv2 rows (2 356 row blocks)
    from masr_amd.utils import synthetic
    eng = _engine(kind)
    try:
        rng = np.random.default_rng(3)
        lens = rng.integers(60000, 160001, 32).astype(np.int32)
        lens[0] = 160000
        pcm = synthetic.synthetic_pcm(32, 160000, seed=9)
        for i, l in enumerate(lens):
            pcm[i, l:] = 0
        feats, frames = eng.fbank_batch(torch.from_numpy(pcm).cuda(), torch.from_numpy(lens).cuda())
        assert _takes_row_blocks(32, feats.shape[1])[1]
        _assert_same(_both(eng, feats, frames))
    finally:
        eng.close()


@pytest.mark.parametrize('nseq,T', [(17, 1439), (33, 995)])
def test_ragged_rows(nseq, T):
    # 17 x 1439 frames: M = 115 957 = 1 811 x 64 + 53;  33 x 995: M = 155 496 = 2 429 x 64 + 40 (partial last row block)
    M, taken = _takes_row_blocks(nseq, T)
    assert taken and M % 64 != 0, M
    eng = _engine('conformer')
    try:
        feats, n = _feats(nseq, T, [T - 29 * i for i in range(nseq)], 5)
        out = _both(eng, feats, n)
        assert out[1][0].shape == (nseq, ((T - 1) // 2 - 1) // 2, 256)
        _assert_same(out)
    finally:
        eng.close()


def test_squeezeformer_skipped_padding():
    # lengths from 2.2 to 10 s: whole 64-row blocks of padded frames are skipped (key 38 on, the default) -- only the valid frames
    # are defined then; with key 38 = 0 every frame is computed and the whole output must match
    nseq, T = 32, 1003
    assert _takes_row_blocks(nseq, T)[1]
    eng = _engine('squeezeformer')
    try:
        lens = [T - 25 * i for i in range(nseq)]
        feats, n = _feats(nseq, T, lens, 11)
        valid = eng.enc_frames(np.array(lens))
        _assert_same(_both(eng, feats, n), valid)
        _assert_same(_both(eng, feats, n, skip_padding=0))
    finally:
        eng.close()
