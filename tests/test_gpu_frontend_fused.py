"""The offline front end on the row-block kernel (gemm_f32.hip conv2_rows_kernel): conv1 computed inside the conv2 A gather
(masr_debug_set key 41; 0 = conv1_kernel writes its output to a workspace first) and the embed projection's four K quarters on
full-width 64-row blocks (key 42; 0 = 128x128 tiles).  Every conv1 value is the same fmaf chain, every conv2 / embed output
element the same MFMA chain, followed by the same epilogue or split-K reduction, so the encoder output and the CTC probabilities
must be BIT-identical with the switches on and off: Conformer and Efficient Conformer on the contract batch, row counts that are
not a multiple of 64 with blocks across sequence boundaries, and the Squeezeformer with and without skipping row blocks of padded
frames (key 38)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F2 = 19     # conv2 output columns for 80 mel bins: ((80 - 1) // 2 - 1) // 2
SETTINGS = ((1, 1), (0, 0), (1, 0), (0, 1), (1, 1))     # (key 41, key 42)


def _takes_row_blocks(nseq, T):
    # launch_gemm (gemm_f32.hip) runs the row blocks above 1 024 tiles of 128x128, or from 200 tiles on when the last round of
    # 512 workgroups is at least half full (key 33, default 50 %); only there is conv1 fused
    M = nseq * (((T - 1) // 2 - 1) // 2) * F2
    t128 = (M + 127) // 128 * 2
    rounds = (t128 + 511) // 512
    return M, t128 > 1024 or (t128 >= 200 and (t128 - (rounds - 1) * 512) * 100 >= 50 * 512)


def _all(eng, feats, lens, **keys):
    from masr_amd._lib import debug_keys
    out = []
    for k41, k42 in SETTINGS:
        with debug_keys(eng, conv1_fused=k41, embed_rows=k42, **keys):
            enc = eng.encode_full(feats, lens, -1).clone()
            out.append((enc, eng.ctc_probs(enc).clone()))
    torch.cuda.synchronize()
    return out


def _assert_same(out, valid=None):
    if valid is not None:
        out = [tuple(torch.cat([t[i, :n] for i, n in enumerate(valid)]) for t in pair) for pair in out]
    e1, p1 = out[0]
    assert torch.isfinite(e1).all() and float(e1.abs().max()) > 0
    for e0, p0 in out[1:]:
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
    # B = 32 x 10 s of PCM through the feature front-end: 2 356 conv2 row blocks, 124 x 4 embed projection blocks
    from masr_amd.utils import synthetic
    eng = _engine(kind)
    try:
        rng = np.random.default_rng(4)
        lens = rng.integers(60000, 160001, 32).astype(np.int32)
        lens[0] = 160000
        pcm = synthetic.synthetic_pcm(32, 160000, seed=13)
        for i, l in enumerate(lens):
            pcm[i, l:] = 0
        feats, frames = eng.fbank_batch(torch.from_numpy(pcm).cuda(), torch.from_numpy(lens).cuda())
        assert _takes_row_blocks(32, feats.shape[1])[1]
        _assert_same(_all(eng, feats, frames))
    finally:
        eng.close()


@pytest.mark.parametrize('nseq,T', [(17, 1439), (33, 995)])
def test_ragged_rows(nseq, T):
    # 17 x 1439 frames: M = 115 957 = 1 811 x 64 + 53;  33 x 995: M = 155 496 = 2 429 x 64 + 40 (partial last row block); a
    # sequence holds 359 x 19 or 247 x 19 rows, so most blocks straddle two (t2) groups and many two sequences
    M, taken = _takes_row_blocks(nseq, T)
    assert taken and M % 64 != 0, M
    eng = _engine('conformer')
    try:
        feats, n = _feats(nseq, T, [T - 29 * i for i in range(nseq)], 6)
        out = _all(eng, feats, n)
        assert out[0][0].shape == (nseq, ((T - 1) // 2 - 1) // 2, 256)
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
        feats, n = _feats(nseq, T, lens, 12)
        valid = eng.enc_frames(np.array(lens))
        _assert_same(_all(eng, feats, n), valid)
        _assert_same(_all(eng, feats, n, skip_padding=0))
    finally:
        eng.close()
