"""GPU: masr_rescore_rows -- the second pass over encoder frames read through a row table (the A_ROWS operand of the tiled f32 GEMM,
csrc/gemm_f32.hip) -- against masr_rescore on the gathered dense copy, bit for bit, and against the float64 restatement
(tests/rescoring_ref.py) under the budget rule of tests/budget.py (C = 8, as tests/test_gpu_rescoring.py has it).

The synthetic model of tests/test_gpu_rescoring.py: V = 50, d = 256 / 4 heads, decoder 2 + 2 blocks, linear_units 384."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import budget            # noqa: E402
import rescoring_ref as rr            # noqa: E402
from test_gpu_rescoring import DEC_CONF, ENC_CONF, V, _fixture, _sd            # noqa: E402

pytestmark = pytest.mark.gpu

D = 256


@pytest.fixture(scope='module')
def fx():
    return _fixture()


@pytest.fixture(scope='module')
def sd():
    return _sd()


@pytest.fixture(scope='module')
def eng(sd):
    from masr_amd.engine import HipEngine
    e = HipEngine(sd, encoder_conf=ENC_CONF, vocab_size=V, attention_decoder=True, decoder_conf=DEC_CONF)
    yield e
    e.close()


def _dev(eng, a):
    return torch.as_tensor(a).to(eng.device)


def _gathered(pool, table, frames):
    """the dense block [B, Tmax, d] of a row table: rows[frame_row] for the valid frames (a number outside the pool: a zero row),
    zeros behind them"""
    table = np.asarray(table, np.int64)
    B, Tmax = table.shape
    valid = (np.arange(Tmax)[None, :] < np.asarray(frames)[:, None]) & (table >= 0) & (table < pool.shape[0])
    dense = torch.zeros(B, Tmax, pool.shape[1], dtype=torch.float32, device=pool.device)
    dense[torch.from_numpy(valid).to(pool.device)] = pool[torch.from_numpy(table[valid]).to(pool.device)]
    return dense


def _both(eng, pool, table, frames, hyps, lens, with_right=True):
    """(masr_rescore_rows through the table, masr_rescore on the gathered copy), each (att, r_att) as numpy"""
    fr, h, l = _dev(eng, np.asarray(frames, np.int32)), _dev(eng, hyps), _dev(eng, lens)
    rows = eng.rescore_rows(pool, _dev(eng, np.asarray(table, np.int64)), fr, h, l, with_right)
    dense = eng.rescore(_gathered(pool, table, frames), fr, h, l, with_right)
    return [a.cpu().numpy() for a in rows], [a.cpu().numpy() for a in dense]


def _ragged_case(n_rows=120, seed=11):
    """B = 3 with frames [33, 16, 1], Tmax = 33 (M = 99: one full 64-row tile and a ragged one): rows from a pool in shuffled, partly
    descending order, pool row 7 shared by utterances 0 and 1, the entries behind the valid frames -1, n_rows and 2^40"""
    rng = np.random.default_rng(seed)
    frames = np.array([33, 16, 1], np.int32)
    perm = rng.permutation(n_rows)
    table = np.full((3, 33), -1, np.int64)
    table[0] = perm[:33]
    table[0, 10:20] = np.sort(table[0, 10:20])[::-1]          # a descending run
    table[1, :16] = perm[40:56]
    table[0, 4] = table[1, 9] = 7                              # one pool row, two utterances
    table[1, 16:] = n_rows                                     # padding: one past the pool,
    table[2, 0] = perm[60]
    table[2, 1:17] = 1 << 40                                   # far outside,
    table[2, 17:] = -1                                         # and the -1 of the pool's own tables
    return frames, table


def test_bit_equal_to_rescore_on_the_gathered_copy(fx, eng):
    """both decoders and with_right = 0; N = 4 with hypothesis lengths {0, 1, 15, 17} (the table of rescoring_v50.npz)"""
    assert sorted(fx['hyp_lens'][0].tolist()) == [0, 1, 15, 17] and fx['hyps'].shape[:2] == (3, 4)
    frames, table = _ragged_case()
    pool = torch.randn(120, D, generator=torch.Generator().manual_seed(5)).to(eng.device)
    for with_right in (True, False):
        rows, dense = _both(eng, pool, table, frames, fx['hyps'], fx['hyp_lens'], with_right)
        assert np.array_equal(rows[0], dense[0]) and np.array_equal(rows[1], dense[1]), with_right
        assert np.isfinite(rows[0]).all() and (rows[1].any() if with_right else not rows[1].any())
    # the padding is never used: other numbers behind the valid frames, the same bits
    other = table.copy()
    other[1, 16:], other[2, 1:] = 3, 0
    again, _ = _both(eng, pool, other, frames, fx['hyps'], fx['hyp_lens'])
    rows, _ = _both(eng, pool, table, frames, fx['hyps'], fx['hyp_lens'])
    assert np.array_equal(again[0], rows[0]) and np.array_equal(again[1], rows[1])


def _tile(M, N):
    """the tile launch_gemm takes for a row-major EPI_STD launch (std_tiles, csrc/gemm_f32.hip)"""
    t128 = -(-M // 128) * -(-N // 128)
    t64 = -(-M // 64) * -(-N // 128)
    return (128, 128) if t128 >= 384 else (64, 128) if t64 >= 200 else (64, 64)


# the source projection is (M, 2 d, d) = (M, 512, 256): 64x64 tiles up to M = 3136, 64x128 from 3137, 128x128 from 12161
@pytest.mark.parametrize('M,tile', [(3136, (64, 64)), (3137, (64, 128)), (12160, (64, 128)), (12161, (128, 128))])
def test_every_tile_shape_of_the_projection(eng, M, tile):
    """one utterance of M frames, N = 1, Lmax = 2: only the projection is large; the rows come from a pool half as large again, in
    a shuffled order"""
    assert _tile(M, 2 * D) == tile and _tile(99, 2 * D) == (64, 64)
    rng = np.random.default_rng(M)
    n_rows = M + M // 2
    pool = torch.randn(n_rows, D, generator=torch.Generator().manual_seed(M)).to(eng.device)
    table = rng.permutation(n_rows)[:M].astype(np.int64)[None, :]
    hyps, lens = np.array([[[3, 7]]], np.int32), np.array([[2]], np.int32)
    rows, dense = _both(eng, pool, table, [M], hyps, lens)
    assert np.array_equal(rows[0], dense[0]) and np.array_equal(rows[1], dense[1])
    assert np.isfinite(rows[0]).all() and np.isfinite(rows[1]).all()


def test_a_row_outside_the_pool_among_the_valid_frames_is_a_zero_row(fx, eng):
    frames, table = _ragged_case()
    table[0, 5], table[0, 32], table[1, 3] = -1, 1 << 40, 120
    pool = torch.randn(120, D, generator=torch.Generator().manual_seed(6)).to(eng.device)
    dense_block = _gathered(pool, table, frames)
    assert not dense_block[0, 5].any() and not dense_block[0, 32].any() and not dense_block[1, 3].any() and dense_block[0, 6].any()
    rows, dense = _both(eng, pool, table, frames, fx['hyps'], fx['hyp_lens'])
    assert np.array_equal(rows[0], dense[0]) and np.array_equal(rows[1], dense[1])
    clean, _ = _both(eng, pool, _ragged_case()[1], frames, fx['hyps'], fx['hyp_lens'])
    assert not np.array_equal(clean[0][:2], rows[0][:2])       # (the zero rows are seen: utterances 0 and 1 score differently)


def test_rows_beyond_two_gib_of_pool(fx, eng):
    """a pool of 2^21 + 64 rows (more than 2^31 bytes at d = 256, never filled): the frames lie in its last 64 rows"""
    n_rows = (1 << 21) + 64
    pool = torch.empty(n_rows, D, dtype=torch.float32, device=eng.device)
    assert pool.numel() * 4 > 1 << 31
    last = torch.randn(64, D, generator=torch.Generator().manual_seed(7)).to(eng.device)
    pool[n_rows - 64:] = last
    rng = np.random.default_rng(8)
    frames = np.array([33, 16, 1], np.int32)
    table = np.full((3, 33), -1, np.int64)
    for b in range(3):
        table[b, :frames[b]] = n_rows - 64 + rng.permutation(64)[:frames[b]]
    fr, h, l = _dev(eng, frames), _dev(eng, fx['hyps']), _dev(eng, fx['hyp_lens'])
    rows = eng.rescore_rows(pool, _dev(eng, table), fr, h, l)
    local = np.where(table >= 0, table - (n_rows - 64), -1)
    dense = eng.rescore(_gathered(last, local, frames), fr, h, l)
    assert torch.equal(rows[0], dense[0]) and torch.equal(rows[1], dense[1])
    del pool


def test_float64_budget_on_the_gathered_memory(fx, sd, eng):
    frames, table = _ragged_case()
    pool = torch.randn(120, D, generator=torch.Generator().manual_seed(5)).to(eng.device)
    memory = _gathered(pool, table, frames).cpu().numpy()
    a64 = rr.scores(rr.to64(sd), memory, frames, fx['hyps'], fx['hyp_lens'])
    a32 = rr.scores(sd, memory, frames, fx['hyps'], fx['hyp_lens'])
    rows, _ = _both(eng, pool, table, frames, fx['hyps'], fx['hyp_lens'])
    budget.check('rescore_rows att', a64[0], a32[0], rows[0])
    budget.check('rescore_rows r_att', a64[1], a32[1], rows[1])


def test_refusals_by_name(fx, sd, eng):
    from masr_amd._lib import MasrError
    from masr_amd.engine import HipEngine
    pool = torch.zeros(8, D, device=eng.device)
    table = torch.zeros(1, 4, dtype=torch.int64, device=eng.device)
    frames = torch.full((1,), 4, dtype=torch.int32, device=eng.device)
    hyps, lens = torch.ones(1, 1, 2, dtype=torch.int32, device=eng.device), torch.ones(1, 1, dtype=torch.int32, device=eng.device)
    with pytest.raises(MasrError, match='masr_rescore_rows: n_rows = 0'):
        eng.rescore_rows(pool[:0], table, frames, hyps, lens)
    with pytest.raises(MasrError, match='masr_rescore_rows: Tmax = 0'):
        eng.rescore_rows(pool, table[:, :0].contiguous(), frames, hyps, lens)
    with pytest.raises(MasrError, match='masr_rescore_rows: N = 65 .* outside 1 .. 64'):
        eng.rescore_rows(pool, table, frames, torch.ones(1, 65, 2, dtype=torch.int32, device=eng.device),
                         torch.ones(1, 65, dtype=torch.int32, device=eng.device))
    plain = HipEngine(sd, encoder_conf=ENC_CONF, vocab_size=V)
    try:
        with pytest.raises(MasrError, match='masr_rescore_rows: this engine holds no attention decoder'):
            plain.rescore_rows(pool, table, frames, hyps, lens)
    finally:
        plain.close()
