"""The activation epilogue of the tiled GEMM (gemm_f32.hip) alone, through masr_op_gemm: act 3 gelu, 4 tanh, 5 hardtanh, 6 selu,
and again 0 none, 1 relu, 2 silu.

Shapes: M in {1, 33, 130}, N in {64, 384}, K in {32, 256} -- partial row and column tiles, one K slab and several.  The inputs put
chosen values in front of the activation.  Output columns 0 .. 15 have a one-hot weight row (column n reads A[m, n], every other
product of its sum is an exact zero and its bias is zero), so their pre-activation value is the float32 number written into A:
0, +-1 (the hardtanh knees) and their float32 neighbours, +-30 (tanh and erf saturated), -100 (the selu exponential underflows),
+-6 and smaller values, rotated by the row so that every row tile sees each.  The other columns are dense sums over the remaining
K - 16 inputs with standard deviation 2.5 plus a bias: a dense range over [-6, 6] and beyond.

Truth is the float64 GEMM followed by the float64 torch activation, the yardstick the same on the CPU in float32; the rule is
tests/budget.py.  Beyond it: hardtanh and relu at the exact inputs give the expected constants bit for bit, selu(-100) is
-scale * alpha rounded to float32, and every output is finite."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import budget

pytestmark = pytest.mark.gpu

ACT = {'none': 0, 'relu': 1, 'silu': 2, 'gelu': 3, 'tanh': 4, 'hardtanh': 5, 'selu': 6}
FN = {'none': lambda x: x, 'relu': F.relu, 'silu': F.silu, 'gelu': F.gelu, 'tanh': torch.tanh, 'hardtanh': F.hardtanh,
      'selu': F.selu}
NEXT = float(np.nextafter(np.float32(1), np.float32(2)))       # the float32 above 1
PREV = float(np.nextafter(np.float32(1), np.float32(0)))       # and below
SPECIAL = [0.0, 1.0, -1.0, 30.0, -30.0, -100.0, NEXT, -NEXT, PREV, -PREV, 6.0, -6.0, 0.5, -0.5, 2.0 ** -20, -3.0]
NS = len(SPECIAL)
SHAPES = [(M, N, K) for M in (1, 33, 130) for N in (64, 384) for K in (32, 256)]
SELU_SCALE, SELU_ALPHA = 1.0507009873554805, 1.6732632423543772


@pytest.fixture(scope='module')
def eng():
    from masr_amd.engine import HipEngine
    e = HipEngine(None, {'num_blocks': 1}, vocab_size=8, streaming=True, use_model='conformer')
    yield e
    e.close()


def _inputs(M, N, K):
    """A [M, K], W [N, K], bias [N] float32 and the exact pre-activation values of columns 0 .. 15 [M, 16]"""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * (2.5 / np.sqrt(K - NS))
    bias = torch.randn(N, generator=g)
    exact = torch.tensor([[SPECIAL[(m + n) % NS] for n in range(NS)] for m in range(M)], dtype=torch.float32)
    a[:, :NS] = exact
    w[:, :NS] = 0
    w[:NS] = 0
    w[:NS, :NS] = torch.eye(NS)
    bias[:NS] = 0
    return a, w, bias, exact


@pytest.fixture(scope='module')
def cases():
    """{shape: (a, w, bias, exact, float32 pre-activation, float64 pre-activation)}, computed once"""
    out = {}
    for M, N, K in SHAPES:
        a, w, bias, exact = _inputs(M, N, K)
        z32 = a @ w.t() + bias
        z64 = a.double() @ w.double().t() + bias.double()
        assert torch.equal(z32[:, :NS], exact) and torch.equal(z64[:, :NS], exact.double())
        out[(M, N, K)] = (a, w, bias, exact, z32, z64)
    return out


@pytest.mark.parametrize('M,N,K', SHAPES)
@pytest.mark.parametrize('name', list(ACT))
def test_epilogue(eng, cases, name, M, N, K):
    a, w, bias, exact, z32, z64 = cases[(M, N, K)]
    y32, y64 = FN[name](z32), FN[name](z64)
    got = eng.op_gemm(a.cuda(), w.cuda(), bias.cuda(), act=ACT[name]).cpu()
    assert tuple(got.shape) == (M, N) and bool(torch.isfinite(got).all())
    budget.check(f'op_gemm {name} M={M} N={N} K={K}', y64, y32, got)
    head = got[:, :NS]
    if name in ('none', 'relu', 'hardtanh'):       # exact functions of exact inputs: the constants, bit for bit
        want = FN[name](exact)
        assert torch.equal(head, want), (head - want).abs().max()
    if name == 'hardtanh':
        assert set(head.flatten().tolist()) >= {1.0, -1.0, 0.0, 0.5, -0.5, PREV, -PREV}
    if name == 'selu':
        at = exact == -100.0
        assert at.any() and bool((head[at] == np.float32(-SELU_SCALE * SELU_ALPHA)).all()), head[at]
    if name in ('tanh', 'gelu'):                   # saturated: +-1, and 30 / -0
        assert bool((head[exact == 30.0] == (1.0 if name == 'tanh' else 30.0)).all())
        assert bool((head[exact == -30.0] == (-1.0 if name == 'tanh' else 0.0)).all())


def test_unknown_act_is_refused_by_name(eng):
    from masr_amd._lib import MasrError
    a, w = torch.zeros(1, 32).cuda(), torch.zeros(64, 32).cuda()
    for act in (8, -1, 7):
        with pytest.raises(MasrError, match='act') as ei:
            eng.op_gemm(a, w, act=act)
        assert 'masr_op_gemm' in str(ei.value) and str(act) in str(ei.value)
