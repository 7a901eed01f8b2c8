"""Gate for 16-row fused FFN tiles: a chain of v_mfma_f32_16x16x4_f32 must sum in exactly the order of the 32x32x2 chain the
fused kernels run today, or a 16-row kernel cannot be bit-identical to the 32-row one (the A/B tests of masr_debug_set keys 8, 9
and 23 compare with torch.equal).  In the 32x32x2 chain, MFMA q of 8-wide k group g adds k = 8g + q, then 8g + 4 + q.  In the
16x16x4 chain lane group kk of the first MFMA of a group takes k = 8g + perm[kk], of the second 8g + perm[4 + kk]."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SAME_ORDER = [0, 4, 1, 5, 2, 6, 3, 7]      # (0, 4), (1, 5), (2, 6), (3, 7): the 32x32x2 pairs, four k per 16x16x4 MFMA


def _probe(a, b, perm):
    from masr_amd import _lib
    k = a.shape[1]
    c32 = torch.empty(16, 16, device='cuda')
    c16 = torch.empty(16, 16, device='cuda')
    p = (ctypes.c_int32 * 8)(*perm)
    rc = _lib.lib().masr_mfma_order_probe(a.data_ptr(), b.data_ptr(), c32.data_ptr(), c16.data_ptr(), k, p,
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return c32, c16


def _operands(seed, k, spread):
    g = torch.Generator().manual_seed(seed)
    # values over many binades: every product and partial sum rounds, so any change of order shows in the last bits
    a = torch.randn(16, k, generator=g) * torch.exp2(torch.randint(-spread, spread + 1, (16, k), generator=g).float())
    b = torch.randn(16, k, generator=g) * torch.exp2(torch.randint(-spread, spread + 1, (16, k), generator=g).float())
    return a.cuda(), b.cuda()


@pytest.mark.parametrize('k', [8, 256, 1024])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_16x16x4_chain_is_bit_identical_to_32x32x2_chain(k, seed):
    a, b = _operands(seed, k, 12)
    c32, c16 = _probe(a, b, SAME_ORDER)
    assert torch.equal(c32, c16), (c32 - c16).abs().max().item()
    ref = (a.double() @ b.double().T)
    assert (c32.double() - ref).abs().max().item() <= 1e-3 * ref.abs().max().item()


def test_probe_sees_a_different_order():
    # the probe can tell orders apart: k in natural order (lane group kk takes 8g + kk, then 8g + 4 + kk) sums differently
    a, b = _operands(5, 256, 12)
    c32, c16 = _probe(a, b, [0, 1, 2, 3, 4, 5, 6, 7])
    assert not torch.equal(c32, c16)
