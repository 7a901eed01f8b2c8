"""A plain reference of the attention WITHOUT the positional term -- the POS = 0 instantiations of masr_amd/csrc/attention.hip,
MultiHeadedAttention of the reference (conformer/attention.py:133-167) -- beside tests/attention_ref.py (a helper module: tests
import it).  Generic in dtype (float64 is the truth of tests/test_gpu_attention_nopos.py, float32 on the CPU its yardstick); it
never calls the code under test.

    score[i, j] = q_i . k_j * scale                                     scale = 1 / sqrt(d_k)
    key j is visible to query i  iff  j < klen  and, for chunk_size > 0,
                                      pos_stride * j < ((pos_stride * (q_abs0 + i)) // chunk_size + 1) * chunk_size
    out_i = sum_j softmax_{visible j}(score[i, :])[j] * v_j ;  a query with no visible key gives zeros

The mask is attention_ref.visible, the one of the relative-position kernels."""
import math

import torch

from tests.attention_ref import visible


def attention(q, k, v, klen, chunk_size=0, pos_stride=1, q_abs0=0):
    """q [nq, H, dk]; k, v [nk, H, dk] -> [nq, H * dk], in the dtype of q"""
    nq, H, dk = q.shape
    nk = k.shape[0]
    scores = (q.transpose(0, 1) @ k.transpose(0, 1).transpose(1, 2)) / math.sqrt(dk)          # [H, nq, nk]
    m = visible(nq, nk, klen, chunk_size, pos_stride, q_abs0)[None]
    scores = scores.masked_fill(~m, -float('inf'))
    top = scores.amax(dim=-1, keepdim=True)
    top = torch.where(torch.isinf(top), torch.zeros_like(top), top)        # a row without a visible key: exp(-inf - 0) = 0
    w = torch.exp(scores - top)
    den = w.sum(dim=-1, keepdim=True)
    attn = torch.where(den > 0, w / den, torch.zeros_like(w))
    return (attn @ v.transpose(0, 1)).transpose(0, 1).reshape(nq, H * dk)
