"""A plain reference of the relative-position attention of masr_amd/csrc/attention.hip (a helper module: tests import it).

Written from the formula at the top of that file, generic in dtype (float64 is the truth of tests/test_gpu_attention_op.py,
float32 on the CPU its yardstick); it never calls the code under test.  tests/test_attention_ref_cpu.py pins it against the
attention of oracle/conformer.py and oracle/efficient_conformer.py.

    score[i, j] = ((q_i + u) . k_j + (q_i + v) . p_j) * scale          scale = 1 / sqrt(d_k)
    key j is visible to query i  iff  j < klen  and, for chunk_size > 0,
                                      pos_stride * j < ((pos_stride * (q_abs0 + i)) // chunk_size + 1) * chunk_size
    out_i = sum_j softmax_{visible j}(score[i, :])[j] * v_j ;  a query with no visible key gives zeros

``p_j`` is the positional row of key j -- the caller gathers rows pos0 + pos_stride * j of its table."""
import math

import torch
import torch.nn.functional as F


def visible(nq, nk, klen, chunk_size=0, pos_stride=1, q_abs0=0):
    """bool [nq, nk]: the mask of the formula above"""
    j = torch.arange(nk)[None, :]
    m = (j < klen).expand(nq, nk).clone()
    if chunk_size > 0:
        i = torch.arange(nq)[:, None]
        m &= pos_stride * j < ((pos_stride * (q_abs0 + i)) // chunk_size + 1) * chunk_size
    return m


def attention(q, k, v, p, bias_u, bias_v, klen, chunk_size=0, pos_stride=1, q_abs0=0):
    """q [nq, H, dk]; k, v, p [nk, H, dk]; bias_u, bias_v [H, dk] -> [nq, H * dk], in the dtype of q"""
    nq, H, dk = q.shape
    nk = k.shape[0]
    qu = (q + bias_u).transpose(0, 1)                       # [H, nq, dk]
    qv = (q + bias_v).transpose(0, 1)
    kt, pt, vt = k.transpose(0, 1), p.transpose(0, 1), v.transpose(0, 1)
    scores = (qu @ kt.transpose(1, 2) + qv @ pt.transpose(1, 2)) / math.sqrt(dk)
    m = visible(nq, nk, klen, chunk_size, pos_stride, q_abs0)[None]
    scores = scores.masked_fill(~m, -float('inf'))
    top = scores.amax(dim=-1, keepdim=True)
    top = torch.where(torch.isinf(top), torch.zeros_like(top), top)        # a row without a visible key: exp(-inf - 0) = 0
    w = torch.exp(scores - top)
    den = w.sum(dim=-1, keepdim=True)
    attn = torch.where(den > 0, w / den, torch.zeros_like(w))
    return (attn @ vt).transpose(0, 1).reshape(nq, H * dk)


def grouped_attention(q, k, v, p, bias_u, bias_v, heads, klen, chunk_size=0, group=3):
    """The grouped form of the Efficient Conformer (oracle/efficient_conformer.py _grouped_attention): q, k, v, p [T, H * dk] of
    the TRUE length T are zero-padded in time to a multiple of ``group`` (P with zeros too, not with positional rows) and
    flat-reshaped to [T / group, H, group * dk]; bias_u, bias_v [H, group * dk]; scale 1 / sqrt(group * dk).  ``klen`` counts
    grouped keys (grouped key j is valid iff frame group * j is); the chunk mask keeps rows and columns 0, group, 2 group, ...
    of the frame-rate mask.  Returns all the grouped rows, [ceil(T / group), H * group * dk] (== the padded [T_pad, H * dk])."""
    T, d = q.shape
    pad = (group - T % group) % group
    g = lambda t: F.pad(t, (0, 0, 0, pad)).reshape(-1, heads, group * d // heads)
    return attention(g(q), g(k), g(v), g(p), bias_u, bias_v, klen, chunk_size, pos_stride=group, q_abs0=0)
