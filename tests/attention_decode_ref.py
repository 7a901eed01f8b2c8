"""Plain-torch restatement of the attention decoding mode (``decoder: attention``; a helper module: tests import it).

The step log-probabilities are the last row of the left decoder's causal forward over [sos, tokens...] with source attention over
the utterance's valid encoder frames -- what the reference's ``forward_one_step`` returns -- with the LayerNorm and the block
count of tests/rescoring_ref.py and the attention in the reference's own 4-D shapes.  The dtype is the state dict's: ``rescoring_ref.to64(sd)`` gives the float64 truth, the float32 dict the
CPU reference.  The search loop holds the rules of include/masr_hip.h:

    top N of a row: the larger value first, of bit-equal values the smaller token id first
    finished rows (last token eos) offer (0, eos), (-inf, eos), ...
    merge: the top N of the N x N sums, of bit-equal sums (-inf included) the smaller parent_rank * N + candidate_rank first
    limit: min(valid encoder frames, max_len if positive, max_pos - 1) steps, or all N finished

and records, per step, the DECISION MARGIN: the smallest gap between consecutive entries of the sorted top N + 1 accumulated scores
over all N x V continuations of the live (unfinished, finite) rows together with the finished rows' own scores."""
import math

import numpy as np
import torch

import rescoring_ref as rr
from masr_amd.engine import positional_table


def _lin(sd, name, x):
    return torch.nn.functional.linear(x, sd[name + '.weight'], sd[name + '.bias'])


def _mha(sd, p, q_in, kv_in, heads, causal):
    """the reference's MultiHeadedAttention on a batch of one, in its shapes ([1, heads, n, dk] matmuls): at 18 rows and more the
    CPU's 2-D and 4-D products take other paths and differ by several float32 ulp, so the restatement keeps the 4-D ones"""
    _, n, d = q_in.shape
    dk = d // heads
    q = _lin(sd, p + 'linear_q', q_in).view(1, -1, heads, dk).transpose(1, 2)
    k = _lin(sd, p + 'linear_k', kv_in).view(1, -1, heads, dk).transpose(1, 2)
    v = _lin(sd, p + 'linear_v', kv_in).view(1, -1, heads, dk).transpose(1, 2)
    scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(dk)
    if causal:
        mask = ~torch.tril(torch.ones(n, k.shape[2], dtype=torch.bool))[None, None]
        att = torch.softmax(scores.masked_fill(mask, float('-inf')), dim=-1).masked_fill(mask, 0.0)
    else:
        att = torch.softmax(scores, dim=-1)
    x = torch.matmul(att, v).transpose(1, 2).contiguous().view(1, -1, d)
    return _lin(sd, p + 'linear_out', x)


def step_logp(sd, memory, tokens, heads=4, pe=None):
    """log_softmax(output_layer(after_norm(x_last))) [V] behind the prefix ``tokens`` (ids after sos) over ``memory`` [T, d]"""
    p = 'decoder.left_decoder.'
    emb = sd[p + 'embed.0.weight']
    V, d = emb.shape
    dt = emb.dtype
    memory = torch.as_tensor(memory).to(dt)[None]
    ys_in = torch.tensor([[V - 1] + [int(t) for t in tokens]], dtype=torch.long)
    n = ys_in.shape[1]
    pe = positional_table(n, d) if pe is None else pe
    with torch.no_grad():
        x = emb[ys_in] * math.sqrt(d) + pe[None, :n].to(dt)
        for i in range(rr.blocks(sd, 'left')):
            q = f'{p}decoders.{i}.'
            y = rr._ln(sd, q + 'norm1', x)
            x = x + _mha(sd, q + 'self_attn.', y, y, heads, True)
            x = x + _mha(sd, q + 'src_attn.', rr._ln(sd, q + 'norm2', x), memory, heads, False)
            y = rr._ln(sd, q + 'norm3', x)
            x = x + _lin(sd, q + 'feed_forward.w_2', torch.relu(_lin(sd, q + 'feed_forward.w_1', y)))
        logits = _lin(sd, p + 'output_layer', rr._ln(sd, p + 'after_norm', x[:, -1]))
        return torch.log_softmax(logits, dim=-1)[0].numpy()


def top_n(values, n):
    """[(value, index)] of the first n in the order: the larger value first, of equal values the smaller index first"""
    v = np.asarray(values)
    order = sorted(range(len(v)), key=lambda i: (-v[i], i))          # (-(-inf) = inf sorts last; equal keys keep the index order)
    return [(v[i], i) for i in order[:n]]


def merge(scores, tops, finished, n, eos):
    """one beam merge: ``scores`` [N], ``tops`` [N][(logp, token)] x N, ``finished`` [N] -> [(score, parent, token)] of the new ranks"""
    cand = []
    for h in range(len(scores)):
        for k in range(n):
            if finished[h]:
                lp, t = (0.0 if k == 0 else -np.inf), eos
            else:
                lp, t = tops[h][k]
            cand.append((scores[h] + lp, h, t))
    flat = top_n([c[0] for c in cand], n)
    return [(cand[i][0], cand[i][1], cand[i][2]) for _, i in flat]


def limit_of(enc_len, max_len=0, max_pos=5000):
    lim = min(int(enc_len), max_pos - 1)
    return min(lim, max_len) if max_len > 0 else lim


def search(sd, memory, n, max_len=0, heads=4, max_pos=5000, run_to_limit=False, logp_fn=None, vocab=None, pe=None):
    """the search of ONE utterance over its valid frames ``memory`` [T, d] -> dict(hyps [(tokens up to the first eos, score)] x N,
    steps, limit, margins [per step], trace [per step (parents, tokens, scores)]).  ``run_to_limit``: no early stop when all N are
    finished (the steps past it must change nothing).  ``logp_fn(tokens)`` with ``vocab``: the step log-probabilities from somewhere
    else (hand-made tables of the tie tests).  ``pe``: positional rows to use instead of this machine's table."""
    if logp_fn is None:
        V, d = sd['decoder.left_decoder.embed.0.weight'].shape
        pe = positional_table(limit_of(len(memory), max_len, max_pos) + 2, d) if pe is None else pe
        logp_fn = lambda toks: step_logp(sd, memory, toks, heads, pe)
    else:
        V = vocab
    eos = V - 1
    hyps = [[] for _ in range(n)]
    scores = [0.0] + [-np.inf] * (n - 1)
    lim = limit_of(len(memory), max_len, max_pos)
    margins, trace, steps = [], [], 0
    for i in range(1, lim + 1):
        finished = [len(h) > 0 and h[-1] == eos for h in hyps]
        if all(finished):
            if not run_to_limit:
                break
        else:
            steps = i
        logps = [None if finished[h] else np.asarray(logp_fn(hyps[h])) for h in range(n)]
        tops = [None if finished[h] else top_n(logps[h], n) for h in range(n)]
        if not all(finished):
            # decision margin over every continuation that could enter or reorder the beam
            allc = []
            for h in range(n):
                if finished[h]:
                    allc.append(np.array([scores[h]], np.float64))
                elif np.isfinite(scores[h]):
                    allc.append(np.float64(scores[h]) + np.asarray(logps[h], np.float64))
            allc = np.sort(np.concatenate(allc))[::-1][:n + 1]
            allc = allc[np.isfinite(allc)]
            margins.append(float(np.min(allc[:-1] - allc[1:])) if len(allc) > 1 else np.inf)
        new = merge(scores, tops, finished, n, eos)
        hyps = [hyps[h] + [int(t)] for _, h, t in new]
        scores = [s for s, _, _ in new]
        trace.append(([h for _, h, _ in new], [int(t) for _, _, t in new], list(scores)))
    out = [(h[:h.index(eos)] if eos in h else list(h), s) for h, s in zip(hyps, scores)]
    return dict(hyps=out, steps=steps, limit=lim, margins=margins, trace=trace)


# the end-to-end case (tests/test_gpu_attention_decode.py), chosen on the CPU (tests/test_attention_decode_cpu.py asserts the cap
# for them): synthetic_pcm seed, utterance lengths in samples (18 .. 32 encoder frames), beam size
E2E = dict(pcm_seed=21, lens=[21360, 20080, 18800, 17520, 16240, 14960, 13680, 12400], beam_size=4)


def safety(r64, r32, c=8.0):
    """(max|e_ref| of the trace, first unsafe step or None): e_ref = the float32 search's accumulated scores minus the float64
    ones over the steps on which both made the same decisions; a step is unsafe when its float64 decision margin does not exceed
    2 c max|e_ref|"""
    e = 0.0
    for (p64, t64, s64), (p32, t32, s32) in zip(r64['trace'], r32['trace']):
        if p64 != p32 or t64 != t32:
            break
        a, b = np.asarray(s64, np.float64), np.asarray(s32, np.float64)
        ok = np.isfinite(a) & np.isfinite(b)
        if ok.any():
            e = max(e, float(np.abs(a[ok] - b[ok]).max()))
    bar = 2 * c * e
    for k, m in enumerate(r64['margins']):
        if not m > bar:
            return e, k + 1
    return e, None
