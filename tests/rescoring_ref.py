"""Plain-torch restatement of the attention decoder's forward and of the rescoring rule (a helper module: tests import it).

Written from the arithmetic of the issue, one hypothesis at a time and without padding: Embedding + PositionalEncoding
(x * sqrt(d) + pe), pre-norm blocks (causal self-attention, source attention over the utterance's valid encoder frames, ReLU
feed-forward; LayerNorm eps 1e-12), after_norm, output_layer, log_softmax, gather, sum in index order.  The dtype is the state
dict's: ``to64(sd)`` gives the float64 truth, the float32 dict the CPU reference."""
import math

import numpy as np
import torch

from masr_amd.engine import positional_table


def to64(sd):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}


def blocks(sd, side):
    head = f'decoder.{side}_decoder.decoders.'
    return len({k[len(head):].split('.', 1)[0] for k in sd if k.startswith(head)})


def _lin(sd, name, x):
    return x @ sd[name + '.weight'].t() + sd[name + '.bias']


def _ln(sd, name, x):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), sd[name + '.weight'], sd[name + '.bias'], 1e-12)


def _mha(sd, p, q_in, kv_in, heads, causal):
    n, d = q_in.shape
    dk = d // heads
    q = _lin(sd, p + 'linear_q', q_in).view(n, heads, dk).transpose(0, 1)
    k = _lin(sd, p + 'linear_k', kv_in).view(-1, heads, dk).transpose(0, 1)
    v = _lin(sd, p + 'linear_v', kv_in).view(-1, heads, dk).transpose(0, 1)
    scores = q @ k.transpose(1, 2) / math.sqrt(dk)
    if causal:
        mask = torch.tril(torch.ones(n, k.shape[1], dtype=torch.bool))
        scores = scores.masked_fill(~mask, float('-inf'))
    att = torch.softmax(scores, dim=-1) @ v
    return _lin(sd, p + 'linear_out', att.transpose(0, 1).reshape(n, d))


def score_one(sd, side, memory, tokens, heads=4, pe=None):
    """sum over the L + 1 positions of log_softmax(logits)[target] of ONE hypothesis (already reversed for side 'right') over
    ``memory`` [T, d] (the valid encoder frames only)"""
    p = f'decoder.{side}_decoder.'
    emb = sd[p + 'embed.0.weight']
    V, d = emb.shape
    dt = emb.dtype
    memory = memory.to(dt)
    ys_in = torch.tensor([V - 1] + list(tokens), dtype=torch.long)
    ys_out = torch.tensor(list(tokens) + [V - 1], dtype=torch.long)
    n = ys_in.shape[0]
    pe = positional_table(n, d) if pe is None else pe
    x = emb[ys_in] * math.sqrt(d) + pe[:n].to(dt)
    for i in range(blocks(sd, side)):
        q = f'{p}decoders.{i}.'
        y = _ln(sd, q + 'norm1', x)
        x = x + _mha(sd, q + 'self_attn.', y, y, heads, True)
        x = x + _mha(sd, q + 'src_attn.', _ln(sd, q + 'norm2', x), memory, heads, False)
        y = _ln(sd, q + 'norm3', x)
        x = x + _lin(sd, q + 'feed_forward.w_2', torch.relu(_lin(sd, q + 'feed_forward.w_1', y)))
    logits = _lin(sd, p + 'output_layer', _ln(sd, p + 'after_norm', x))
    lp = torch.log_softmax(logits, dim=-1)[torch.arange(n), ys_out]
    acc = torch.zeros((), dtype=dt)
    for v in lp:            # index order
        acc = acc + v
    return acc


def scores(sd, memory, mem_lens, hyps, lens, heads=4, with_right=True):
    """``memory`` [B, T, d], ``mem_lens`` [B] valid frames, ``hyps`` [B, N, Lmax] / ``lens`` [B, N] -> (att, r_att) [B, N] numpy in
    the state dict's dtype (r_att zero without a right decoder or with ``with_right=False``)"""
    hyps, lens = np.asarray(hyps), np.asarray(lens)
    B, N, _ = hyps.shape
    dt = sd['decoder.left_decoder.embed.0.weight'].dtype
    npdt = np.float64 if dt == torch.float64 else np.float32
    att, r_att = np.zeros((B, N), npdt), np.zeros((B, N), npdt)
    right = with_right and blocks(sd, 'right') > 0
    pe = positional_table(hyps.shape[2] + 1, sd['decoder.left_decoder.embed.0.weight'].shape[1])
    with torch.no_grad():
        for b in range(B):
            mem = torch.as_tensor(memory[b])[:int(mem_lens[b])]
            for n in range(N):
                t = [int(v) for v in hyps[b, n, :int(lens[b, n])]]
                att[b, n] = float(score_one(sd, 'left', mem, t, heads, pe)) if npdt is np.float64 else \
                    score_one(sd, 'left', mem, t, heads, pe).numpy()
                if right:
                    r = score_one(sd, 'right', mem, t[::-1], heads, pe)
                    r_att[b, n] = float(r) if npdt is np.float64 else r.numpy()
    return att, r_att


def combine(att, r_att, ctc, ctc_weight, reverse_weight):
    att, r_att, ctc = (np.asarray(a, np.float64) for a in (att, r_att, ctc))
    return att * (1.0 - reverse_weight) + r_att * reverse_weight + ctc_weight * ctc


def pick(total):
    """highest combined score; an exact tie goes to the earlier rank"""
    best = 0
    for i in range(1, len(total)):
        if total[i] > total[best]:
            best = i
    return best


# the end-to-end case (tests/test_gpu_rescoring.py), chosen on the CPU (tests/test_rescoring_cpu.py asserts the cap for them):
# synthetic_pcm seed, utterance lengths in samples, n-best size, weights
E2E = dict(pcm_seed=21, lens=[32000, 30000, 28000, 26000, 24000, 22000, 20000, 18000], beam_size=6, ctc_weight=0.5,
           reverse_weight=0.3, cutoff_prob=0.99, cutoff_top_n=40)
