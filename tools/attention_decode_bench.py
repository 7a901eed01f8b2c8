"""Times one pass of ``decoder: attention`` (masr_attention_decode) beside the encoder pass it follows.

    python tools/attention_decode_bench.py [--batch 32] [--seconds 10] [--beam 10] [--runs 5] [--vocab 4233] [--max-len 0] [--torch] [--joint] [--lm]

Synthetic Conformer checkpoint with the shipped decoder (3 + 3 blocks, 4 heads, linear_units 1024; only the left half is used),
``batch`` utterances of ``seconds`` s, beam ``beam``.  Per run, alternating: the encoder pass (masr_encode_full) and the search,
each timed with events on the stream; prints medians, min / max, the steps run and the run count as one JSON line.  Synthetic
checkpoints rarely emit eos, so the search runs to its limit (the utterance's encoder frames): the figure is the worst case of
that length.  ``--torch``: the same search in plain torch on the device beside it (batched over the hypotheses, the whole prefix
recomputed every step as the reference's forward_one_step does without a cache; ties as torch.topk leaves them).  ``--joint``: one
pass of ``decoder: joint`` beside it on the same encoder output (the CTC head + masr_joint_decode, ``--ctc-weight`` 0.3,
``--candidates`` 20).  ``--lm`` (implies ``--joint``): one more pass beside those, masr_joint_decode_lm with a synthetic
character ARPA model of ``--lm-order`` 3 over the vocabulary (``--lm-higher`` n-grams drawn per order above 1) at ``--lm-weight`` 0.3,
and the same call with lm_weight 0 (which launches what masr_joint_decode launches).  The per-kernel split comes from a kernel trace of this script."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_search(sd, enc, enc_lens, n, pe, heads=4, max_len=0):
    """the search on the device in plain torch, all utterances in lockstep to the longest limit (equal lengths in this tool)"""
    p = 'decoder.left_decoder.'
    F = torch.nn.functional
    B, Tp, d = enc.shape
    V = sd[p + 'embed.0.weight'].shape[0]
    eos, S, dk = V - 1, B * n, d // heads
    nl = len({k.split('.')[3] for k in sd if k.startswith(p + 'decoders.')})
    mem = enc.repeat_interleave(n, 0)
    mem_mask = (torch.arange(Tp, device=enc.device)[None] < enc_lens.repeat_interleave(n)[:, None])[:, None, None]
    lin = lambda name, x: F.linear(x, sd[name + '.weight'], sd[name + '.bias'])
    ln = lambda name, x: F.layer_norm(x, (d,), sd[name + '.weight'], sd[name + '.bias'], 1e-12)

    def mha(q_name, q_in, kv_in, mask):
        q = lin(q_name + 'linear_q', q_in).view(S, -1, heads, dk).transpose(1, 2)
        k = lin(q_name + 'linear_k', kv_in).view(S, -1, heads, dk).transpose(1, 2)
        v = lin(q_name + 'linear_v', kv_in).view(S, -1, heads, dk).transpose(1, 2)
        sc = (q @ k.transpose(2, 3)) / math.sqrt(dk)
        sc = sc.masked_fill(~mask, float('-inf'))
        return lin(q_name + 'linear_out', (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(S, -1, d))
    hyps = torch.full((S, 1), eos, dtype=torch.long, device=enc.device)
    scores = torch.full((B, n), float('-inf'), device=enc.device)
    scores[:, 0] = 0
    scores = scores.view(S, 1)
    limit = int(enc_lens.max()) if max_len <= 0 else min(int(enc_lens.max()), max_len)
    for i in range(1, limit + 1):
        x = sd[p + 'embed.0.weight'][hyps] * math.sqrt(d) + pe[:i]
        causal = torch.tril(torch.ones(i, i, dtype=torch.bool, device=enc.device))[None, None]
        for l in range(nl):
            q = f'{p}decoders.{l}.'
            y = ln(q + 'norm1', x)
            x = x + mha(q + 'self_attn.', y, y, causal)
            x = x + mha(q + 'src_attn.', ln(q + 'norm2', x), mem, mem_mask)
            x = x + lin(q + 'feed_forward.w_2', torch.relu(lin(q + 'feed_forward.w_1', ln(q + 'norm3', x))))
        logp = torch.log_softmax(lin(p + 'output_layer', ln(p + 'after_norm', x[:, -1])), -1)
        top_v, top_i = logp.topk(n)
        fin = (hyps[:, -1] == eos) & (i > 1)
        top_v = torch.where(fin[:, None], torch.cat([torch.zeros(S, 1, device=enc.device),
                                                     torch.full((S, n - 1), float('-inf'), device=enc.device)], 1), top_v)
        top_i = torch.where(fin[:, None], torch.full_like(top_i, eos), top_i)
        cand = (scores + top_v).view(B, n * n)
        scores, flat = cand.topk(n)
        parent = flat // n + (torch.arange(B, device=enc.device) * n)[:, None]
        tok = top_i.view(B, n * n).gather(1, flat)
        hyps = torch.cat([hyps[parent.view(-1)], tok.view(-1, 1)], 1)
        scores = scores.view(S, 1)
    return hyps, scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--beam', type=int, default=10)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--vocab', type=int, default=4233)
    ap.add_argument('--max-len', type=int, default=0)
    ap.add_argument('--torch', action='store_true')
    ap.add_argument('--joint', action='store_true')
    ap.add_argument('--ctc-weight', type=float, default=0.3)
    ap.add_argument('--candidates', type=int, default=20)
    ap.add_argument('--lm', action='store_true')
    ap.add_argument('--lm-weight', type=float, default=0.3)
    ap.add_argument('--lm-order', type=int, default=3)
    ap.add_argument('--lm-higher', type=int, default=20000)
    a = ap.parse_args()
    a.joint = a.joint or a.lm
    from masr_amd.engine import HipEngine, positional_table
    from masr_amd.utils import synthetic
    dec = dict(linear_units=1024, num_blocks=3, r_num_blocks=3)
    sd = synthetic.conformer_state_dict(0, a.vocab, decoder=dec)
    eng = HipEngine(sd, vocab_size=a.vocab, attention_decoder=True, decoder_conf=dict(attention_heads=4, **dec))
    n = int(a.seconds * 16000)
    pcm = torch.from_numpy(synthetic.synthetic_pcm(a.batch, n, seed=3)).to(eng.device)
    ns = torch.full((a.batch,), n, dtype=torch.int32, device=eng.device)
    feats, frames = eng.fbank_batch(pcm, ns)
    enc_lens = eng.enc_frames(frames).to(torch.int32).contiguous()

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1), out
    t_enc, t_dec, t_torch, t_joint, t_lm0, t_lm, steps = [], [], [], [], [], [], 0
    lm = None
    if a.lm:
        import tempfile
        from masr_amd.decoders.lm_scorer import LanguageModel, write_synthetic_arpa
        toks = synthetic.synthetic_vocab(a.vocab)
        with tempfile.TemporaryDirectory() as tmp:
            lm = LanguageModel(write_synthetic_arpa(os.path.join(tmp, 'bench.arpa'), toks, order=a.lm_order, n_higher=a.lm_higher), toks)
    dsd = {k: v.to(eng.device) for k, v in sd.items() if k.startswith('decoder.left_decoder.')} if a.torch else None
    pe = positional_table(int(enc_lens.max()) + 2, 256).to(eng.device) if a.torch else None
    for k in range(a.runs + 2):
        te, enc = timed(lambda: eng.encode_full(feats, frames, -1))
        td, out = timed(lambda: eng.attention_decode(enc, enc_lens, a.beam, a.max_len))
        steps = out[3]
        if a.joint:
            tj, _ = timed(lambda: eng.joint_decode(enc, enc_lens, eng.ctc_probs(enc), a.beam, a.candidates, a.ctc_weight, 0.0, a.max_len))
        if a.lm:
            fused = lambda w: eng.joint_decode_lm(enc, enc_lens, eng.ctc_probs(enc), lm, w, a.beam, a.candidates, a.ctc_weight, 0.0,
                                                  a.max_len)
            tl0, _ = timed(lambda: fused(0.0))
            tl, _ = timed(lambda: fused(a.lm_weight))
        if a.torch:
            with torch.no_grad():
                tt, _ = timed(lambda: torch_search(dsd, enc, enc_lens, a.beam, pe, 4, a.max_len))
        if k >= 2:                       # two warm-up rounds (workspaces, clocks)
            t_enc.append(te)
            t_dec.append(td)
            if a.joint:
                t_joint.append(tj)
            if a.lm:
                t_lm0.append(tl0)
                t_lm.append(tl)
            if a.torch:
                t_torch.append(tt)
    stat = lambda v: {'median_ms': float(np.median(v)), 'min_ms': float(min(v)), 'max_ms': float(max(v))}
    res = {'batch': a.batch, 'seconds': a.seconds, 'beam': a.beam, 'runs': a.runs, 'steps': steps, 'enc_frames': int(enc_lens.max()),
           'encoder_pass': stat(t_enc), 'attention_decode_pass': stat(t_dec), 'decoder': eng.decoder_info()}
    res['ms_per_step'] = res['attention_decode_pass']['median_ms'] / max(steps, 1)
    if a.torch:
        res['torch_search'] = stat(t_torch)
    if a.joint:
        res['joint_decode_pass'] = dict(stat(t_joint), ctc_weight=a.ctc_weight, candidates=a.candidates)
    if a.lm:
        res['joint_decode_lm_weight0_pass'] = stat(t_lm0)
        res['joint_decode_lm_pass'] = dict(stat(t_lm), lm_weight=a.lm_weight, order=lm.max_order, n_ngrams=lm.n_ngrams)
        res['lm_ms_per_step'] = (res['joint_decode_lm_pass']['median_ms'] - res['joint_decode_pass']['median_ms']) / max(steps, 1)
    print(json.dumps(res))
    eng.close()


if __name__ == '__main__':
    main()
