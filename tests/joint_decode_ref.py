"""Restatement of the joint CTC / attention search (``decoder: joint``; a helper module: tests import it), built on the step
log-probabilities and the selection order of tests/attention_decode_ref.py and the prefix scorer of tests/ctc_prefix_ref.py.

Every hypothesis carries A, psi, n and the key J = ((1 - lam) A + lam psi) + gamma n, evaluated in ``dtype`` (float64: the truth;
float32: the restatement of the device).  Per step and live hypothesis: the top M attention log-probabilities, psi of those M
candidates, J of each; finished hypotheses offer themselves once; the top N of the N x M keys, ties to the smaller flat index.

The DECISION MARGIN of a step is the smaller of two gaps, both in the run's own arithmetic (float64 for the truth): the smallest
gap among the sorted top N + 1 finite keys of the N x M candidates, and, per live hypothesis with a finite A, the gap between its
M-th and (M + 1)-th attention log-probability (the candidate set itself is a decision).  ``attention_decode_ref.safety`` reads
the margins and the trace as it does for the attention search."""
import numpy as np

import attention_decode_ref as ar
import ctc_prefix_ref as cp


def key_of(att, psi, n, lam, gamma, dt):
    w = dt(1.0) - dt(lam)
    mix = w * dt(att)
    if lam != 0:
        mix = mix + dt(lam) * dt(psi)
    return dt(mix + dt(gamma) * dt(n))


def search(sd, memory, lp, n, m, lam, gamma, max_len=0, heads=4, max_pos=5000, logp_fn=None, vocab=None, pe=None, dtype=np.float64):
    """the joint search of ONE utterance: ``memory`` [T, d] its valid encoder frames, ``lp`` [T, V] the log posteriors of the same
    frames (cast to ``dtype``) -> dict(hyps [(tokens up to the first eos, J)] x N, parts [(A, psi)] x N, steps, limit, margins,
    trace [per step (parents, tokens, keys)]).  ``logp_fn(tokens)`` with ``vocab``: hand-made attention tables."""
    dt = np.dtype(dtype).type
    if logp_fn is None:
        V, d = sd['decoder.left_decoder.embed.0.weight'].shape
        from masr_amd.engine import positional_table
        pe = positional_table(ar.limit_of(len(memory), max_len, max_pos) + 2, d) if pe is None else pe
        logp_fn = lambda toks: ar.step_logp(sd, memory, toks, heads, pe)
    else:
        V = vocab
    eos = V - 1
    ninf = dt(-np.inf)
    lp = None if lam == 0 else np.asarray(lp).astype(dtype)
    state0 = cp.empty_state(lp) if lam != 0 else (None, None)
    hyps = [dict(tok=[], att=dt(0.0) if h == 0 else ninf, psi=dt(0.0), n=0, key=dt(0.0) if h == 0 else ninf, r=state0) for h in range(n)]
    lim = ar.limit_of(len(memory), max_len, max_pos)
    margins, trace, steps = [], [], 0
    for i in range(1, lim + 1):
        fin = [len(h['tok']) > 0 and h['tok'][-1] == eos for h in hyps]
        if all(fin):
            break
        steps = i
        cand, gaps = [], []
        for h, hyp in enumerate(hyps):
            if fin[h]:
                cand += [(hyp['key'], h, eos, hyp['att'], hyp['psi'], hyp['n'])] + [(ninf, h, eos, ninf, ninf, hyp['n'])] * (m - 1)
                continue
            logp = np.asarray(logp_fn(hyp['tok']))
            tops = ar.top_n(logp, m)
            if np.isfinite(hyp['att']) and m < V:
                srt = np.sort(np.asarray(logp, np.float64))[::-1]
                gaps.append(float(srt[m - 1] - srt[m]))
            ids = [t for _, t in tops]
            last = hyp['tok'][-1] if hyp['tok'] else None
            psi = cp.score(lp, hyp['r'][0], hyp['r'][1], last, ids, not hyp['tok']) if lam != 0 else [dt(0.0)] * m
            for k, (v, t) in enumerate(tops):
                att = dt(hyp['att'] + dt(v))
                cnt = hyp['n'] + (t != eos)
                cand.append((key_of(att, psi[k], cnt, lam, gamma, dt), h, int(t), att, dt(psi[k]), cnt))
        keys = np.array([c[0] for c in cand], np.float64)
        top = np.sort(keys[np.isfinite(keys)])[::-1][:n + 1]
        if len(top) > 1:
            gaps.append(float(np.min(top[:-1] - top[1:])))
        margins.append(min(gaps) if gaps else np.inf)
        new = []
        for _, c in ar.top_n([c[0] for c in cand], n):
            key, h, t, att, psi, cnt = cand[c]
            par = hyps[h]
            r = par['r']
            if lam != 0 and not fin[h] and t != eos:
                last = par['tok'][-1] if par['tok'] else None
                if t == cp.BLANK:
                    r = (np.full_like(r[0], -np.inf), np.full_like(r[1], -np.inf))
                else:
                    r = cp.advance(lp, r[0], r[1], last, t, not par['tok'])
            new.append(dict(tok=par['tok'] + [t], att=att, psi=psi, n=cnt, key=key, r=r, parent=h))
        hyps = new
        trace.append(([h['parent'] for h in hyps], [h['tok'][-1] for h in hyps], [float(h['key']) for h in hyps]))
    cut = lambda t: t[:t.index(eos)] if eos in t else list(t)
    return dict(hyps=[(cut(h['tok']), float(h['key'])) for h in hyps], parts=[(float(h['att']), float(h['psi'])) for h in hyps],
                steps=steps, limit=lim, margins=margins, trace=trace)


def log_posteriors(sd, memory, dtype=np.float64):
    """ln softmax of the CTC head over ``memory`` [T, d] in ``dtype`` (the posteriors of tests that have no device)"""
    w = np.asarray(sd['ctc.ctc_lo.weight'].detach().cpu().numpy(), dtype)
    b = np.asarray(sd['ctc.ctc_lo.bias'].detach().cpu().numpy(), dtype)
    z = np.asarray(memory, dtype) @ w.T + b
    z = z - z.max(axis=-1, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=-1, keepdims=True))).astype(dtype)


# the end-to-end case of the GPU search-parity test, chosen on the CPU (tests/test_joint_decode_cpu.py asserts the cap for it):
# synthetic_pcm seed, utterance lengths in samples (18 .. 32 encoder frames), beam size, CTC-scored candidates, the (lam, gamma) grid
E2E = dict(pcm_seed=21, lens=[21360, 20080, 18800, 17520, 16240, 14960, 13680, 12400], beam_size=4, ctc_candidates=8,
           grid=[(0.3, 0.0), (0.3, 0.5), (0.7, 0.0), (0.7, 0.5)])
