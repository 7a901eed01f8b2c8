"""Restatement of the joint search with shallow fusion of the n-gram language model (``decoder: joint`` with ``lm_weight``; a helper
module: tests import it): the search of tests/joint_decode_ref.py with a fourth part per hypothesis,

    Lm(g . c) = Lm(g) + lm(g, c)        J = (((1 - lam) A + lam psi) + mu Lm) + gamma n        (mu = lm_weight)

lm(g, c) is ``LanguageModel.cond_log_prob(g + [c])`` (eos asked for as the model's ``</s>``): a float32 value, exact in float64.
Lm and J are accumulated in ``dtype`` (float64: the truth; float32: the restatement of the device).  The LM is a partial scorer:
the M candidates of a hypothesis stay its top M by attention log-probability.  With mu = 0 the model is never asked and the
function returns ``joint_decode_ref.search``'s hypotheses, keys and trace exactly.

Decision margins are those of joint_decode_ref over the NEW key (plus the candidate-set gap, which the LM does not touch); the
trace is in the shape ``attention_decode_ref.safety`` reads."""
import numpy as np

import attention_decode_ref as ar
import ctc_prefix_ref as cp


def key_of(att, psi, lm, n, lam, mu, gamma, dt):
    w = dt(1.0) - dt(lam)
    mix = w * dt(att)
    if lam != 0:
        mix = mix + dt(lam) * dt(psi)
    if mu != 0:
        mix = mix + dt(mu) * dt(lm)
    return dt(mix + dt(gamma) * dt(n))


def lm_fn_of(model, vocab):
    """(tokens, candidate) -> lm(g, c) of ``model`` (a LanguageModel over ``vocab`` tokens), remembered per (window, candidate)"""
    eos, memo = vocab - 1, {}
    k = max(model.max_order - 1, 0)

    def fn(tokens, c):
        key = (tuple(tokens[len(tokens) - min(len(tokens), k):]), c)
        if key not in memo:
            memo[key] = np.float32(model.cond_log_prob(list(tokens) + [model.eos if c == eos else c]))
        return memo[key]
    return fn


def search(memory, lp, n, m, lam, mu, gamma, logp_fn, vocab, lm_fn=None, max_len=0, max_pos=5000, dtype=np.float64):
    """the search of ONE utterance: ``memory`` [T, d] its valid encoder frames (only their count is read here), ``lp`` [T, V] the
    log posteriors of the same frames, ``logp_fn(tokens)`` the attention log-probabilities [V] behind ``tokens``, ``lm_fn(tokens,
    c)`` the language model (``lm_fn_of``; not needed with mu = 0) -> dict(hyps [(tokens up to the first eos, J)] x N, parts
    [(A, psi)] x N, lm [Lm] x N, steps, limit, margins, trace [per step (parents, tokens, keys)])"""
    dt = np.dtype(dtype).type
    V, eos = vocab, vocab - 1
    ninf = dt(-np.inf)
    lp = None if lam == 0 else np.asarray(lp).astype(dtype)
    state0 = cp.empty_state(lp) if lam != 0 else (None, None)
    hyps = [dict(tok=[], att=dt(0.0) if h == 0 else ninf, psi=dt(0.0), lm=dt(0.0), n=0, key=dt(0.0) if h == 0 else ninf, r=state0)
            for h in range(n)]
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
                cand += [(hyp['key'], h, eos, hyp['att'], hyp['psi'], hyp['lm'], hyp['n'])]
                cand += [(ninf, h, eos, ninf, ninf, hyp['lm'], hyp['n'])] * (m - 1)
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
                lm = dt(hyp['lm'] + dt(lm_fn(hyp['tok'], int(t)))) if mu != 0 else dt(0.0)
                cand.append((key_of(att, psi[k], lm, cnt, lam, mu, gamma, dt), h, int(t), att, dt(psi[k]), lm, cnt))
        keys = np.array([c[0] for c in cand], np.float64)
        top = np.sort(keys[np.isfinite(keys)])[::-1][:n + 1]
        if len(top) > 1:
            gaps.append(float(np.min(top[:-1] - top[1:])))
        margins.append(min(gaps) if gaps else np.inf)
        new = []
        for _, c in ar.top_n([c[0] for c in cand], n):
            key, h, t, att, psi, lm, cnt = cand[c]
            par = hyps[h]
            r = par['r']
            if lam != 0 and not fin[h] and t != eos:
                last = par['tok'][-1] if par['tok'] else None
                if t == cp.BLANK:
                    r = (np.full_like(r[0], -np.inf), np.full_like(r[1], -np.inf))
                else:
                    r = cp.advance(lp, r[0], r[1], last, t, not par['tok'])
            new.append(dict(tok=par['tok'] + [t], att=att, psi=psi, lm=lm, n=cnt, key=key, r=r, parent=h))
        hyps = new
        trace.append(([h['parent'] for h in hyps], [h['tok'][-1] for h in hyps], [float(h['key']) for h in hyps]))
    cut = lambda t: t[:t.index(eos)] if eos in t else list(t)
    return dict(hyps=[(cut(h['tok']), float(h['key'])) for h in hyps], parts=[(float(h['att']), float(h['psi'])) for h in hyps],
                lm=[float(h['lm']) for h in hyps], steps=steps, limit=lim, margins=margins, trace=trace)


# the model of the GPU tests (tests/test_gpu_joint_lm.py) and of the CPU test that asserts their cap: V = 50, encoder of 2 blocks,
# left decoder of 1 block, no right decoder
V = 50
SEED = 11
DEC = dict(linear_units=384, num_blocks=1, r_num_blocks=0)


def state_dict(vocab=V):
    from masr_amd.utils import synthetic
    return synthetic.conformer_state_dict(SEED, vocab, d_ff=256, num_blocks=2, decoder=DEC)


def synthetic_model(path, vocab, order, seed=5, n_higher=400):
    """(LanguageModel, vocabulary list): write_synthetic_arpa over synthetic_vocab(vocab) at ``path``, loaded"""
    from masr_amd.decoders.lm_scorer import LanguageModel, write_synthetic_arpa
    from masr_amd.utils import synthetic
    toks = synthetic.synthetic_vocab(vocab)
    write_synthetic_arpa(str(path), toks, order=order, seed=seed, n_higher=n_higher)
    return LanguageModel(str(path), toks), toks


# the end-to-end case of the GPU search-parity test, chosen on the CPU (tests/test_joint_lm_cpu.py asserts the cap for it):
# synthetic_pcm seed, utterance lengths in samples (18 .. 32 encoder frames), beam size, scored candidates, the synthetic ARPA
# (write_synthetic_arpa seed / order / n_higher over synthetic_vocab(V)), the (ctc_weight, lm_weight, length_bonus) grid
E2E_LM = dict(pcm_seed=21, lens=[21360, 20080, 18800, 17520, 16240, 14960, 13680, 12400], beam_size=4, ctc_candidates=8,
              arpa_seed=5, arpa_order=3, arpa_n_higher=400,
              grid=[(0.3, 0.3, 0.0), (0.3, 0.6, 0.5), (0.0, 0.3, 0.0), (0.7, 0.1, 0.5)])
