"""Writes tests/golden/attention_decode_v50.npz: ``forward_one_step`` of the LIVE reference's left decoder on fixed prefixes.

    python tools/make_attention_decode_golden.py [path of the reference checkout]

Builds the reference ``ConformerModel`` on the CPU from the seeded synthetic weights of ``masr_amd/utils/synthetic.py`` (the recipe
of tools/make_rescoring_golden.py: V = 50, 2 encoder blocks, decoder 2 + 2 blocks, 4 heads, linear_units 384), runs its encoder on
fixed features and ``model.decoder.left_decoder.forward_one_step`` on every fixed prefix [sos, tokens...] alone (batch of one, the
utterance's valid frames only, no cache: the whole prefix is recomputed, as the reference does), in float32 and -- the same module
converted with ``.double()``, on the float32 encoder output -- in float64.  Only recorded data goes into the file: the inputs, the
encoder output, the prefixes, the positional rows the model added and the log-probability rows.

The reference ships ``forward_one_step`` and no decoding loop of this mode.  The loop recorded here is WeNet's ``attention`` mode
written out as data flow over the live model's steps -- batched over the beam, ``torch.topk`` on the rows, the finished rows' scores
and predictions masked, ``torch.topk`` over the flattened N x N sums, parents by integer division of the flat index -- and is shaped
differently on purpose from the per-hypothesis loop of tests/attention_decode_ref.py, which the CPU test holds against its traces
(parents, tokens and accumulated scores of every step, float64 and float32) wherever no tie decides.  One trace runs with the eos
bias raised so that hypotheses finish while others run on."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECIPE = dict(seed=11, vocab_size=50, num_blocks=2, d_ff=256,
              decoder=dict(linear_units=384, num_blocks=2, r_num_blocks=2))
FEAT_LENS = [131, 99, 67]
PREFIX_LENS = [[0, 1, 9, 17], [17, 0, 5, 1], [2, 17, 0, 11]]
BEAM = 4
EOS_BIAS = 14.0                 # the fourth trace: utterance 2 with output_layer.bias[eos] raised by this


def recipe_inputs():
    """the fixed features and prefixes (seeded; no reference needed)"""
    rng = np.random.default_rng(17)
    T = max(FEAT_LENS)
    feats = (rng.standard_normal((len(FEAT_LENS), T, 80)) * 3 + 13).astype(np.float32)
    for b, n in enumerate(FEAT_LENS):
        feats[b, n:] = 0
    V, L = RECIPE['vocab_size'], max(max(r) for r in PREFIX_LENS)
    prefixes = np.zeros((len(PREFIX_LENS), len(PREFIX_LENS[0]), L), np.int32)
    for b, row in enumerate(PREFIX_LENS):
        for n, l in enumerate(row):
            prefixes[b, n, :l] = rng.integers(0, V - 1, l)
    return feats, np.array(FEAT_LENS, np.int32), prefixes, np.array(PREFIX_LENS, np.int32)


def beam_loop(dec, mem, n, V):
    """WeNet's attention decoding over one utterance's valid frames ``mem`` [1, T, d] with the live left decoder ``dec``: at most T
    steps -> (parents, tokens, scores) [steps, n] of every step"""
    eos = V - 1
    T = mem.shape[1]
    memory, mem_mask = mem.repeat(n, 1, 1), torch.ones(n, 1, T, dtype=torch.bool)
    hyps = torch.full((n, 1), eos, dtype=torch.long)
    scores = torch.tensor([0.0] + [-float('inf')] * (n - 1), dtype=mem.dtype).unsqueeze(1)
    end_flag = torch.zeros(n, 1, dtype=torch.bool)
    zero_rest = torch.tensor([0.0] + [-float('inf')] * (n - 1), dtype=mem.dtype)
    trace = []
    for i in range(1, T + 1):
        if end_flag.sum() == n:
            break
        tgt_mask = torch.tril(torch.ones(i, i, dtype=torch.bool)).unsqueeze(0).repeat(n, 1, 1)
        with torch.no_grad():
            logp, _ = dec.forward_one_step(memory, mem_mask, hyps, tgt_mask, None)
        top_v, top_i = logp.topk(n)
        top_v = torch.where(end_flag, zero_rest.unsqueeze(0).expand(n, n), top_v)           # mask_finished_scores
        top_i = torch.where(end_flag, torch.full_like(top_i, eos), top_i)                   # mask_finished_preds
        scores, flat = (scores + top_v).view(1, n * n).topk(n)
        parent = torch.div(flat, n, rounding_mode='floor').view(-1)
        tok = top_i.reshape(-1)[flat.view(-1)]
        hyps = torch.cat([hyps[parent], tok.view(-1, 1)], dim=1)
        scores = scores.view(n, 1)
        end_flag = (hyps[:, -1] == eos).view(n, 1)
        trace.append((parent.numpy().copy(), tok.numpy().copy(), scores.view(-1).numpy().copy()))
    return trace


def main():
    from oracle import shims
    if len(sys.argv) > 1:
        shims.REFERENCE_ROOT = sys.argv[1]
    shims.install()
    import yaml
    from masr.model_utils.conformer.model import ConformerModel
    from masr_amd.utils import synthetic
    cfg = yaml.safe_load(open(os.path.join(shims.REFERENCE_ROOT, 'configs', 'conformer.yml'), encoding='utf-8'))
    enc_conf = dict(cfg['encoder_conf'], num_blocks=RECIPE['num_blocks'], linear_units=RECIPE['d_ff'])
    dec_conf = dict(cfg['decoder_conf'], attention_heads=4, **RECIPE['decoder'])
    V = RECIPE['vocab_size']
    sd = synthetic.conformer_state_dict(RECIPE['seed'], V, d_ff=RECIPE['d_ff'], num_blocks=RECIPE['num_blocks'],
                                        decoder=RECIPE['decoder'])
    p = os.path.join(tempfile.mkdtemp(), 'm.json')
    json.dump({'mean': [0.0] * 80, 'istd': [1.0] * 80}, open(p, 'w'))
    m = ConformerModel(input_dim=80, vocab_size=V, mean_istd_path=p, streaming=True, encoder_conf=enc_conf, decoder_conf=dec_conf,
                       **cfg['model_conf']).eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all('pe' in k.split('.')[-1] or 'global_cmvn' in k for k in missing), (missing, unexpected)
    feats, flens, prefixes, plens = recipe_inputs()
    B, N, L = prefixes.shape
    with torch.no_grad():
        memory, mask = m.encoder(torch.from_numpy(feats), torch.from_numpy(flens).long(), -1, -1)
    mem_lens = mask.squeeze(1).sum(1).to(torch.int32)
    out = {}
    for name, dt in (('32', torch.float32), ('64', torch.float64)):
        dec = (m.decoder.double() if dt == torch.float64 else m.decoder).left_decoder
        rows = np.zeros((B, N, V), np.float64 if dt == torch.float64 else np.float32)
        for b in range(B):
            T = int(mem_lens[b])
            mem = memory[b:b + 1, :T].to(dt)
            mem_mask = torch.ones(1, 1, T, dtype=torch.bool)
            for n in range(N):
                n_in = int(plens[b, n]) + 1
                tgt = torch.full((1, n_in), V - 1, dtype=torch.long)
                tgt[0, 1:] = torch.from_numpy(prefixes[b, n, :n_in - 1].astype(np.int64))
                tgt_mask = torch.tril(torch.ones(n_in, n_in, dtype=torch.bool)).unsqueeze(0)
                with torch.no_grad():
                    y, _ = dec.forward_one_step(mem, mem_mask, tgt, tgt_mask, None)
                rows[b, n] = y[0].numpy()
        out['logp' + name] = rows
    # search traces: the three utterances, and utterance 2 again with eos made likely
    cases = [(b, 0.0) for b in range(B)] + [(2, EOS_BIAS)]
    smax = int(mem_lens.max())
    for name, dt in (('32', torch.float32), ('64', torch.float64)):
        dec = (m.decoder.double() if dt == torch.float64 else m.decoder.float()).left_decoder
        par = np.full((len(cases), smax, BEAM), -1, np.int32)
        tok = np.full((len(cases), smax, BEAM), -1, np.int32)
        sco = np.zeros((len(cases), smax, BEAM), np.float64 if dt == torch.float64 else np.float32)
        steps = np.zeros(len(cases), np.int32)
        for c, (b, bias) in enumerate(cases):
            with torch.no_grad():
                dec.output_layer.bias[V - 1] += bias
            trace = beam_loop(dec, memory[b:b + 1, :int(mem_lens[b])].to(dt), BEAM, V)
            with torch.no_grad():
                dec.output_layer.bias[V - 1] -= bias
            steps[c] = len(trace)
            for k, (p_, t_, s_) in enumerate(trace):
                par[c, k], tok[c, k], sco[c, k] = p_, t_, s_
        out.update({'trace_parents' + name: par, 'trace_tokens' + name: tok, 'trace_scores' + name: sco, 'trace_steps' + name: steps})
    out['trace_cases'] = np.array([[b, bias] for b, bias in cases], np.float64)
    path = os.path.join(ROOT, 'tests', 'golden', 'attention_decode_v50.npz')
    # the positional rows the model added (float32 sin / cos differ by an ulp between CPUs: the record keeps its own)
    pe = dec.embed[1].pe[0, :smax + 2].float().numpy()
    np.savez_compressed(path, recipe=json.dumps(RECIPE), feats=feats, feat_lens=flens, memory=memory.numpy(),
                        mem_lens=mem_lens.numpy(), prefixes=prefixes, prefix_lens=plens, pe=pe, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    for k, v in out.items():
        print(k, v.dtype, v.reshape(-1)[:4])


if __name__ == '__main__':
    main()
