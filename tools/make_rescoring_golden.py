"""Writes tests/golden/rescoring_v50.npz: the attention decoder of the LIVE reference model on fixed hypothesis tables.

    python tools/make_rescoring_golden.py [path of the reference checkout]

Builds the reference ``ConformerModel`` on the CPU from the seeded synthetic weights of ``masr_amd/utils/synthetic.py`` (V = 50,
2 encoder blocks, decoder 2 + 2 blocks, 4 heads, linear_units 384), runs its encoder on fixed features and ``model.decoder(...)``
(BiTransformerDecoder.forward) on fixed hypothesis tables, in float32 and -- the same module converted with ``.double()``, on the
float32 encoder output -- in float64.  Only recorded data goes into the file: the inputs, the encoder output, the tables and
att / r_att = sum over the L + 1 positions of log_softmax(logits)[target] of both decoders."""
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
HYP_LENS = [[0, 1, 15, 17], [17, 0, 15, 1], [1, 17, 0, 15]]


def recipe_inputs():
    """the fixed features and hypothesis tables (seeded; no reference needed)"""
    rng = np.random.default_rng(7)
    T = max(FEAT_LENS)
    feats = (rng.standard_normal((len(FEAT_LENS), T, 80)) * 3 + 13).astype(np.float32)
    for b, n in enumerate(FEAT_LENS):
        feats[b, n:] = 0
    V, Lmax = RECIPE['vocab_size'], max(max(r) for r in HYP_LENS)
    hyps = np.zeros((len(HYP_LENS), len(HYP_LENS[0]), Lmax), np.int32)
    for b, row in enumerate(HYP_LENS):
        for n, L in enumerate(row):
            hyps[b, n, :L] = rng.integers(1, V - 1, L)
    hyps[0, 2, :15] = V - 2                     # a hypothesis made only of the last ordinary token
    hyps[1, 0, 16] = V - 2                      # ... and one ending in it
    return feats, np.array(FEAT_LENS, np.int32), hyps, np.array(HYP_LENS, np.int32)


def sums(logits, targets, lens):
    lp = torch.log_softmax(logits, dim=-1)
    out = []
    for s in range(logits.shape[0]):
        acc = torch.zeros((), dtype=logits.dtype)
        for p in range(int(lens[s])):
            acc = acc + lp[s, p, targets[s, p]]
        out.append(acc)
    return torch.stack(out)


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
    feats, flens, hyps, hlens = recipe_inputs()
    B, N, Lmax = hyps.shape
    with torch.no_grad():
        memory, mask = m.encoder(torch.from_numpy(feats), torch.from_numpy(flens).long(), -1, -1)
    mem_lens = mask.squeeze(1).sum(1).to(torch.int32)
    S, Lp, sos = B * N, Lmax + 1, V - 1
    ys_in, r_ys_in = torch.full((S, Lp), sos, dtype=torch.long), torch.full((S, Lp), sos, dtype=torch.long)
    tgt, r_tgt = torch.full((S, Lp), sos, dtype=torch.long), torch.full((S, Lp), sos, dtype=torch.long)
    for s in range(S):
        L = int(hlens.reshape(-1)[s])
        h = torch.from_numpy(hyps.reshape(S, Lmax)[s, :L].astype(np.int64))
        ys_in[s, 1:L + 1], tgt[s, :L] = h, h
        r_ys_in[s, 1:L + 1], r_tgt[s, :L] = h.flip(0), h.flip(0)
    in_lens = torch.from_numpy(hlens.reshape(-1).astype(np.int64)) + 1
    out = {}
    for name, dt in (('32', torch.float32), ('64', torch.float64)):
        dec = m.decoder.double() if dt == torch.float64 else m.decoder
        mem = memory.to(dt).repeat_interleave(N, 0)
        with torch.no_grad():
            l_x, r_x, _ = dec(mem, mask.repeat_interleave(N, 0), ys_in, in_lens, r_ys_in, 0.3)
        out['att' + name] = sums(l_x, tgt, in_lens).numpy().reshape(B, N)
        out['r_att' + name] = sums(r_x, r_tgt, in_lens).numpy().reshape(B, N)
    path = os.path.join(ROOT, 'tests', 'golden', 'rescoring_v50.npz')
    np.savez_compressed(path, recipe=json.dumps(RECIPE), feats=feats, feat_lens=flens, memory=memory.numpy(),
                        mem_lens=mem_lens.numpy(), hyps=hyps, hyp_lens=hlens, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    for k, v in out.items():
        print(k, v.dtype, v.reshape(-1)[:4])


if __name__ == '__main__':
    main()
