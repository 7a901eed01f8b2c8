"""The Conformer with each ``activation_type`` (d_ff 2048, 12 blocks, V = 4233, synthetic weights): time per call of
``encode_full`` on 32 x 10 s.  At 256 / 4 swish runs the fused row-block kernels and every other activation the width-generic
layer of separate launches; swish at 512 / 8 (the same generic layer) is printed for scale.  Best of three means of 10 calls, host
clock around calls ending in a device synchronise, after warm-up.  Needs a GPU.

usage: python tools/activation_bench.py [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                            # noqa: E402
from masr_amd.engine import ACTIVATION_TYPES, HipEngine  # noqa: E402
from masr_amd.utils import synthetic                    # noqa: E402

V, BLOCKS, DFF = 4233, 12, 2048


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def bench(act, d, heads, feats, lens):
    sd = synthetic.conformer_state_dict(0, V, d=d, heads=heads, d_ff=DFF, num_blocks=BLOCKS)
    e = HipEngine(sd, {'output_size': d, 'attention_heads': heads, 'linear_units': DFF, 'num_blocks': BLOCKS,
                       'activation_type': act}, vocab_size=V)
    full = lambda: e.encode_full(feats, lens, -1)       # noqa: E731
    ms = min(timed(full, 3, 10) for _ in range(3))
    e.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    a = ap.parse_args()
    g = torch.Generator(device='cpu').manual_seed(1)
    feats = (torch.randn(32, 998, 80, generator=g) * 3 + 13).cuda()
    lens = torch.full((32,), 998, dtype=torch.int32, device='cuda')
    rows = [('swish', 256, 'fused row-block kernels', bench('swish', 256, 4, feats, lens))]
    rows += [(act, 256, 'width-generic layer', bench(act, 256, 4, feats, lens)) for act in ACTIVATION_TYPES if act != 'swish']
    rows += [('swish', 512, 'width-generic layer', bench('swish', 512, 8, feats, lens)),
             ('gelu', 512, 'width-generic layer', bench('gelu', 512, 8, feats, lens))]
    base = rows[0][3]
    text = ['| activation_type | output_size | layer | ms per encode_full (32 x 10 s) | ratio to swish at 256 |', '|---|---|---|---|---|']
    text += [f'| {act} | {d} | {path} | {ms:.3f} | {ms / base:.2f} |' for act, d, path, ms in rows]
    print('\n'.join(text))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(text) + '\n')


if __name__ == '__main__':
    main()
