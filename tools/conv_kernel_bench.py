"""Cost of encoder_conf.cnn_module_kernel off the shipped values: time per call of ``encode_full`` on 32 x 10 s (12 blocks,
V = 4233, synthetic weights) for the Conformer at K = 15 / 31 / 9 and the Squeezeformer at K = 31 / 15, each as a ratio to the
shipped K; and the Conformer at K = 15 / 16 / 14 / 23 with the conv-module head stage switched off (masr_debug_set no_ffn_head = 1), so
that the depthwise kernel runs as its own launch: dwconv_ln_silu_kernel<15, 0> against dwconv_ln_silu_taps_kernel<16, 0> on rows
of the same shape (run the script under a kernel trace to read the two kernels' own times).  Needs a GPU.

usage: python tools/conv_kernel_bench.py [--reps 10] [--only-separate]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                            # noqa: E402
from masr_amd._lib import debug_keys                    # noqa: E402
from masr_amd.engine import HipEngine                   # noqa: E402
from masr_amd.utils import synthetic                    # noqa: E402

V, BLOCKS = 4233, 12


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def engine(family, K):
    if family == 'conformer':
        sd = synthetic.conformer_state_dict(0, V, num_blocks=BLOCKS, kernel=K)
        return HipEngine(sd, {'num_blocks': BLOCKS, 'cnn_module_kernel': K}, vocab_size=V)
    sd = synthetic.squeezeformer_state_dict(0, V, num_blocks=BLOCKS, kernel=K, streaming=True)
    return HipEngine(sd, {'num_blocks': BLOCKS, 'cnn_module_kernel': K}, vocab_size=V, use_model='squeezeformer')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--only-separate', action='store_true', help='the no_ffn_head runs only (for a kernel trace)')
    a = ap.parse_args()
    g = torch.Generator(device='cpu').manual_seed(1)
    feats = (torch.randn(32, 998, 80, generator=g) * 3 + 13).cuda()
    lens = torch.full((32,), 998, dtype=torch.int32, device='cuda')
    runs = (('conformer', (15, 31, 9), {}), ('squeezeformer', (31, 15), {}), ('conformer', (15, 16, 14, 23), {'no_ffn_head': 1}))
    for family, ks, keys in runs[2:] if a.only_separate else runs:
        base = None
        for K in ks:
            e = engine(family, K)
            with debug_keys(e, keys):
                ms = min(timed(lambda: e.encode_full(feats, lens, -1), 3, a.reps) for _ in range(3))
            e.close()
            base = base or ms
            print(json.dumps({'family': family, 'cnn_module_kernel': K, 'keys': keys, 'encode_full_ms': round(ms, 3),
                              'ratio_to_shipped': round(ms / base, 3)}), flush=True)


if __name__ == '__main__':
    main()
