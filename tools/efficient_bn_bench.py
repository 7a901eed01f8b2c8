"""encode_full of the Conformer and Efficient-Conformer builds with cnn_module_norm layer_norm / batch_norm: ms per call.

Shapes: 32 x 10 s (998 feature frames, ragged lengths of BASELINE configs[1]'s kind) and, for the Efficient Conformer, the
efficient_b256 workload's device work (256 utterances = 8 passes of 32 x 10 s, one "call" = the 8 passes).  12 blocks,
V = 4233, streaming: True, synthetic weights.  Every (family, norm, shape) is warmed up, then the configurations are timed in turn,
REPEATS rounds of CALLS calls each (host clock around calls that end in a device synchronise), so that drift of the box hits all
of them alike; per configuration: median, min and max over the rounds = its run-to-run spread.  A configuration that the library
under test refuses (the Efficient Conformer's batch_norm before this variant existed) is reported as refused.

usage: python tools/efficient_bn_bench.py [--repeats 7] [--calls 20] [--keys no_chain=1] [--only conformer:batch_norm]
       [--skip efficient_conformer:batch_norm]
       (--only: one configuration, e.g. under rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from masr_amd._lib import debug_keys  # noqa: E402
from masr_amd.engine import HipEngine  # noqa: E402
from masr_amd.utils import synthetic  # noqa: E402

V, T = 4233, 998


def engine(family, norm):
    if family == 'conformer':
        sd = synthetic.conformer_state_dict(0, V, cnn_module_norm=norm)
    elif norm == 'layer_norm':
        sd = synthetic.efficient_conformer_state_dict(0, V)
    else:
        sd = synthetic.efficient_conformer_state_dict(0, V, cnn_module_norm=norm)
    return HipEngine(sd, {'cnn_module_norm': norm}, vocab_size=V, streaming=True, use_model=family)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--keys', default='', help='masr_debug_set switches for every call, name=value[,name=value]')
    ap.add_argument('--only', default='', help='family:norm')
    ap.add_argument('--skip', default='', help='family:norm left out (the same set of configurations on both sides of an A/B)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    keys = {k: int(v) for k, v in (kv.split('=') for kv in args.keys.split(',') if kv)}
    rng = np.random.default_rng(1234)
    lens = rng.integers(600, T + 1, 32).astype(np.int32)
    lens[0] = T
    feats = rng.standard_normal((32, T, 80)).astype(np.float32) * 3 + 13
    feats *= (np.arange(T)[None, :, None] < lens[:, None, None])
    feats, lens = torch.from_numpy(feats).cuda(), torch.from_numpy(lens).cuda()
    configs = []
    for family in ('conformer', 'efficient_conformer'):
        for norm in ('layer_norm', 'batch_norm'):
            if (args.only and args.only != f'{family}:{norm}') or args.skip == f'{family}:{norm}':
                continue
            try:
                configs.append((family, norm, engine(family, norm)))
            except Exception as ex:        # noqa: BLE001 (a library that does not know the variant says so in its own words)
                print(json.dumps({'family': family, 'norm': norm, 'refused': str(ex)[:160]}), flush=True)
    shapes = {'b32': 1, 'b256': 8}
    times = {}
    for family, norm, e in configs:
        for shape, passes in shapes.items():
            if shape == 'b256' and family != 'efficient_conformer':
                continue
            times[(family, norm, shape)] = []
    with debug_keys(configs[0][2], **keys):       # (process-wide switches: one block around everything)
        for family, norm, e in configs:           # warm-up: code objects, packed weight copies, workspaces
            for _ in range(3):
                e.encode_full(feats, lens, -1)
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for family, norm, e in configs:
                for shape, passes in shapes.items():
                    if (family, norm, shape) not in times:
                        continue
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.calls * passes):
                        e.encode_full(feats, lens, -1)
                    torch.cuda.synchronize()
                    times[(family, norm, shape)].append(1e3 * (time.perf_counter() - t0) / args.calls)
    for (family, norm, shape), ts in times.items():
        print(json.dumps({'family': family, 'norm': norm, 'shape': shape, 'keys': keys, 'ms_median': round(float(np.median(ts)), 4),
                          'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4), 'rounds': [round(t, 4) for t in ts]}), flush=True)
    for _, _, e in configs:
        e.close()


if __name__ == '__main__':
    main()
