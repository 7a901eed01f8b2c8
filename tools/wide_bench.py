"""The Conformer at output_size 512 / attention_heads 8 next to the 256 / 4 engine (d_ff 2048, 12 blocks, V = 4233, synthetic
weights): time per call of ``encode_full`` on 32 x 10 s and of a chunk step of 128 streams (67-frame windows), the share of
each kernel class in the call (HIP events through masr_profile_*, tools/kernel_times.py style) and the achieved TFLOP/s from
``oracle.conformer.conformer_flops``.  Needs a GPU.

usage: python tools/wide_bench.py [--out profiles/r10_wide.md] [--label TEXT] [--widths 512,256]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                            # noqa: E402
from masr_amd.engine import HipEngine                   # noqa: E402
from masr_amd.utils import synthetic                    # noqa: E402
from oracle.conformer import conformer_flops            # noqa: E402

V, BLOCKS, DFF = 4233, 12, 2048
# masr_profile_select classes (include/masr_hip.h); 9-12 are the row kernels of csrc/wide.hip and time nothing on the 256 engine
KINDS = ((1, 'all GEMM'), (2, 'of which FFN'), (3, 'of which conv2'), (4, 'attention'), (9, 'wide LayerNorm'), (10, 'wide GLU'),
         (11, 'wide dwconv+LN+SiLU'), (12, 'wide conv_hist + kv_append'))
SUMMED = (1, 4, 9, 10, 11, 12)        # disjoint classes: the rest of the call is 'other'


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def shares(e, fn, reps):
    """{kernel class: ms per call} by HIP events around every launch of the class (a run of its own per class)"""
    out = {}
    for kind, name in KINDS:
        e.profile_select(kind)
        e.profile_read(reset=True)
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ms, _, _ = e.profile_read(reset=True)
        out[name] = ms / reps
    e.profile_select(0)
    return out


def bench(d, heads):
    sd = synthetic.conformer_state_dict(0, V, d=d, heads=heads, d_ff=DFF, num_blocks=BLOCKS)
    e = HipEngine(sd, {'output_size': d, 'attention_heads': heads, 'linear_units': DFF, 'num_blocks': BLOCKS}, vocab_size=V)
    rows = []
    # encode_full: 32 utterances of 10 s = 998 feature frames
    g = torch.Generator(device='cpu').manual_seed(1)
    feats = (torch.randn(32, 998, 80, generator=g) * 3 + 13).cuda()
    lens = torch.full((32,), 998, dtype=torch.int32, device='cuda')
    full = lambda: e.encode_full(feats, lens, -1)       # noqa: E731
    ms = timed(full, 3, 10)
    fl = conformer_flops(998, V=V, d=d, d_ff=DFF, L=BLOCKS, batch=32) - 32 * 2 * d * V * 249      # (no CTC head in encode_full)
    rows.append(('encode_full 32 x 10 s', ms, fl, shares(e, full, 3)))
    # chunk step: 128 streams in lock-step, 67-frame windows (16 encoder frames per step)
    sids = [e.stream_open(0) for _ in range(128)]
    win = (torch.randn(128, 67, 80, generator=g) * 3 + 13).cuda()
    step = lambda: e.encode_chunk(sids, win, want_probs=False, want_argmax=True)      # noqa: E731
    ms = timed(step, 4, 12)
    # (conformer_flops counts attention over the window's own 16 keys; the cached keys of the timed steps, 64-384, are not in it)
    fl = conformer_flops(67, V=V, d=d, d_ff=DFF, L=BLOCKS, batch=128)
    rows.append(('chunk step 128 streams', ms, fl, shares(e, step, 3)))
    for s in sids:
        e.stream_close(s)
    e.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--label', default='')
    ap.add_argument('--widths', default='512,256')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'wide_bench needs a GPU'
    lines = [f'### {a.label or "wide_bench"} ({torch.cuda.get_device_name(0)})', '',
             '| engine | call | ms per call | TFLOP/s (algorithmic) | ' + ' | '.join(f'{n} ms' for _, n in KINDS) + ' | other ms |',
             '|---|---|---|---|' + '---|' * (len(KINDS) + 1)]
    for d in (int(w) for w in a.widths.split(',')):
        for name, ms, fl, sh in bench(d, d // 64):
            other = ms - sum(sh[n] for k, n in KINDS if k in SUMMED)
            lines.append(f'| {d} / {d // 64} | {name} | {ms:.3f} | {fl / ms / 1e9:.1f} | ' +
                         ' | '.join(f'{sh[n]:.3f}' for _, n in KINDS) + f' | {other:.3f} |')
    lines += ['', '"other" = the call minus the classes listed (at 256: the LayerNorm, depthwise and cache kernels of that path, which '
              'have no class; at both widths conv1, softmax, descriptor kernels and the gaps between launches).  The per-class '
              'figures come from runs with events around every launch of the class, which add ~6 us of stream time per launch, '
              'so a class of many short launches reads high and "other" can come out negative.', '']
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a', encoding='utf-8') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
