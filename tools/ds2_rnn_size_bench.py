"""Time the DeepSpeech2 recurrence at rnn_size 256 / 512 / 1024 / 2048 (lstm.hip, gru.hip), one engine at a time in ONE process.

* ``step``     per-step time of the recurrence: HIP events around a layer's step loop (masr_profile_select kind 8; the events
               sit on the launch stream, one pair per layer and call), divided by the number of steps.  1-layer engines, V = 50,
               T = 403 feature frames (99 steps), full-length sequences, B in {1, 16, 32}, uni- and bi-directional.  Each point
               is the median over ``--rounds`` rounds of ``--calls`` calls, with the min and max of the rounds as its spread.
* ``units``    the same measurement with the matrix-core step on 8 hidden units per workgroup (masr_debug_set key 43 = -8)
               against the product's 4 where that form runs (B = 16, 32) at rnn_size 256 and 512, alternating in each round,
               and a bit-for-bit comparison of the two outputs.
* ``e2e``      one test.wav-sized utterance (8.39 s), PCM -> hypothesis row on the host, 5 layers, V = 4233, p50 of 30 calls.
* ``encode``   wall time of encode_full (torch events) on the ``step`` shapes at rnn_size 1024: this one also runs on a tree that
               has no profile kind 8, so ``--tree DIR`` measures another checkout of this repository (the parent commit, built
               in DIR, a directory under this repository such as the git-ignored ab/parent) in a child process, alternating
               with this tree, for a same-session A/B.

    python tools/ds2_rnn_size_bench.py [--what step,units,e2e,encode] [--sizes 256,512,1024,2048] [--rounds 5] [--tree DIR]
                                       [--out FILE]

One JSON line per point.  Reads nothing outside the repository (test.wav comes from tests/golden/testwav.npz).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T_FEAT = 403          # ((403 - 1) // 2 - 1) // 2 = 99 steps
STEPS = 99
BATCHES = (1, 16, 32)


def imports(root):
    sys.path.insert(0, root)
    from masr_amd import _lib
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    return _lib, HipEngine, synthetic


def make(HipEngine, synthetic, H, gru, streaming, layers=1, V=50):
    sd = synthetic.deepspeech2_state_dict(0, V, num_rnn_layers=layers, bidirectional=not streaming, use_gru=gru, rnn_size=H)
    conf = {'num_rnn_layers': layers, 'use_gru': gru, 'rnn_size': H}
    return HipEngine(sd, encoder_conf=conf, vocab_size=V, streaming=streaming, use_model='deepspeech2')


def feats(B, dev):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, T_FEAT, 80, generator=g) * 3 + 13).to(dev)
    return x, torch.full((B,), T_FEAT, dtype=torch.int32, device=dev)


def step_us(eng, x, lens, calls):
    """median-of-calls per-step time in microseconds of the step loop (events on the stream around the loop)"""
    for _ in range(3):
        eng.encode_full(x, lens)
    eng.profile_select(8)
    eng.profile_read(True)
    per = []
    for _ in range(calls):
        eng.encode_full(x, lens)
        ms, n, _ = eng.profile_read(True)
        per.append(ms / n / STEPS * 1e3)
    eng.profile_select(0)
    return float(np.median(per))


def encode_ms(eng, x, lens, calls):
    for _ in range(3):
        eng.encode_full(x, lens)
    torch.cuda.synchronize()
    per = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.encode_full(x, lens)
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b))
    return float(np.median(per))


def point(kind, H, gru, streaming, B, vals, unit, **extra):
    d = {'what': kind, 'rnn_size': H, 'cell': 'gru' if gru else 'lstm', 'dir': 'uni' if streaming else 'bi', 'B': B,
         'median': round(float(np.median(vals)), 3), 'min': round(min(vals), 3), 'max': round(max(vals), 3), 'unit': unit,
         'rounds': [round(v, 3) for v in vals]}
    d.update(extra)
    return d


def run_step(mods, sizes, rounds, calls, emit):
    _lib, HipEngine, synthetic = mods
    for H in sizes:
        for gru in (False, True):
            for streaming in (True, False):
                eng = make(HipEngine, synthetic, H, gru, streaming)
                for B in BATCHES:
                    x, lens = feats(B, eng.device)
                    vals = [step_us(eng, x, lens, calls) for _ in range(rounds)]
                    ndir = 1 if streaming else 2
                    mb = ndir * (3 if gru else 4) * H * H * 4 / 1e6
                    emit(point('step', H, gru, streaming, B, vals, 'us/step', whh_MB_per_step=round(mb, 1),
                               whh_GBps=round(mb / np.median(vals) * 1e3, 0)))
                eng.close()


def run_units(mods, sizes, rounds, calls, emit):
    _lib, HipEngine, synthetic = mods
    for H in [h for h in sizes if h <= 512]:
        for gru in (False, True):
            for streaming in (True, False):
                eng = make(HipEngine, synthetic, H, gru, streaming)
                for B in (16, 32):
                    x, lens = feats(B, eng.device)
                    vals, outs = {4: [], 8: []}, {}
                    for r in range(rounds):
                        for u in ((4, 8) if r % 2 == 0 else (8, 4)):
                            with _lib.debug_keys(eng, {'rnn_mfma_units': -8} if u == 8 else {}):
                                vals[u].append(step_us(eng, x, lens, calls))
                                outs[u] = eng.encode_full(x, lens).clone()
                    for u in (8, 4):
                        emit(point('units', H, gru, streaming, B, vals[u], 'us/step', units=u,
                                   workgroups=H // u * (1 if streaming else 2), equal_bits=bool(torch.equal(outs[4], outs[8]))))
                eng.close()


def run_e2e(mods, sizes, rounds, emit):
    _lib, HipEngine, synthetic = mods
    wav = np.load(os.path.join(ROOT, 'tests', 'golden', 'testwav.npz'))['pcm']
    for H in sizes:
        for gru in (False, True):
            for streaming in (True, False):
                eng = make(HipEngine, synthetic, H, gru, streaming, layers=5, V=4233)
                xs = torch.from_numpy(np.ascontiguousarray(wav[None])).to(eng.device)
                ns = torch.tensor([len(wav)], dtype=torch.int32, device=eng.device)

                def one():
                    return eng.to_host(eng.transcribe_rows(xs, ns, True, -20.0, gain_in=eng.host_gains(xs, ns, -20.0)))
                vals = []
                for _ in range(rounds):
                    for _ in range(3):
                        one()
                    lat = []
                    for _ in range(30):
                        t0 = time.perf_counter()
                        one()
                        lat.append(time.perf_counter() - t0)
                    vals.append(float(np.percentile(lat, 50)) * 1e3)
                emit(point('e2e_testwav', H, gru, streaming, 1, vals, 'ms/call', audio_s=round(len(wav) / 16000.0, 2)))
                eng.close()


def run_encode(mods, calls, emit, tag):
    """one pass over the 1024 shapes; the parent process alternates trees and gathers the rounds"""
    _lib, HipEngine, synthetic = mods
    for gru in (False, True):
        for streaming in (True, False):
            eng = make(HipEngine, synthetic, 1024, gru, streaming)
            for B in BATCHES:
                x, lens = feats(B, eng.device)
                emit({'what': 'encode', 'tree': tag, 'rnn_size': 1024, 'cell': 'gru' if gru else 'lstm',
                      'dir': 'uni' if streaming else 'bi', 'B': B, 'ms': round(encode_ms(eng, x, lens, calls), 4)})
            eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='step,units,e2e,encode')
    ap.add_argument('--sizes', default='256,512,1024,2048')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--tree', default='', help='another checkout of this repository (built) for the encode A/B')
    ap.add_argument('--out', default='')
    ap.add_argument('--encode-child', default='', help=argparse.SUPPRESS)
    args = ap.parse_args()
    lines = []

    def emit(d):
        print(json.dumps(d, ensure_ascii=False), flush=True)
        lines.append(d)

    if args.encode_child:                      # child of the encode A/B: one pass on the tree given
        tag, root = args.encode_child.split('=', 1)
        run_encode(imports(root), args.calls, emit, tag)
        return
    what = args.what.split(',')
    sizes = [int(s) for s in args.sizes.split(',')]
    if 'encode' in what:
        # every pass is a fresh process (the two trees load different libraries); this process has not touched the GPU yet
        other = os.path.abspath(args.tree) if args.tree else ''
        if other and os.path.commonpath([other, ROOT]) != ROOT:
            ap.error('--tree must be a directory under this repository')
        trees = [('this', ROOT)] + ([('other', other)] if other else [])
        passes = {}
        for r in range(args.rounds):
            for tag, root in (trees if r % 2 == 0 else trees[::-1]):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), '--encode-child', f'{tag}={root}', '--calls',
                                      str(max(args.calls, 10))], check=True, capture_output=True, text=True, timeout=300).stdout
                for ln in out.splitlines():
                    if ln.startswith('{'):
                        d = json.loads(ln)
                        passes.setdefault((d['tree'], d['cell'], d['dir'], d['B']), []).append(d['ms'])
        for (tag, cell, dr, B), vals in passes.items():
            emit(point('encode_full', 1024, cell == 'gru', dr == 'uni', B, vals, 'ms/call', tree=tag))
    rest = [w for w in what if w != 'encode']
    if rest:
        mods = imports(ROOT)
        if 'step' in rest:
            run_step(mods, sizes, args.rounds, args.calls, emit)
        if 'units' in rest:
            run_units(mods, sizes, args.rounds, args.calls, emit)
        if 'e2e' in rest:
            run_e2e(mods, sizes, min(args.rounds, 3), emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(json.dumps(x, ensure_ascii=False) for x in lines) + '\n')


if __name__ == '__main__':
    main()
