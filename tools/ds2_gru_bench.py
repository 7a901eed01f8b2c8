"""Time the DeepSpeech2 GRU engine (encoder_conf.use_gru: True) against the LSTM engine in ONE process, alternating, on the two
DeepSpeech2 workloads of bench.py (deepspeech2.yml, streaming: False, V = 4233, synthetic weights):

* ``ds2_testwav_b1``  one test.wav-sized utterance (8.39 s) PCM -> hypothesis row on the host, p50 of 50 calls;
* ``ds2_b32x10s``     32 x 10 s per pass, PCM -> packed hypothesis rows, 5 passes.

``gru_u16`` is the GRU engine with the matrix-core step on 16 units per workgroup (masr_debug_set key 43) instead of 8; it only
differs from ``gru`` where that form runs (4 < B <= 32, here ds2_b32x10s).  Each round times every engine once, the order rotating
from round to round; the medians over the rounds are printed as one JSON line per workload and engine.

    python tools/ds2_gru_bench.py [--rounds 5] [--workloads b1,b32] [--engines lstm,gru,gru_u16] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from masr_amd._lib import debug_keys       # noqa: E402
from masr_amd.engine import HipEngine      # noqa: E402
from masr_amd.utils import synthetic       # noqa: E402

V = 4233
N_10S = 160000


def make(cell):
    sd = synthetic.deepspeech2_state_dict(0, V, bidirectional=True, use_gru=cell == 'gru')
    return HipEngine(sd, encoder_conf={'use_gru': cell == 'gru'}, vocab_size=V, streaming=False, use_model='deepspeech2')


def time_b1(eng, xs, ns):
    def one():
        return eng.to_host(eng.transcribe_rows(xs, ns, True, -20.0, gain_in=eng.host_gains(xs, ns, -20.0)))
    for _ in range(3):
        one()
    lat = []
    for _ in range(50):
        t0 = time.perf_counter()
        one()
        lat.append(time.perf_counter() - t0)
    return float(np.percentile(lat, 50)) * 1e3


def time_b32(eng, pcm, n, steps=5):
    def batch():
        return eng.transcribe_rows(pcm, n, True, -20.0, gain_in=eng.host_gains(pcm, n, -20.0))
    for _ in range(2):
        batch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        rows = batch()
    eng.to_host(rows)
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--workloads', default='b1,b32')
    ap.add_argument('--engines', default='lstm,gru,gru_u16')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    workloads = args.workloads.split(',')
    names = args.engines.split(',')
    engines = {}
    for name in names:
        cell = 'gru' if name.startswith('gru') else 'lstm'
        engines.setdefault(cell, make(cell))
    dev = next(iter(engines.values())).device
    wav = np.load(os.path.join(ROOT, 'tests', 'golden', 'testwav.npz'))['pcm']
    xs = torch.from_numpy(np.ascontiguousarray(wav[None])).to(dev)
    ns = torch.tensor([len(wav)], dtype=torch.int32, device=dev)
    pcm = torch.from_numpy(synthetic.synthetic_pcm(32, N_10S, seed=1234)).to(dev)
    n = torch.full((32,), N_10S, dtype=torch.int32, device=dev)
    res = {(w, name): [] for w in workloads for name in names}
    for r in range(args.rounds):
        order = names[r % len(names):] + names[:r % len(names)]
        for name in order:
            eng = engines['gru' if name.startswith('gru') else 'lstm']
            with debug_keys(eng, {'rnn_mfma_units': 16} if name == 'gru_u16' else {}):
                if 'b1' in workloads:
                    res[('b1', name)].append(time_b1(eng, xs, ns))
                if 'b32' in workloads:
                    res[('b32', name)].append(time_b32(eng, pcm, n))
    lines = []
    for (w, name), ms in res.items():
        med = float(np.median(ms))
        audio_s = len(wav) / 16000.0 if w == 'b1' else 32 * N_10S / 16000.0
        lines.append({'workload': 'ds2_testwav_b1' if w == 'b1' else 'ds2_b32x10s', 'engine': name,
                      'ms_median': round(med, 3), 'ms_rounds': [round(x, 3) for x in ms],
                      'value': round(audio_s / (med * 1e-3), 1), 'unit': 'audio-seconds/sec',
                      'device': torch.cuda.get_device_name(dev)})
    text = '\n'.join(json.dumps(x, ensure_ascii=False) for x in lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    for eng in engines.values():
        eng.close()


if __name__ == '__main__':
    main()
