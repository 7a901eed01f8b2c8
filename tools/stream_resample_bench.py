"""What resampling off-rate STREAMING sessions on the device buys (GPU box): ``StreamPool`` steps of N sessions, each fed one 0.64 s
chunk of mono int16 PCM per step, at 8 / 44.1 / 48 kHz -- with the device path (``masr_pool_step_rates``: one resample_feeds
launch inside the step) and with MASR_DEVICE_RESAMPLE=0 (``AudioSegment.resample`` per chunk on the host, as before) -- and at
16 kHz, the floor: the same step with nothing to resample.

Per (sessions, rate): host clock around feed-all + step (the step ends in the wait for its results), median and min / max over
``runs`` x ``steps`` timed steps behind ``warmup`` untimed ones per run (sessions are reset between runs: a stream holds 20 such
chunks); audio-s/s = sessions x 0.64 / median; and the resample_feeds launch of such a step alone between two HIP events.

usage: python tools/stream_resample_bench.py --sessions 16 [--rates 16000,8000,44100,48000] [--runs 3] [--steps 10] [--warmup 3]
                                             [--out results.jsonl]
       python tools/stream_resample_bench.py --table results.jsonl [--markdown OUT.md]
One JSON line per (sessions, rate); ``--table`` turns the collected lines into the markdown table."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK_S, MODEL_RATE = 0.64, 16000


def step_ms(pool, handles, chunks, rate, runs, steps, warmup):
    import torch
    times = []
    for _ in range(runs):
        for h in handles:
            pool.reset(h)
        for k in range(warmup + steps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for i, h in enumerate(handles):
                pool.feed(h, chunks[i][k], sample_rate=rate)
            out = pool.step()
            dt = (time.perf_counter() - t) * 1e3
            assert len(out) == len(handles)
            if k >= warmup:
                times.append(dt)
    return times


def kernel_ms(eng, n, rate, reps=20):
    """the resample_feeds launch of one step (n int16 feeds of 0.64 s, one per row) alone, between two events -> (median, min)"""
    import torch
    from masr_amd import _lib
    from masr_amd.data_utils.resample import resampled_length
    n_in = int(CHUNK_S * rate)
    n_out = resampled_length(n_in, rate, MODEL_RATE)
    feeds = np.array([(2 * n_in * i, 0, n_in, n_out, i, 37, 0) for i in range(n)], _lib.RESAMPLE_FEED)
    rates = np.array([eng.resample_rate(rate, MODEL_RATE)], _lib.RESAMPLE_RATE)
    src = torch.from_numpy(np.random.default_rng(rate).integers(-3000, 3000, n * n_in).astype(np.int16).view(np.uint8)).to(eng.device)
    out = torch.zeros(n, n_out + 400, dtype=torch.float32, device=eng.device)
    tiles = eng.resample_plan(feeds, rates, src.numel(), n, out.shape[1])
    # the tables go up ONCE; between the events there is the C entry alone (its host-side checks run ahead of the launch and
    # overlap nothing: the events bracket what the stream executes)
    dev = [eng.to_device(a.view(np.uint8)) for a in (feeds, rates, tiles)]
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    dptr = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch():
        _lib.check(eng.lib.masr_resample_feeds(eng.h, dptr(src), src.numel(), ptr(feeds), dptr(dev[0]), n, ptr(rates), dptr(dev[1]), 1,
                                               ptr(tiles), dptr(dev[2]), tiles.shape[0], dptr(out), n, out.shape[1], stream))
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def table(path, markdown):
    rows = [json.loads(line) for line in open(path) if line.strip().startswith('{')]
    floor = {r['sessions']: r for r in rows if r['rate'] == MODEL_RATE}
    head = ['sessions', 'source rate', 'device path: ms / step (min - max)', 'audio-s/s', 'MASR_DEVICE_RESAMPLE=0: ms / step (min - max)',
            'audio-s/s', 'kernel per step (ms)', 'same results']
    lines = ['| ' + ' | '.join(head) + ' |', '|' + '---|' * len(head)]
    fmt = lambda r, k: f"{r[k + '_ms']:.2f} ({r[k + '_min_ms']:.2f} - {r[k + '_max_ms']:.2f})"
    for r in rows:
        if r['rate'] == MODEL_RATE:
            cells = [str(r['sessions']), '16000 Hz (floor)', fmt(r, 'device'), f"{r['device_audio_s_per_s']:.0f}", '--', '--', '--', '--']
        else:
            cells = [str(r['sessions']), f"{r['rate']} Hz", fmt(r, 'device'), f"{r['device_audio_s_per_s']:.0f}", fmt(r, 'host'),
                     f"{r['host_audio_s_per_s']:.0f}", f"{r['kernel_ms']:.3f} (min {r['kernel_min_ms']:.3f})",
                     'yes' if r['same_results'] else 'NO']
        lines.append('| ' + ' | '.join(cells) + ' |')
    lines.append('')
    if rows:
        r = rows[0]
        lines.append(f"One 0.64 s chunk of mono int16 PCM per session and step; medians over {r['runs']} runs x {r['steps']} timed steps "
                     f"(host path: {r['host_runs']} run) behind {r['warmup']} untimed ones per run, host clock around feed + step; kernel: "
                     "median of 20 launches between two events.  audio-s/s = sessions x 0.64 s / median step.")
    for n, f in sorted(floor.items()):
        lines.append(f"Floor, {n} sessions at 16 kHz: {f['device_ms']:.2f} ms / step, {f['device_audio_s_per_s']:.0f} audio-s/s.")
    text = '\n'.join(lines)
    print(text)
    if markdown:
        with open(markdown, 'w') as f:
            f.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sessions', type=int, default=16)
    ap.add_argument('--rates', default='16000,8000,44100,48000')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--host-runs', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--table', default=None)
    ap.add_argument('--markdown', default=None)
    args = ap.parse_args()
    if args.table:
        return table(args.table, args.markdown)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('stream_resample_bench: no GPU -- nothing here can be measured without one')
    import bench
    from masr_amd.data_utils import resample as rs
    from masr_amd.serving import StreamPool
    from masr_amd.utils import synthetic
    if args.warmup + args.steps > 20:
        raise SystemExit('a stream of max_frames_out=320 holds 20 chunks of 0.64 s: warmup + steps <= 20')
    os.environ.pop('MASR_DEVICE_RESAMPLE', None)
    os.environ.pop('MASR_POOL_PY', None)
    pred = bench.facade('conformer', 'ctc_greedy', 0)
    n, total = args.sessions, args.warmup + args.steps
    at16 = synthetic.synthetic_pcm(n, int(total * CHUNK_S * MODEL_RATE), seed=1234)
    for rate in [int(r) for r in args.rates.split(',')]:
        if rate == MODEL_RATE:
            pcm = at16
        else:                                        # the same sessions "recorded" at `rate` (made once, outside the clock)
            pcm = np.stack([np.clip(np.rint(rs.resample_native(x.astype(np.float32) / 32768.0, MODEL_RATE, rate) * 32768.0), -32768,
                                    32767).astype(np.int16) for x in at16])
        m = int(CHUNK_S * rate)
        chunks = [[pcm[i, k * m:(k + 1) * m].tobytes() for k in range(total)] for i in range(n)]
        row = {'sessions': n, 'rate': rate, 'runs': args.runs, 'host_runs': args.host_runs, 'steps': args.steps, 'warmup': args.warmup}

        def measure(runs):
            pool = StreamPool(pred, max_frames_out=320)
            try:
                hs = [pool.open() for _ in range(n)]
                times = step_ms(pool, hs, chunks, rate, runs, args.steps, args.warmup)
                last = [pool.sessions[h].result for h in hs]
                return times, last, pool.device_resampled
            finally:
                pool.shutdown()
        times, dev_last, n_dev = measure(args.runs)
        med = statistics.median(times)
        row.update({'device_ms': round(med, 3), 'device_min_ms': round(min(times), 3), 'device_max_ms': round(max(times), 3),
                    'device_audio_s_per_s': round(n * CHUNK_S / (med / 1e3), 1), 'device_resampled_feeds': n_dev})
        if rate != MODEL_RATE:
            os.environ['MASR_DEVICE_RESAMPLE'] = '0'
            try:
                times, host_last, n_host = measure(args.host_runs)
            finally:
                os.environ.pop('MASR_DEVICE_RESAMPLE', None)
            med = statistics.median(times)
            k_med, k_min = kernel_ms(pred.predictor.engine, n, rate)
            row.update({'host_ms': round(med, 3), 'host_min_ms': round(min(times), 3), 'host_max_ms': round(max(times), 3),
                        'host_audio_s_per_s': round(n * CHUNK_S / (med / 1e3), 1), 'kernel_ms': round(k_med, 4), 'kernel_min_ms': round(k_min, 4),
                        'same_results': dev_last == host_last and n_dev > 0 and n_host == 0})
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
