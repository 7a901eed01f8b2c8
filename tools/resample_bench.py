"""What resampling off-rate audio on the device buys (GPU box): 32 x 10 s utterances "recorded" at 8, 44.1 and 48 kHz.

Per rate:
  * the resampling kernel alone, HIP events on its stream (the source rows already on the device);
  * a ``MASRPredictor.predict_batch`` call with the device path (host clock around calls that end in the results' read-back);
  * the same call with MASR_DEVICE_RESAMPLE=0 -- the host path of the commit before the device path existed; with
    ``--parent-predict PATH`` (a ``predict.py`` of that commit) its MASRPredictor is timed beside it, as the cross-check of
    the stand-in;
  * whether both paths return the same results (they must).
and, once, the same call on 16 kHz input: the pass the resampler feeds.

usage: python tools/resample_bench.py [--calls 10] [--host-calls 2] [--rates 8000,44100,48000] [--parent-predict PATH]
       [--markdown OUT.md]
Prints one JSON line per rate and a markdown table."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from masr_amd.utils import synthetic  # noqa: E402

BATCH, SECONDS, MODEL_RATE = 32, 10, 16000


def call_ms(fn, calls, warmup=1):
    """median / min host time of ``fn()`` in ms; ``fn`` ends in a wait for its results"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times)


def kernel_ms(eng, pcm, rate, reps):
    """the launch of ``HipEngine.resample_rows`` alone between two events on the current stream -> (median, min) ms"""
    src = torch.from_numpy(pcm).to(eng.device)
    n_in = [pcm.shape[1]] * pcm.shape[0]
    out = torch.empty(pcm.shape[0], SECONDS * MODEL_RATE, dtype=torch.float32, device=eng.device)
    for _ in range(3):
        eng.resample_rows(src, n_in, rate, MODEL_RATE, out=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.resample_rows(src, n_in, rate, MODEL_RATE, out=out)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--host-calls', type=int, default=2)
    ap.add_argument('--rates', default='8000,44100,48000')
    ap.add_argument('--parent-predict', default=None)
    ap.add_argument('--markdown', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('resample_bench: no GPU -- nothing here can be measured without one')
    os.environ.pop('MASR_DEVICE_RESAMPLE', None)
    pred = bench.facade('conformer', 'ctc_greedy', 0)
    eng = pred.predictor.engine
    parent = None
    if args.parent_predict:
        spec = importlib.util.spec_from_file_location('masr_parent_predict', args.parent_predict)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        ours = sys.modules.get('masr_amd.predict')
        sys.modules['masr_amd.predict'] = mod               # bench.facade builds whatever class that module holds
        try:
            parent = bench.facade('conformer', 'ctc_greedy', 0)
        finally:
            sys.modules['masr_amd.predict'] = ours
        assert type(parent) is mod.MASRPredictor and type(pred) is not type(parent)
    at16 = list(synthetic.synthetic_pcm(BATCH, SECONDS * MODEL_RATE, seed=1234))
    base_med, base_min = call_ms(lambda: pred.predict_batch(at16), args.calls, warmup=2)
    print(json.dumps({'rate': MODEL_RATE, 'predict_batch_ms': round(base_med, 3), 'predict_batch_min_ms': round(base_min, 3)}), flush=True)
    rows = []
    for rate in [int(r) for r in args.rates.split(',')]:
        pcm = synthetic.synthetic_pcm(BATCH, SECONDS * rate, seed=rate)
        audio = list(pcm)
        k_med, k_min = kernel_ms(eng, pcm, rate, 20)
        run = lambda p=pred: p.predict_batch(audio, sample_rate=rate)
        dev_res = run()
        dev_med, dev_min = call_ms(run, args.calls, warmup=1)
        os.environ['MASR_DEVICE_RESAMPLE'] = '0'
        try:
            host_res = run()
            host_med, host_min = call_ms(run, args.host_calls, warmup=0)
        finally:
            os.environ.pop('MASR_DEVICE_RESAMPLE', None)
        row = {'rate': rate, 'kernel_ms': round(k_med, 3), 'kernel_min_ms': round(k_min, 3),
               'predict_batch_device_ms': round(dev_med, 3), 'predict_batch_device_min_ms': round(dev_min, 3),
               'predict_batch_host_ms': round(host_med, 1), 'predict_batch_host_min_ms': round(host_min, 1),
               'same_results': dev_res == host_res}
        if parent is not None:
            par_res = run(parent)
            par_med, par_min = call_ms(lambda: run(parent), args.host_calls, warmup=0)
            row.update({'predict_batch_parent_ms': round(par_med, 1), 'predict_batch_parent_min_ms': round(par_min, 1),
                        'same_results_parent': dev_res == par_res})
        rows.append(row)
        print(json.dumps(row), flush=True)
    head = ['source rate', 'kernel (ms)', 'predict_batch, device path (ms)', 'predict_batch, MASR_DEVICE_RESAMPLE=0 (ms)']
    if parent is not None:
        head.append('predict_batch, parent commit (ms)')
    head.append('same results')
    lines = ['| ' + ' | '.join(head) + ' |', '|' + '---|' * len(head)]
    for r in rows:
        cells = [f"{r['rate']} Hz", f"{r['kernel_ms']:.3f} (min {r['kernel_min_ms']:.3f})",
                 f"{r['predict_batch_device_ms']:.2f} (min {r['predict_batch_device_min_ms']:.2f})",
                 f"{r['predict_batch_host_ms']:.0f} (min {r['predict_batch_host_min_ms']:.0f})"]
        if parent is not None:
            cells.append(f"{r['predict_batch_parent_ms']:.0f} (min {r['predict_batch_parent_min_ms']:.0f})")
        cells.append('yes' if r['same_results'] and r.get('same_results_parent', True) else 'NO')
        lines.append('| ' + ' | '.join(cells) + ' |')
    lines.append('')
    lines.append(f'{BATCH} x {SECONDS} s utterances per call (int16 PCM); medians of {args.calls} calls (device path), {args.host_calls} '
                 f'(host path) and 20 launches (kernel).  The same call on 16 kHz input: {base_med:.2f} ms (min {base_min:.2f}).')
    table = '\n'.join(lines)
    print(table)
    if args.markdown:
        with open(args.markdown, 'w') as f:
            f.write(table + '\n')


if __name__ == '__main__':
    main()
