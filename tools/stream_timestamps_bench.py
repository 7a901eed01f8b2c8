"""What token timestamps cost on streaming sessions at serving scale (GPU box): ``StreamPool`` steps of N sessions, each fed one
0.64 s chunk of mono int16 PCM at 16 kHz per step over a 20 s utterance (31 steps), for

  greedy, C step            ``StreamPool(pred)``: masr_pool_step, what a greedy pool runs without the flag
  greedy, python framing    the same with MASR_POOL_PY=1
  greedy, timestamps        ``StreamPool(pred, timestamps=True)``: the python framing + the posterior rows + one masr_ctc_align_rows
  beam, python framing      ``ctc_beam_search`` without the flag
  beam, timestamps          ... and with it

Per configuration: host clock around feed-all + step (the step ends in the wait for its results) for every step of the utterance
behind ``warmup`` untimed utterance(s); the median over all steps, and over the first and the last five (the alignment covers the whole
history, so a step grows with the utterance).  Then the masr_ctc_align_rows launch alone between two HIP events, N utterances with
histories of 16 / 250 / 1000 frames (hypotheses of one token per four frames, rows scattered over the pool), and the device memory the
row pool of the timestamps run reached.

usage: python tools/stream_timestamps_bench.py [--sessions 128] [--seconds 20] [--runs 1] [--warmup 1] [--out results.jsonl]
       python tools/stream_timestamps_bench.py --table results.jsonl [--markdown OUT.md]
One JSON line per configuration and per history length; ``--table`` turns the collected lines into the markdown tables."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK_S, RATE = 0.64, 16000
CONFIGS = [('greedy, C step', 'ctc_greedy', False, False), ('greedy, python framing (MASR_POOL_PY=1)', 'ctc_greedy', False, True),
           ('greedy, timestamps', 'ctc_greedy', True, False), ('beam search, python framing', 'ctc_beam_search', False, False),
           ('beam search, timestamps', 'ctc_beam_search', True, False)]


def utterance_ms(pool, handles, chunks):
    """one utterance on every session -> the milliseconds of each of its steps"""
    import torch
    for h in handles:
        pool.reset(h)
    times = []
    for k in range(len(chunks[0])):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i, h in enumerate(handles):
            pool.feed(h, chunks[i][k])
        out = pool.step()
        times.append((time.perf_counter() - t) * 1e3)
        assert len(out) == len(handles)
    return times


def kernel_ms(eng, n, frames, vocab, reps=10):
    """the masr_ctc_align_rows launch over ``n`` utterances of ``frames`` frames alone, between two events -> (median, min) ms"""
    import torch
    rng = np.random.default_rng(frames)
    n_rows = n * frames
    rows = torch.rand(n_rows, vocab, dtype=torch.float32, device=eng.device) / vocab
    table = torch.from_numpy(rng.permutation(n_rows).astype(np.int64).reshape(n, frames)).to(eng.device)
    L = max(frames // 4, 1)
    tokens = torch.from_numpy(rng.integers(1, vocab, (n, L)).astype(np.int32)).to(eng.device)
    nf = torch.full((n,), frames, dtype=torch.int32, device=eng.device)
    nt = torch.full((n,), L, dtype=torch.int32, device=eng.device)
    out = torch.empty(n * (3 * L + 2), dtype=torch.int32, device=eng.device)
    for _ in range(2):
        eng.ctc_align_rows(rows, table, nf, tokens, nt, out=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.ctc_align_rows(rows, table, nf, tokens, nt, out=out)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def table(path, markdown):
    rows = [json.loads(line) for line in open(path) if line.strip().startswith('{')]
    steps = [r for r in rows if r['kind'] == 'step']
    lines = []
    if steps:
        r = steps[0]
        lines += [f"{r['sessions']} sessions x 0.64 s per step over a {r['seconds']} s utterance ({r['n_steps']} steps), median of "
                  f"{r['runs']} timed utterance(s) behind {r['warmup']} untimed; host clock around feed + step.", '',
                  '| configuration | ms / step, median (min - max) | first 5 steps | last 5 steps | audio-s/s | row pool |',
                  '|---|---|---|---|---|---|']
        for r in steps:
            pool = f"{r['pool_rows']} rows, {r['pool_bytes'] / 2 ** 20:.0f} MiB" if r.get('pool_rows') else '--'
            lines.append(f"| {r['config']} | {r['ms']:.2f} ({r['min_ms']:.2f} - {r['max_ms']:.2f}) | {r['first5_ms']:.2f} | "
                         f"{r['last5_ms']:.2f} | {r['audio_s_per_s']:.0f} | {pool} |")
        lines.append('')
    kern = [r for r in rows if r['kind'] == 'kernel']
    if kern:
        lines += ['| masr_ctc_align_rows alone: utterances | frames each | tokens each | ms, median (min) |', '|---|---|---|---|']
        for r in kern:
            lines.append(f"| {r['sessions']} | {r['frames']} | {r['tokens']} | {r['kernel_ms']:.3f} ({r['kernel_min_ms']:.3f}) |")
    text = '\n'.join(lines)
    print(text)
    if markdown:
        with open(markdown, 'w') as f:
            f.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sessions', type=int, default=128)
    ap.add_argument('--seconds', type=float, default=20.0)
    ap.add_argument('--runs', type=int, default=1)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--histories', default='16,250,1000')
    ap.add_argument('--out', default=None)
    ap.add_argument('--table', default=None)
    ap.add_argument('--markdown', default=None)
    args = ap.parse_args()
    if args.table:
        return table(args.table, args.markdown)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('stream_timestamps_bench: no GPU -- nothing here can be measured without one')
    import bench
    from masr_amd.serving import StreamPool
    from masr_amd.utils import synthetic
    os.environ.pop('MASR_POOL_PY', None)
    n, n_steps = args.sessions, int(args.seconds / CHUNK_S)
    m = int(CHUNK_S * RATE)
    pcm = synthetic.synthetic_pcm(n, n_steps * m, seed=1234)
    chunks = [[pcm[i, k * m:(k + 1) * m].tobytes() for k in range(n_steps)] for i in range(n)]

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')
    preds = {}
    for name, decoder, stamps, py in CONFIGS:
        if decoder not in preds:
            # (beam search without a language model file: the reference's conformer.yml values otherwise)
            conf = {'alpha': 2.2, 'beta': 4.3, 'beam_size': 300, 'cutoff_prob': 0.99, 'cutoff_top_n': 40, 'num_processes': 10,
                    'language_model_path': None}
            preds[decoder] = bench.facade('conformer', decoder, 0, beam_conf=conf if decoder == 'ctc_beam_search' else None)
        if py:
            os.environ['MASR_POOL_PY'] = '1'
        try:
            pool = StreamPool(preds[decoder], max_frames_out=512, **({'timestamps': True} if stamps else {}))
        finally:
            os.environ.pop('MASR_POOL_PY', None)
        try:
            assert (pool.framing == 'c') == (decoder == 'ctc_greedy' and not stamps and not py)
            hs = [pool.open() for _ in range(n)]
            for _ in range(args.warmup):
                utterance_ms(pool, hs, chunks)
            runs = np.array([utterance_ms(pool, hs, chunks) for _ in range(args.runs)])
            per_step = np.median(runs, axis=0)
            med = float(np.median(per_step))
            row = {'kind': 'step', 'config': name, 'sessions': n, 'seconds': args.seconds, 'n_steps': n_steps, 'runs': args.runs,
                   'warmup': args.warmup, 'ms': round(med, 3), 'min_ms': round(float(per_step.min()), 3),
                   'max_ms': round(float(per_step.max()), 3), 'first5_ms': round(float(np.median(per_step[:5])), 3),
                   'last5_ms': round(float(np.median(per_step[-5:])), 3), 'audio_s_per_s': round(n * CHUNK_S / (med / 1e3), 1),
                   'per_step_ms': [round(float(x), 2) for x in per_step]}
            if stamps:
                row.update({'pool_rows': int(pool._post.shape[0]), 'rows_in_use': int(pool._alloc.in_use),
                            'pool_bytes': int(pool._post.numel() * 4),
                            'tokens_last': int(np.median([len(pool.last_tokens(h)) for h in hs]))})
            emit(row)
        finally:
            pool.shutdown()
            del pool
            torch.cuda.empty_cache()
    eng = preds['ctc_greedy'].predictor.engine
    for frames in [int(x) for x in args.histories.split(',')]:
        k_med, k_min = kernel_ms(eng, n, frames, eng.vocab_size)
        emit({'kind': 'kernel', 'sessions': n, 'frames': frames, 'tokens': max(frames // 4, 1), 'kernel_ms': round(k_med, 4),
              'kernel_min_ms': round(k_min, 4)})
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
