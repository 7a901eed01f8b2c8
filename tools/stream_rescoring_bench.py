"""What the attention second pass at the end of streaming utterances costs at serving scale (GPU box).

``StreamPool`` steps of N sessions, each fed one 0.64 s chunk of mono int16 PCM at 16 kHz per step over an utterance of
``--seconds`` (the last feed carries ``is_end=True``), on one synthetic Conformer checkpoint with the shipped decoder (3 + 3 blocks,
4 heads, linear_units 1024), for

  ctc_beam_search            alpha = beta = 0, no language model: the first pass alone (this path makes the calls it made before
                             ``on_streams`` existed; the tool runs on an older checkout too, where only this configuration exists)
  attention_rescoring        ``attention_rescoring_decoder_conf.on_streams: 'rescore_at_end'``, the same beam and cutoffs

Per configuration: host clock around feed-all + step (the step ends in the wait for its results) for every step of the utterance
behind ``--warmup`` untimed utterance(s); the median over the steps that end no utterance, and the last step (all N end there) on
its own.  Then the masr_rescore_rows launch alone between two HIP events against masr_rescore on a pre-gathered dense copy: N
utterances with histories of 16 / 250 / 1000 frames, rows scattered over the pool, ``--nbest`` hypotheses of ``--hyp-len`` tokens.

usage: python tools/stream_rescoring_bench.py [--sessions 128] [--seconds 20] [--beam 10] [--runs 1] [--warmup 1] [--out results.jsonl]
One JSON line per configuration and per history length."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK_S, RATE = 0.64, 16000
DEC = dict(linear_units=1024, num_blocks=3, r_num_blocks=3)


def predictor(sd, vocab, decoder, beam, on_streams=True):
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    vpath = os.path.join(tempfile.mkdtemp(prefix='masr_bench_'), 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(vocab):
            f.write(f'{t}\t1\n')
    rconf = {'beam_size': beam, 'cutoff_prob': 0.99, 'cutoff_top_n': 40}
    if on_streams:
        rconf['on_streams'] = 'rescore_at_end'
    cfg = {'encoder_conf': {}, 'decoder_conf': dict(attention_heads=4, **DEC), 'model_conf': {'ctc_weight': 0.3, 'reverse_weight': 0.3},
           'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'attention_rescoring_decoder_conf': rconf,
           'ctc_beam_search_decoder_conf': {'alpha': 0, 'beta': 0, 'beam_size': beam, 'cutoff_prob': 0.99, 'cutoff_top_n': 40,
                                            'num_processes': 10, 'language_model_path': None},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'conformer', 'streaming': True, 'decoder': decoder,
           'metrics_type': 'cer'}
    return MASRPredictor(configs=cfg, use_gpu=True, state_dict=sd)


def utterance_ms(pool, handles, chunks):
    """one utterance on every session, the last feed with is_end -> the milliseconds of each of its steps"""
    import torch
    for h in handles:
        pool.reset(h)
    times, last = [], len(chunks[0]) - 1
    for k in range(last + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i, h in enumerate(handles):
            pool.feed(h, chunks[i][k], k == last)
        out = pool.step()
        times.append((time.perf_counter() - t) * 1e3)
        assert len(out) == len(handles)
    return times


def launch_ms(eng, n, frames, nbest, hyp_len, reps=10):
    """masr_rescore_rows over ``n`` utterances of ``frames`` scattered rows, and masr_rescore on the pre-gathered dense copy, each
    alone between two events, alternating -> ((median, min) ms of the row-table launch, (median, min) ms of the dense launch)"""
    import torch
    rng = np.random.default_rng(frames)
    n_rows = n * frames
    rows = torch.randn(n_rows, eng.d_model, dtype=torch.float32, device=eng.device)
    table = torch.from_numpy(rng.permutation(n_rows).astype(np.int64).reshape(n, frames)).to(eng.device)
    dense = rows[table].contiguous()
    nf = torch.full((n,), frames, dtype=torch.int32, device=eng.device)
    hyps = torch.from_numpy(rng.integers(1, eng.vocab_size - 1, (n, nbest, hyp_len)).astype(np.int32)).to(eng.device)
    lens = torch.from_numpy(rng.integers(hyp_len // 2, hyp_len + 1, (n, nbest)).astype(np.int32)).to(eng.device)
    calls = (lambda: eng.rescore_rows(rows, table, nf, hyps, lens, True), lambda: eng.rescore(dense, nf, hyps, lens, True))
    for fn in calls * 2:
        out = fn()
    torch.cuda.synchronize()
    times = ([], [])
    for _ in range(reps):
        for fn, ts in zip(calls, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
    del out
    return tuple((statistics.median(ts), min(ts)) for ts in times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sessions', type=int, default=128)
    ap.add_argument('--seconds', type=float, default=20.0)
    ap.add_argument('--beam', type=int, default=10)
    ap.add_argument('--vocab', type=int, default=4233)
    ap.add_argument('--runs', type=int, default=1)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--histories', default='16,250,1000')
    ap.add_argument('--nbest', type=int, default=10)
    ap.add_argument('--hyp-len', type=int, default=40)
    ap.add_argument('--configs', default='ctc_beam_search,attention_rescoring')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('stream_rescoring_bench: no GPU -- nothing here can be measured without one')
    from masr_amd.serving import StreamPool
    from masr_amd.utils import synthetic
    os.environ.pop('MASR_POOL_PY', None)
    n, n_steps = args.sessions, int(args.seconds / CHUNK_S)
    m = int(CHUNK_S * RATE)
    pcm = synthetic.synthetic_pcm(n, n_steps * m, seed=1234)
    chunks = [[pcm[i, k * m:(k + 1) * m].tobytes() for k in range(n_steps)] for i in range(n)]
    sd = synthetic.conformer_state_dict(0, args.vocab, decoder=DEC)

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')
    pred = None
    for decoder in args.configs.split(','):
        pred = predictor(sd, args.vocab, decoder, args.beam)
        pool = StreamPool(pred, max_frames_out=512)
        try:
            hs = [pool.open() for _ in range(n)]
            for _ in range(args.warmup):
                utterance_ms(pool, hs, chunks)
            runs = np.array([utterance_ms(pool, hs, chunks) for _ in range(args.runs)])
            per_step = np.median(runs, axis=0)
            mid = per_step[:-1]
            emit({'kind': 'step', 'config': decoder, 'sessions': n, 'seconds': args.seconds, 'n_steps': n_steps, 'beam': args.beam,
                  'runs': args.runs, 'warmup': args.warmup, 'ms': round(float(np.median(mid)), 3), 'min_ms': round(float(mid.min()), 3),
                  'max_ms': round(float(mid.max()), 3), 'end_step_ms': round(float(per_step[-1]), 3),
                  'end_step_all_runs_ms': [round(float(x), 2) for x in runs[:, -1]],
                  'per_step_ms': [round(float(x), 2) for x in per_step],
                  'enc_pool_rows': int(pool._enc.shape[0]) if getattr(pool, 'rescoring', False) else 0})
        finally:
            pool.shutdown()
            del pool
            torch.cuda.empty_cache()
    if pred is not None and pred.configs.decoder == 'attention_rescoring':
        eng = pred.predictor.engine
        for frames in [int(x) for x in args.histories.split(',')]:
            (r_med, r_min), (d_med, d_min) = launch_ms(eng, n, frames, args.nbest, args.hyp_len)
            emit({'kind': 'launch', 'sessions': n, 'frames': frames, 'nbest': args.nbest, 'hyp_len': args.hyp_len,
                  'rescore_rows_ms': round(r_med, 4), 'rescore_rows_min_ms': round(r_min, 4), 'rescore_dense_ms': round(d_med, 4),
                  'rescore_dense_min_ms': round(d_min, 4)})
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
