"""What token timestamps cost: per-call time of ``predict_batch`` with and without ``timestamps=True`` for each decoder, and the
alignment kernel alone.

    python tools/align_bench.py                         # (a) + (b): conformer 32 x 10 s for the four decoders, squeezeformer_b64_beam
    python tools/align_bench.py --no-timestamps         # (a) only: runs on a commit without the argument too (the parent, twice,
                                                        #     gives the run-to-run spread "no difference" is judged against)
    python tools/align_bench.py --kernel                # (c): masr_ctc_align alone on the contract shape, for
                                                        #     rocprofv3 --kernel-trace --stats -- python tools/align_bench.py --kernel

Every figure is the median over ``--calls`` timed calls behind ``--warmup`` untimed ones (the caching allocator's per-stream pools
settle with the third call), with the 10th / 90th percentile beside it; one JSON line per case."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOCAB = 4233
DECODER = dict(linear_units=1024, num_blocks=3, r_num_blocks=3)


def predictor(use_model, decoder, streaming=True, beam_conf=None):
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    d = tempfile.mkdtemp(prefix='masr_align_')
    vpath = os.path.join(d, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(VOCAB):
            f.write(f'{t}\t1\n')
    with_decoder = decoder in ('attention', 'attention_rescoring')
    if use_model == 'conformer':
        sd = synthetic.conformer_state_dict(0, VOCAB, decoder=DECODER if with_decoder else None)
    else:
        sd = synthetic.squeezeformer_state_dict(0, VOCAB)
    cfg = {'encoder_conf': {}, 'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                                                   'use_dB_normalization': True, 'target_dB': -20},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': use_model, 'streaming': streaming, 'decoder': decoder,
           'metrics_type': 'cer'}
    if with_decoder:
        cfg['decoder_conf'] = dict(attention_heads=4, **DECODER)
        cfg['model_conf'] = {'ctc_weight': 0.3, 'reverse_weight': 0.3}
    if beam_conf:
        cfg['ctc_beam_search_decoder_conf'] = beam_conf
    return MASRPredictor(configs=cfg, use_gpu=True, state_dict=sd)


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms)
    return {'median_ms': round(float(np.median(ms)), 3), 'p10_ms': round(float(np.percentile(ms, 10)), 3),
            'p90_ms': round(float(np.percentile(ms, 90)), 3), 'calls': calls}


def case(name, pred, audio, args, **kw):
    line = {'case': name, 'off': timed(lambda: pred.predict_batch(audio, **kw), args.calls, args.warmup)}
    if not args.no_timestamps:
        line['on'] = timed(lambda: pred.predict_batch(audio, timestamps=True, **kw), args.calls, args.warmup)
        line['added_ms'] = round(line['on']['median_ms'] - line['off']['median_ms'], 3)
        res = pred.predict_batch(audio, timestamps=True, **kw)
        line['tokens_per_utterance'] = round(float(np.mean([len(r['tokens'] or []) for r in res])), 1)
        line['unaligned'] = sum(r['tokens'] is None for r in res)
    print(json.dumps(line), flush=True)


def kernel_alone(args):
    """masr_ctc_align on the contract shape: B = 32, T' = 249, the vocabulary of 4233, hypotheses of ``--tokens`` tokens"""
    from masr_amd.engine import HipEngine
    eng = HipEngine(None, vocab_size=VOCAB)
    rng = np.random.default_rng(0)
    B, Tp, L = 32, 249, args.tokens
    post = torch.softmax(torch.from_numpy(rng.standard_normal((B, Tp, VOCAB)).astype(np.float32) * 4).to(eng.device), dim=-1)
    tokens = torch.from_numpy(rng.integers(1, VOCAB, (B, L)).astype(np.int32)).to(eng.device)
    n_frames = torch.full((B,), Tp, dtype=torch.int32, device=eng.device)
    n_tokens = torch.full((B,), L, dtype=torch.int32, device=eng.device)
    out = timed(lambda: eng.ctc_align(post, n_frames, tokens, n_tokens), args.calls, args.warmup)
    assert int(eng.ctc_align(post, n_frames, tokens, n_tokens)[4].abs().sum()) == 0
    print(json.dumps({'case': f'masr_ctc_align alone B={B} T\'={Tp} V={VOCAB} L={L} (launch + wait)', **out}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-timestamps', action='store_true')
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--tokens', type=int, default=40)
    ap.add_argument('--decoders', default='ctc_greedy,ctc_beam_search,attention_rescoring,attention')
    ap.add_argument('--skip-squeezeformer', action='store_true')
    args = ap.parse_args()
    if args.kernel:
        return kernel_alone(args)
    from masr_amd.utils import synthetic
    pcm = synthetic.synthetic_pcm(32, 160000, seed=1234)
    audio = [pcm[i] for i in range(32)]
    beam = {'alpha': 0, 'beta': 0, 'beam_size': 300, 'cutoff_prob': 0.99, 'cutoff_top_n': 40, 'num_processes': 10,
            'language_model_path': None}
    for decoder in [d for d in args.decoders.split(',') if d]:
        pred = predictor('conformer', decoder, beam_conf=beam if decoder == 'ctc_beam_search' else None)
        case(f'conformer 32 x 10 s {decoder}', pred, audio, args)
        pred.predictor.engine.close()
    if not args.skip_squeezeformer:
        # squeezeformer_b64_beam of bench.py: 64 utterances of 2 - 20 s (seed 1234), passes of 32, beam 300, a character n-gram LM
        from masr_amd.decoders.lm_scorer import write_synthetic_arpa
        rng = np.random.default_rng(1234)
        lens = np.sort(rng.integers(32000, 320001, 64).astype(np.int32))[::-1].copy()
        pcm = synthetic.synthetic_pcm(64, int(lens.max()), seed=1234)
        audio = [pcm[i, :lens[i]] for i in range(64)]
        lm = write_synthetic_arpa(os.path.join(tempfile.mkdtemp(prefix='masr_lm_'), 'lm.arpa'), synthetic.synthetic_vocab(VOCAB), seed=5)
        pred = predictor('squeezeformer', 'ctc_beam_search', streaming=False,
                         beam_conf=dict(beam, alpha=2.2, beta=4.3, language_model_path=lm))
        case('squeezeformer_b64_beam', pred, audio, args, batch_size=32)
        pred.predictor.engine.close()


if __name__ == '__main__':
    main()
