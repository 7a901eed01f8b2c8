"""Times the second pass of ``decoder: attention_rescoring`` beside the encoder pass it follows.

    python tools/rescoring_bench.py [--batch 32] [--seconds 10] [--nbest 10] [--hyp-len 40] [--runs 20] [--vocab 4233]

Synthetic Conformer checkpoint with the shipped decoder (3 + 3 blocks, 4 heads, linear_units 1024), ``batch`` utterances of
``seconds`` s, ``nbest`` random hypotheses of ``hyp-len`` tokens each.  Per run, alternating: the encoder pass (masr_encode_full)
and the rescoring pass (masr_rescore, both decoders), each timed with events on the stream; prints medians, min / max and the
run count as one JSON line.  The per-kernel split comes from a kernel trace of this script (``--runs 5`` under a tracer).

    python tools/rescoring_bench.py --predict-batch

times ``MASRPredictor.predict_batch`` with the decoder on one lane and on two instead."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--nbest', type=int, default=10)
    ap.add_argument('--hyp-len', type=int, default=40)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--vocab', type=int, default=4233)
    a = ap.parse_args()
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    dec = dict(linear_units=1024, num_blocks=3, r_num_blocks=3)
    sd = synthetic.conformer_state_dict(0, a.vocab, decoder=dec)
    eng = HipEngine(sd, vocab_size=a.vocab, attention_decoder=True, decoder_conf=dict(attention_heads=4, **dec))
    n = int(a.seconds * 16000)
    pcm = torch.from_numpy(synthetic.synthetic_pcm(a.batch, n, seed=3)).to(eng.device)
    ns = torch.full((a.batch,), n, dtype=torch.int32, device=eng.device)
    feats, frames = eng.fbank_batch(pcm, ns)
    enc_lens = eng.enc_frames(frames).to(torch.int32).contiguous()
    rng = np.random.default_rng(1)
    hyps = torch.from_numpy(rng.integers(1, a.vocab - 1, (a.batch, a.nbest, a.hyp_len)).astype(np.int32)).to(eng.device)
    lens = torch.from_numpy(rng.integers(a.hyp_len // 2, a.hyp_len + 1, (a.batch, a.nbest)).astype(np.int32)).to(eng.device)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1), out
    enc = None
    t_enc, t_res = [], []
    for k in range(a.runs + 3):
        te, enc = timed(lambda: eng.encode_full(feats, frames, -1))
        tr, _ = timed(lambda: eng.rescore(enc, enc_lens, hyps, lens, True))
        if k >= 3:                       # three warm-up rounds (workspaces, clocks)
            t_enc.append(te)
            t_res.append(tr)
    stat = lambda v: {'median_ms': float(np.median(v)), 'min_ms': float(min(v)), 'max_ms': float(max(v))}
    print(json.dumps({'batch': a.batch, 'seconds': a.seconds, 'nbest': a.nbest, 'hyp_len': a.hyp_len, 'runs': a.runs,
                      'encoder_pass': stat(t_enc), 'rescoring_pass': stat(t_res), 'decoder': eng.decoder_info()}))
    eng.close()


def predict_batch_lanes(runs=10, batch=32, passes=2, seconds=10.0, vocab=4233, nbest=10, first_pass='host'):
    """``predict_batch`` of ``passes`` x ``batch`` utterances with ``decoder: attention_rescoring`` (passes of ``batch``), on one
    lane and on two (MASR_LANES, read per call), alternating; host wall time per call -> one JSON line.  ``first_pass``: 'host' or
    'gpu' (``--first-pass gpu``: attention_rescoring_decoder_conf.first_pass)"""
    import tempfile
    import time
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    dec = dict(linear_units=1024, num_blocks=3, r_num_blocks=3)
    sd = synthetic.conformer_state_dict(0, vocab, decoder=dec)
    vpath = os.path.join(tempfile.mkdtemp(), 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(vocab):
            f.write(f'{t}\t1\n')
    cfg = {'encoder_conf': {}, 'decoder_conf': dict(attention_heads=4, **dec), 'model_conf': {'ctc_weight': 0.3, 'reverse_weight': 0.3},
           'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'attention_rescoring_decoder_conf': {'beam_size': nbest, 'first_pass': first_pass}, 'dataset_conf': {'dataset_vocab': vpath},
           'use_model': 'conformer', 'streaming': True, 'decoder': 'attention_rescoring', 'metrics_type': 'cer'}
    pred = MASRPredictor(configs=cfg, use_gpu=True, state_dict=sd)
    n = int(seconds * 16000)
    pcm = synthetic.synthetic_pcm(batch * passes, n, seed=5)
    audio = [pcm[i] for i in range(batch * passes)]
    times = {'1': [], '2': []}
    lengths = []
    for k in range(runs + 2):
        for lanes in ('1', '2'):
            os.environ['MASR_LANES'] = lanes
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pred.predict_batch(audio, batch_size=batch)
            dt = (time.perf_counter() - t0) * 1e3
            if k >= 2:
                times[lanes].append(dt)
            lengths = [len(r['text']) for r in res]
    stat = lambda v: {'median_ms': float(np.median(v)), 'min_ms': float(min(v)), 'max_ms': float(max(v))}
    print(json.dumps({'predict_batch': f'{passes} passes x {batch} utterances x {seconds} s, beam_size {nbest}', 'first_pass': first_pass, 'runs': runs,
                      'one_lane': stat(times['1']), 'two_lanes': stat(times['2']),
                      'winner_tokens_mean': float(np.mean(lengths))}))


if __name__ == '__main__':
    if '--predict-batch' in sys.argv:
        predict_batch_lanes(first_pass=sys.argv[sys.argv.index('--first-pass') + 1] if '--first-pass' in sys.argv else 'host')
    else:
        main()
