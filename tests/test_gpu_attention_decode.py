"""GPU: attention decoding (masr_attention_decode / masr_op_decoder_step, csrc/decoder_step.hip) against the plain-torch restatement
(tests/attention_decode_ref.py) under the float64 budget rule of tests/budget.py (C = 8 unchanged: truth = the restatement in
float64, reference = the restatement in float32): the step's log-probabilities at the cache, lane-split and width edges, the
top-N / merge tie rules, the search against the float64 search wherever its decisions are safe, bit-for-bit invariance of an
utterance's result, and the mode end to end through MASRPredictor.

V = 50, d = 256 / 4 heads, decoder 2 + 2 blocks, linear_units 384 unless a case says otherwise (the shapes and the synthetic
checkpoint of tests/test_gpu_rescoring.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_decode_ref as ar            # noqa: E402
import budget            # noqa: E402
import rescoring_ref as rr            # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
V = 50
SEED = 11
DEC = dict(linear_units=384, num_blocks=2, r_num_blocks=2)
DEC_CONF = dict(attention_heads=4, **DEC)
ENC_CONF = dict(num_blocks=2, linear_units=256)


def _sd(decoder=DEC, vocab=V, **kw):
    from masr_amd.utils import synthetic
    return synthetic.conformer_state_dict(SEED, vocab, d_ff=256, num_blocks=2, decoder=decoder, **kw)


def _engine(sd_, vocab=V, dec=DEC, **kw):
    from masr_amd.engine import HipEngine
    return HipEngine(sd_, encoder_conf=ENC_CONF, vocab_size=vocab, attention_decoder=True, decoder_conf=dict(attention_heads=4, **dec),
                     **kw)


@pytest.fixture(scope='module')
def sd():
    return _sd()


@pytest.fixture(scope='module')
def eng(sd):
    e = _engine(sd)
    yield e
    e.close()


@pytest.fixture
def poll(monkeypatch):
    def set_(n):
        monkeypatch.setenv('MASR_ATTENTION_POLL', str(n))
    return set_


def _ref_rows(sd_, memory, mem_lens, prefixes, lens, heads=4):
    """the restatement's log-probability rows [B, N, V] behind every prefix, float64 and float32"""
    B, N, _ = prefixes.shape
    out = []
    for s in (rr.to64(sd_), sd_):
        rows = np.zeros((B, N, s['decoder.left_decoder.embed.0.weight'].shape[0]), np.float64)
        for b in range(B):
            for n in range(N):
                rows[b, n] = ar.step_logp(s, memory[b, :int(mem_lens[b])], prefixes[b, n, :int(lens[b, n])], heads)
        out.append(rows)
    return out


def _safe_rows(y64, e_ref_max, n):
    """rows whose gaps between consecutive entries of the float64 top n + 1 all exceed 2 C max|e_ref|"""
    top = -np.sort(-budget.as64(y64), axis=-1)[..., :n + 1]
    return (top[..., :-1] - top[..., 1:]).min(axis=-1) > 2 * budget.C * e_ref_max


def _check_step(name, sd_, eng_, memory, mem_lens, prefixes, lens, top_n, heads=4):
    y64, y32 = _ref_rows(sd_, memory, mem_lens, prefixes, lens, heads)
    ids, top, logp = eng_.op_decoder_step(torch.as_tensor(memory).to(eng_.device), mem_lens, prefixes, lens, top_n=top_n)
    f = budget.check(name + ' logp', y64, y32, logp)
    safe = _safe_rows(y64, f['max_ref'], top_n)
    want = np.argsort(-y64, axis=-1, kind='stable')[..., :top_n]
    print(f'{name}: {int(safe.sum())} of {safe.size} rows with safe top-{top_n} gaps', flush=True)
    assert safe.any()
    assert np.array_equal(ids[safe], want[safe])
    # the top-N the kernel reports is the top-N of the rows it reports, in its order
    for b, n in np.ndindex(*ids.shape[:2]):
        assert [(v, i) for v, i in ar.top_n(logp[b, n], top_n)] == list(zip(top[b, n].tolist(), ids[b, n].tolist())), (b, n)
    return ids, top, logp


def test_step_parity_prefix_and_source_length_edges(sd, eng):
    """one ragged batch: source lengths 1, 63, 64, 65, 130 (one lane's share of the keys at, below and past 64 and past 128),
    decoder inputs [sos, tokens...] of 1, 2, 63, 64, 65 and 66 positions (the self-attention's key count round the same edges)"""
    rng = np.random.default_rng(5)
    mem_lens = np.array([1, 63, 64, 65, 130], np.int32)
    memory = rng.standard_normal((5, 130, 256)).astype(np.float32)
    lens = np.tile(np.array([0, 1, 62, 63, 64, 65], np.int32), (5, 1))
    prefixes = rng.integers(0, V - 1, (5, 6, 65)).astype(np.int32)
    _check_step('ragged', sd, eng, memory, mem_lens, prefixes, lens, 4)


def test_step_width_512_heads_8():
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sdw = synthetic.conformer_state_dict(5, V, d=512, heads=8, d_ff=256, num_blocks=1, decoder=DEC)
    e = HipEngine(sdw, encoder_conf=dict(output_size=512, attention_heads=8, num_blocks=1, linear_units=256), vocab_size=V,
                  attention_decoder=True, decoder_conf=dict(attention_heads=8, **DEC))
    try:
        rng = np.random.default_rng(4)
        memory = rng.standard_normal((2, 21, 512)).astype(np.float32)
        prefixes = rng.integers(0, V - 1, (2, 2, 9)).astype(np.int32)
        _check_step('512/8', sdw, e, memory, np.array([21, 13], np.int32), prefixes, np.array([[9, 3], [0, 8]], np.int32), 3, heads=8)
    finally:
        e.close()


def test_step_checkpoint_without_right_decoder():
    dec = dict(DEC, r_num_blocks=0)
    sd0 = _sd(dec)
    e = _engine(sd0, dec=dec)
    try:
        rng = np.random.default_rng(8)
        memory = rng.standard_normal((2, 17, 256)).astype(np.float32)
        prefixes = rng.integers(0, V - 1, (2, 2, 5)).astype(np.int32)
        _check_step('r_num_blocks=0', sd0, e, memory, np.array([17, 9], np.int32), prefixes, np.array([[5, 0], [2, 4]], np.int32), 3)
        _, lens, _, _ = e.attention_decode(torch.from_numpy(memory).to(e.device), torch.tensor([17, 9], dtype=torch.int32).to(e.device), 3)
        assert lens.shape == (2, 3)
    finally:
        e.close()


@pytest.mark.parametrize('family', ['squeezeformer', 'efficient_conformer'])
def test_step_other_families_use_the_same_decoder_keys(family):
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    make = synthetic.squeezeformer_state_dict if family == 'squeezeformer' else synthetic.efficient_conformer_state_dict
    sdf = make(2, V, num_blocks=12)
    sdf.update(synthetic.attention_decoder_state_dict(2, V, 256, **DEC))
    e = HipEngine(sdf, vocab_size=V, use_model=family, streaming=family != 'squeezeformer', attention_decoder=True,
                  decoder_conf=DEC_CONF)
    try:
        rng = np.random.default_rng(6)
        feats = (rng.standard_normal((2, 131, 80)) * 3 + 13).astype(np.float32)
        feats[1, 99:] = 0
        lens = torch.tensor([131, 99], dtype=torch.int32)
        enc = e.encode_full(torch.from_numpy(feats).to(e.device), lens.to(e.device), -1)
        mem_lens = np.asarray(e.enc_frames(lens.numpy())).astype(np.int32)
        prefixes = rng.integers(0, V - 1, (2, 2, 7)).astype(np.int32)
        _check_step(family, sdf, e, enc.cpu().numpy(), mem_lens, prefixes, np.array([[7, 2], [0, 5]], np.int32), 3)
    finally:
        e.close()


def test_fixture_parity_with_the_live_reference_record(eng):
    """forward_one_step of the live reference on fixed prefixes, recorded in float64 and float32 (tools/make_attention_decode_golden.py)"""
    z = np.load(os.path.join(GOLDEN, 'attention_decode_v50.npz'))
    ids, top, logp = eng.op_decoder_step(torch.from_numpy(z['memory']).to(eng.device), z['mem_lens'], z['prefixes'], z['prefix_lens'],
                                         top_n=4)
    f = budget.check('fixture logp', z['logp64'], z['logp32'], logp)
    safe = _safe_rows(z['logp64'], f['max_ref'], 4)
    want = np.argsort(-z['logp64'], axis=-1, kind='stable')[..., :4]
    assert safe.any() and np.array_equal(ids[safe], want[safe])


# ---- top-N and merge edges --------------------------------------------------------------------------------------------------
def _mem(T, seed=0, d=256):
    return np.random.default_rng(seed).standard_normal((T, d)).astype(np.float32)


def _decode(eng_, memories, n, max_len=0, tp=None, lcap=None):
    """attention_decode over a list of utterances [T_b, d] -> (per utterance [(tokens, score)] x N, steps)"""
    B, tp = len(memories), tp or max(len(m) for m in memories)
    enc = np.zeros((B, tp, memories[0].shape[1]), np.float32)
    for b, m in enumerate(memories):
        enc[b, :len(m)] = m
    lens = torch.tensor([len(m) for m in memories], dtype=torch.int32)
    tokens, hl, scores, steps = eng_.attention_decode(torch.from_numpy(enc).to(eng_.device), lens.to(eng_.device), n, max_len, lcap)
    tokens, hl, scores = tokens.cpu().numpy(), hl.cpu().numpy(), scores.cpu().numpy()
    assert ((tokens == V - 1) | (np.arange(tokens.shape[2])[None, None] < hl[..., None])).all()      # eos behind every length
    return [[(tokens[b, k, :hl[b, k]].tolist(), scores[b, k]) for k in range(n)] for b in range(B)], steps


def _assert_search(name, got, r64, r32, n):
    """the device's N hypotheses against the float64 search: equal in order with scores within the budget when every step is safe"""
    e_ref, unsafe = ar.safety(r64, r32)
    print(f'{name}: steps {r64["steps"]} of {r64["limit"]}, min margin {min(r64["margins"]):.3e}, 2 C max|e_ref| '
          f'{2 * budget.C * e_ref:.3e}, first unsafe step {unsafe}', flush=True)
    if unsafe is not None:
        return False
    assert [h for h, _ in got] == [h for h, _ in r64['hyps']], name
    s64 = np.array([s for _, s in r64['hyps']], np.float64)
    s = np.array([s for _, s in got], np.float64)
    fin = np.isfinite(s64)
    assert np.array_equal(np.isfinite(s), fin)
    assert np.abs(s[fin] - s64[fin]).max() <= budget.C * max(e_ref, budget.ULP32 * np.abs(s64[fin]).max()), name
    return True


@pytest.mark.parametrize('n', [1, V])
def test_beam_of_one_and_of_the_whole_vocabulary(sd, eng, n, poll):
    poll(1)
    mem = _mem(6, 1)
    got, steps = _decode(eng, [mem], n)
    r64, r32 = ar.search(rr.to64(sd), mem, n), ar.search(sd, mem, n)
    assert steps == r64['steps']
    safe = _assert_search(f'N={n}', got[0], r64, r32, n)
    assert safe or n == V
    if not safe:
        # 51 of 2500 candidates lie closer than the float32 error: the same decisions up to the first unsafe step (the search cut
        # there by max_len), and a full beam of distinct hypotheses in descending order behind it
        _, k = ar.safety(r64, r32)
        assert k > 1
        cut, _ = _decode(eng, [mem], n, max_len=k - 1)
        assert [h for h, _ in cut[0]] == [h for h, _ in ar.search(rr.to64(sd), mem, n, max_len=k - 1)['hyps']]
        s = np.array([s for _, s in got[0]])
        assert np.isfinite(s).all() and (np.diff(s) <= 0).all() and len({tuple(h) for h, _ in got[0]}) == n


def test_first_step_only_rank_zero_is_finite(sd, eng):
    """max_len = 1: the N x N candidates of step 1 are rank 0's top N and -inf everywhere else; the -inf ties go by flat index, so
    the beam is exactly rank 0's top N in order, with their log-probabilities as scores"""
    mem = _mem(9, 2)
    got, steps = _decode(eng, [mem], 5, max_len=1)
    ids, top, _ = eng.op_decoder_step(torch.from_numpy(mem[None]).to(eng.device), [9], np.zeros((1, 1, 1), np.int32),
                                      np.zeros((1, 1), np.int32), top_n=5)
    assert steps == 1
    assert [h for h, _ in got[0]] == [[t] if t != V - 1 else [] for t in ids[0, 0].tolist()]
    assert np.array_equal(np.array([s for _, s in got[0]], np.float32), top[0, 0])
    # a beam wider than the finite candidates of a 1-step search still holds only rank 0's: N = V
    got, _ = _decode(eng, [mem], V, max_len=1)
    assert sorted(t for h, _ in got[0] for t in (h or [V - 1])) == list(range(V))


def test_vocabulary_4233_top_64():
    """V = 4233 (no multiple of 64 or 256) with N = 64"""
    vocab = 4233
    sdv = _sd(vocab=vocab)
    e = _engine(sdv, vocab=vocab)
    try:
        rng = np.random.default_rng(12)
        memory = rng.standard_normal((1, 11, 256)).astype(np.float32)
        prefixes = rng.integers(0, vocab - 1, (1, 2, 3)).astype(np.int32)
        lens = np.array([[0, 3]], np.int32)
        y64, y32 = _ref_rows(sdv, memory, [11], prefixes, lens)
        ids, top, logp = e.op_decoder_step(torch.from_numpy(memory).to(e.device), [11], prefixes, lens, top_n=64)
        budget.check('V=4233 logp', y64, y32, logp)
        for n in range(2):
            assert [(v, i) for v, i in ar.top_n(logp[0, n], 64)] == list(zip(top[0, n].tolist(), ids[0, n].tolist()))
        tokens, hl, scores, steps = e.attention_decode(torch.from_numpy(memory).to(e.device),
                                                       torch.tensor([11], dtype=torch.int32).to(e.device), 64, 2)
        assert steps == 2 and tokens.shape == (1, 64, 2)
        s = scores.cpu().numpy()[0]
        assert np.isfinite(s).all() and (np.diff(s) <= 0).all()
    finally:
        e.close()


def test_two_bit_equal_output_rows_the_smaller_id_first(sd):
    """rows 3 and 41 of the output layer made the same (weights and bias) and the likeliest: their log-probabilities are bit-equal
    and id 3 comes first, in the step's top-N and in the beam"""
    sd2 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
    w, b = sd2['decoder.left_decoder.output_layer.weight'], sd2['decoder.left_decoder.output_layer.bias']
    w[41] = w[3]
    b[3] += 30.0
    b[41] = b[3]
    e = _engine(sd2)
    try:
        mem = _mem(7, 3)
        ids, top, logp = e.op_decoder_step(torch.from_numpy(mem[None]).to(e.device), [7], np.zeros((1, 1, 1), np.int32),
                                           np.zeros((1, 1), np.int32), top_n=3)
        assert logp[0, 0, 3] == logp[0, 0, 41] and ids[0, 0, :2].tolist() == [3, 41] and top[0, 0, 0] == top[0, 0, 1]
        got, _ = _decode(e, [mem], 2, max_len=1)
        assert [h for h, _ in got[0]] == [[3], [41]] and got[0][0][1] == got[0][1][1]
    finally:
        e.close()


@pytest.mark.parametrize('bias', [14.0, 16.0])
def test_raised_eos_bias_finished_rows_and_early_stop(sd, bias, poll):
    """eos made likely: hypotheses finish from step 1 on while others run on (finished rows offer (0, eos) alone), and the search
    stops below its limit when all N are finished; with the poll at every step `steps` is the float64 search's"""
    sd2 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
    sd2['decoder.left_decoder.output_layer.bias'][V - 1] += bias
    e = _engine(sd2)
    try:
        mem = _mem(20, 0)
        r64, r32 = ar.search(rr.to64(sd2), mem, 4), ar.search(sd2, mem, 4)
        assert r64['steps'] < r64['limit'] and len({len(h) for h, _ in r64['hyps']}) > 1
        poll(1)
        got, steps = _decode(e, [mem], 4)
        assert _assert_search(f'eos bias {bias}', got[0], r64, r32, 4)
        assert steps == r64['steps']
        poll(0)                      # never polled: the steps up to the limit add +0 and eos
        again, steps = _decode(e, [mem], 4)
        assert steps == r64['limit']
        assert _same(again, got)
    finally:
        e.close()


def _same(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(hx == hy and np.float32(sx).tobytes() == np.float32(sy).tobytes()
                                                             for (hx, sx), (hy, sy) in zip(x, y)) for x, y in zip(a, b))


# ---- the search ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def e2e(sd, eng):
    """the 8 utterances of attention_decode_ref.E2E through the engine's own front end and encoder, and the restatement's searches
    over that encoder output (float64 truth, float32 reference), once"""
    from masr_amd.utils import synthetic
    E = ar.E2E
    pcm = synthetic.synthetic_pcm(8, max(E['lens']), seed=E['pcm_seed'])
    for i, n in enumerate(E['lens']):
        pcm[i, n:] = 0
    ns = torch.tensor(E['lens'], dtype=torch.int32, device=eng.device)
    feats, frames = eng.fbank_batch(torch.from_numpy(pcm).to(eng.device), ns)
    enc = eng.encode_full(feats, frames, -1)
    mem_lens = np.asarray(eng.enc_frames(frames.cpu().numpy())).astype(np.int32)
    assert 18 <= mem_lens.min() and mem_lens.max() <= 32 and len(set(mem_lens.tolist())) == 8
    mems = [enc[b, :mem_lens[b]].cpu().numpy() for b in range(8)]
    sd64 = rr.to64(sd)
    r64 = [ar.search(sd64, m, E['beam_size']) for m in mems]
    r32 = [ar.search(sd, m, E['beam_size']) for m in mems]
    return dict(pcm=pcm, mems=mems, r64=r64, r32=r32, n=E['beam_size'])


def test_search_parity_with_the_float64_search(sd, eng, e2e):
    got, _ = _decode(eng, e2e['mems'], e2e['n'])
    safe = 0
    for b in range(8):
        if _assert_search(f'E2E utterance {b}', got[b], e2e['r64'][b], e2e['r32'][b], e2e['n']):
            safe += 1
            continue
        # unsafe: the same decisions up to the first unsafe step (the search cut there by max_len)
        _, k = ar.safety(e2e['r64'][b], e2e['r32'][b])
        if k > 1:
            cut, _ = _decode(eng, [e2e['mems'][b]], e2e['n'], max_len=k - 1)
            c64 = ar.search(rr.to64(sd), e2e['mems'][b], e2e['n'], max_len=k - 1)
            assert [h for h, _ in cut[0]] == [h for h, _ in c64['hyps']], b
    assert safe >= 6, safe


def test_an_utterance_alone_in_a_batch_padded_on_the_other_lane_and_polled(eng, e2e, poll):
    """bit for bit: an utterance's N hypotheses and scores do not depend on B, its neighbours, the padding of Tp, the lane, or on
    how often the host polls for the end"""
    n = e2e['n']
    full, _ = _decode(eng, e2e['mems'], n)
    for b in (0, 3, 7):
        alone, _ = _decode(eng, [e2e['mems'][b]], n)
        assert _same(alone, [full[b]]), b
    wide, _ = _decode(eng, e2e['mems'][2:5], n, tp=77)
    assert _same(wide, full[2:5])
    back, _ = _decode(eng, e2e['mems'][::-1], n)
    assert _same(back[::-1], full)
    eng.select_lane(1)
    try:
        with torch.cuda.stream(eng.side_stream(4)):
            lane1, _ = _decode(eng, e2e['mems'], n)
    finally:
        eng.select_lane(0)
    assert _same(lane1, full)
    for every in (1, 0, 3):
        poll(every)
        polled, steps = _decode(eng, e2e['mems'], n)
        assert _same(polled, full), every
        assert every != 0 or steps == 32


def test_an_utterance_inside_a_batch_whose_rows_change_the_gemm_tile(eng):
    """bit for bit across the tiled GEMM's tile choice: alone an utterance's 50 rows run on 64 x 64 tiles; among 130 utterances
    (6500 rows) the q, k | v and feed-forward projections cross the row-count threshold and run on 64 x 128 tiles"""
    rng = np.random.default_rng(31)
    mems = [rng.standard_normal((4, 256)).astype(np.float32) for _ in range(130)]
    full, steps = _decode(eng, mems, V, max_len=3)
    assert steps == 3
    for b in (0, 77, 129):
        alone, _ = _decode(eng, [mems[b]], V, max_len=3)
        assert _same(alone, [full[b]]), b


def test_max_len_cuts_the_same_search(sd, eng, e2e):
    """max_len = k: the search of the first k steps whatever else bounds it (lcap, a batch whose other utterances are shorter)"""
    n, mem = e2e['n'], e2e['mems'][0]
    a, steps = _decode(eng, [mem], n, max_len=5)
    assert steps == 5
    b, _ = _decode(eng, [mem], n, max_len=5, lcap=32)
    c, _ = _decode(eng, [mem], n, max_len=0, lcap=5)
    d, _ = _decode(eng, [mem, e2e['mems'][7][:3]], n, max_len=5)
    assert _same(a, b) and _same(a, c) and _same(a, d[:1])
    assert all(len(h) <= 3 for h, _ in d[1])
    r64, r32 = ar.search(rr.to64(sd), mem, n, max_len=5), ar.search(sd, mem, n, max_len=5)
    _assert_search('max_len=5', a[0], r64, r32, n)


# ---- through the facade ---------------------------------------------------------------------------------------------------------
def _cfg(tmp_path, decoder, **more):
    from masr_amd.utils import synthetic
    vpath = os.path.join(tmp_path, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(V):
            f.write(f'{t}\t1\n')
    cfg = {'encoder_conf': dict(ENC_CONF), 'decoder_conf': dict(DEC_CONF),
           'model_conf': {'ctc_weight': 0.3, 'reverse_weight': 0.3},
           'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'attention_decoder_conf': {'beam_size': ar.E2E['beam_size']},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'conformer', 'streaming': True, 'decoder': decoder,
           'metrics_type': 'cer'}
    cfg.update(more)
    return cfg


def test_predictor_returns_the_float64_texts_of_the_safe_utterances(tmp_path, sd):
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    pred = MASRPredictor(configs=_cfg(str(tmp_path), 'attention'), use_gpu=True, state_dict=sd)
    dec = pred.attention_decoder
    seen = []
    inner = dec.search_launch

    def spy(eng_, enc, enc_lens):
        seen.append((enc.cpu().numpy(), enc_lens.cpu().numpy()))
        return inner(eng_, enc, enc_lens)
    dec.search_launch = spy
    E = ar.E2E
    pcm = synthetic.synthetic_pcm(8, max(E['lens']), seed=E['pcm_seed'])
    audio = [pcm[i, :n].copy() for i, n in enumerate(E['lens'])]
    sd64 = rr.to64(sd)

    def check(mem, result, name):
        """the result of one utterance against the float64 search over the encoder output the facade searched; False = unsafe"""
        r64, r32 = ar.search(sd64, mem, E['beam_size']), ar.search(sd, mem, E['beam_size'])
        e_ref, unsafe = ar.safety(r64, r32)
        if unsafe is not None:
            return False
        toks, score = r64['hyps'][0]
        assert result['text'] == pred._text(toks), name
        assert abs(result['score'] - score) <= budget.C * max(e_ref, budget.ULP32 * abs(score)), name
        return True
    res = pred.predict_batch(audio)
    assert len(seen) == 1 and len(res) == 8
    memory, mem_lens = seen[0]
    kept = sum(check(memory[b, :mem_lens[b]], res[b], f'predict_batch {b}') for b in range(8))
    assert kept >= 6, kept
    # predict: one utterance through its own pass (its own encoder output)
    kept = 0
    for b in range(8):
        one = pred.predict(audio_data=audio[b])
        memory, mem_lens = seen[-1]
        assert memory.shape[0] == 1
        kept += check(memory[0, :mem_lens[0]], one, f'predict {b}')
        if kept >= 2:
            break
    assert kept >= 2
    with pytest.raises(Exception, match="decoder='attention' does not run on streaming sessions"):
        pred.predict_stream(pcm[0, :16000].tobytes())
    with pytest.raises(Exception, match="decoder='attention' needs the encoder output"):
        pred.decode(np.zeros((4, V), np.float32), False, False)


def test_greedy_engine_is_what_it_was(sd, eng):
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    g = HipEngine(sd, encoder_conf=ENC_CONF, vocab_size=V)
    try:
        assert g.decoder_info() == {'enabled': False, 'num_blocks': 0, 'r_num_blocks': 0, 'weight_bytes': 0, 'workspace_bytes': 0}
        pcm = torch.from_numpy(synthetic.synthetic_pcm(2, 24000, seed=3)).to(g.device)
        ns = torch.tensor([24000, 17000], dtype=torch.int32, device=g.device)
        rows = [x.transcribe_rows(pcm, ns, True, -20.0).cpu().numpy() for x in (g, eng)]
        assert np.array_equal(rows[0], rows[1])
        assert g.decoder_info()['workspace_bytes'] == 0
        eng.op_decoder_step(torch.zeros(1, 4, 256, device=eng.device), [4], np.zeros((1, 1, 1), np.int32), np.zeros((1, 1), np.int32))
        assert eng.decoder_info()['enabled'] and eng.decoder_info()['workspace_bytes'] > 0
    finally:
        g.close()


def test_refusals_on_a_live_engine(sd, eng):
    from masr_amd._lib import MasrError
    from masr_amd.engine import HipEngine
    enc = torch.zeros(1, 4, 256, device=eng.device)
    lens = torch.tensor([4], dtype=torch.int32, device=eng.device)
    g = HipEngine(sd, encoder_conf=ENC_CONF, vocab_size=V)
    try:
        with pytest.raises(MasrError, match='no attention decoder'):
            g.attention_decode(enc, lens, 4)
        with pytest.raises(MasrError, match='no attention decoder'):
            g.op_decoder_step(enc, [4], np.zeros((1, 1, 1), np.int32), np.zeros((1, 1), np.int32))
    finally:
        g.close()
    with pytest.raises(MasrError, match='exceeds the vocabulary'):
        eng.attention_decode(enc, lens, V + 1)
    with pytest.raises(MasrError, match='outside 1 .. 64'):
        eng.attention_decode(enc, lens, 65)
    with pytest.raises(MasrError, match='outside 1 .. 64'):
        eng.attention_decode(enc, lens, 0)
    big = torch.zeros(1311, 1, 256, device=eng.device)
    with pytest.raises(MasrError, match='65535'):
        eng.attention_decode(big, torch.ones(1311, dtype=torch.int32, device=eng.device), 50)
    with pytest.raises(MasrError, match='outside 0 .. L'):
        eng.op_decoder_step(enc, [4], np.zeros((1, 1, 2), np.int32), np.array([[3]], np.int32))
    with pytest.raises(MasrError, match='outside the vocabulary'):
        eng.op_decoder_step(enc, [4], np.full((1, 1, 2), V, np.int32), np.array([[2]], np.int32))
    with pytest.raises(MasrError, match='outside 1 .. Tp'):
        eng.op_decoder_step(enc, [5], np.zeros((1, 1, 2), np.int32), np.array([[2]], np.int32))
