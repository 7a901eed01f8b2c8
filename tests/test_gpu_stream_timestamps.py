"""GPU: token timestamps on streaming sessions -- masr_ctc_align_rows (csrc/ctc_align.hip: the forced alignment reading its frames
through a row table), the posterior history of a ``StreamPool(predictor, timestamps=True)`` and the ``'tokens'`` of its results.

Everything is exact.  The kernel alone must give the bits of masr_ctc_align on the gathered dense copy and of the float32 numpy
restatement (tests/ctc_align_ref.py); the pool's history must be, to the bit, what the CTC head wrote for the same windows in the same
lock-step calls on a second engine; and the ``'tokens'`` of every result must equal ``utterance_tokens`` of the CPU alignment of that
history.  Host side: tests/test_stream_timestamps_cpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_align_ref as ar            # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
V = 50
MAX_TOKENS = 1024


def _log_softmax32(x):
    x = np.asarray(x, np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, name):
    for g, w, what in zip(got, want, ('start', 'end', 'peak', 'score', 'status')):
        assert g.dtype == w.dtype and np.array_equal(_bits(g), _bits(w)), f'{name}: {what}\n{g}\n{w}'


@pytest.fixture(scope='module')
def bare():
    """a weight-less engine: the alignment needs no model"""
    from masr_amd.engine import HipEngine
    e = HipEngine(None, vocab_size=V)
    yield e
    e.close()


def _dev(eng, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(eng.device)


def _rows_call(eng, rows_dev, table, n_frames, tokens, n_tokens, is_log=True):
    out = eng.ctc_align_rows(rows_dev, _dev(eng, table, np.int64), _dev(eng, n_frames, np.int32), _dev(eng, tokens, np.int32),
                             _dev(eng, n_tokens, np.int32), input_is_log=is_log)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _dense_call(eng, post, n_frames, tokens, n_tokens, is_log=True):
    out = eng.ctc_align(_dev(eng, post, np.float32), _dev(eng, n_frames, np.int32), _dev(eng, tokens, np.int32),
                        _dev(eng, n_tokens, np.int32), input_is_log=is_log)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


# ---- the kernel alone -------------------------------------------------------------------------------------------------------------
N_ROWS, KV = 300, 37
T_OF = [1, 16, 17, 40]


@pytest.fixture(scope='module')
def awkward():
    """B = 4 utterances over one [300, 37] matrix of random log-probability rows, with row tables as a row pool makes them:
      0: T = 1, L = 0 -- one row in the middle of the others';
      1: T = 16, L = 1 -- strictly decreasing rows;
      2: T = 17, adjacent equal tokens -- a 16-row block on the even rows of a region it shares with utterance 3, and frame 16 in
         the SAME row as frame 15 (a row may repeat);
      3: T = 40 = L (every frame a token) -- 16-row blocks from three places: the odd rows of the shared region, a block high up,
         then a block below both (block boundaries at frames 16 and 32).
    Entries behind n_frames hold garbage: negative, n_rows and far beyond 2^31."""
    rng = np.random.default_rng(11)
    rows = _log_softmax32(rng.standard_normal((N_ROWS, KV)) * 3)
    table = np.empty((4, 40), np.int64)
    table[:] = np.array([-7, N_ROWS, 1 << 40, -(1 << 35)])[rng.integers(0, 4, (4, 40))]
    table[0, :1] = [101]
    table[1, :16] = np.arange(60, 28, -2)
    table[2, :16] = 100 + 2 * np.arange(16)
    table[2, 16] = table[2, 15]
    table[3, :16] = 99 + 2 * np.arange(16)
    table[3, 16:32] = np.arange(280, 296)
    table[3, 32:40] = np.arange(3, 11)
    lmax = 40
    tokens = np.full((4, lmax), -1, np.int32)
    n_tokens = np.array([0, 1, 5, 40], np.int32)
    tokens[1, :1] = [KV - 1]
    tokens[2, :5] = [5, 5, 9, 3, 3]
    h = rng.integers(1, KV, 40)
    for i in range(1, 40):
        while h[i] == h[i - 1]:
            h[i] = rng.integers(1, KV)
    tokens[3] = h
    n_frames = np.array(T_OF, np.int32)
    dense = np.full((4, 40, KV), np.nan, np.float32)
    for b in range(4):
        dense[b, :T_OF[b]] = rows[table[b, :T_OF[b]]]
    return rows, table, n_frames, tokens, n_tokens, dense


def test_rows_kernel_equals_the_dense_kernel_and_the_restatement_to_the_bit(bare, awkward):
    rows, table, n_frames, tokens, n_tokens, dense = awkward
    rows_dev = _dev(bare, rows, np.float32)
    got = _rows_call(bare, rows_dev, table, n_frames, tokens, n_tokens)
    assert got[4].tolist() == [0, 0, 0, 0]
    assert got[0][3].tolist() == list(range(40)) and got[1][3].tolist() == list(range(40))          # L = T: the diagonal
    _same(got, _dense_call(bare, dense, n_frames, tokens, n_tokens), 'rows against masr_ctc_align on the gathered copy')
    _same(got, ar.align_batch(dense, n_frames, tokens, n_tokens, np.float32), 'rows against the float32 restatement')
    # probabilities: the kernel takes the logarithm itself, of the same values wherever they lie (one row holds zeros and a NaN)
    p = np.exp(rows.astype(np.float64)).astype(np.float32)
    p[104, :] = 0
    p[106, 5] = np.nan
    pd = np.full((4, 40, KV), np.nan, np.float32)
    for b in range(4):
        pd[b, :T_OF[b]] = p[table[b, :T_OF[b]]]
    got_p = _rows_call(bare, _dev(bare, p, np.float32), table, n_frames, tokens, n_tokens, is_log=False)
    _same(got_p, _dense_call(bare, pd, n_frames, tokens, n_tokens, is_log=False), 'probabilities')
    assert got_p[4].tolist() == [0, 0, 0, 0] and got_p[3][2] < ar.NEG / 2          # utterance 2 crosses the row of zeros
    # the other lane has its own predecessor workspace: the same bits
    bare.select_lane(1)
    try:
        _same(_rows_call(bare, rows_dev, table, n_frames, tokens, n_tokens), got, 'lane 1')
    finally:
        bare.select_lane(0)


@pytest.mark.parametrize('bad', [N_ROWS, -1, 1 << 33])
def test_a_row_number_out_of_range_is_status_2_for_its_utterance_alone(bare, awkward, bad):
    rows, table, n_frames, tokens, n_tokens, dense = awkward
    rows_dev = _dev(bare, rows, np.float32)
    good = _rows_call(bare, rows_dev, table, n_frames, tokens, n_tokens)
    t = table.copy()
    t[2, 11] = bad                                             # inside the 17 valid frames of utterance 2
    got = _rows_call(bare, rows_dev, t, n_frames, tokens, n_tokens)
    assert got[4].tolist() == [0, 0, 2, 0]
    assert (got[0][2] == -1).all() and (got[1][2] == -1).all() and (got[2][2] == 0).all() and got[3][2] == 0
    for b in (0, 1, 3):
        _same(tuple(g[b:b + 1] for g in got), tuple(g[b:b + 1] for g in good), f'utterance {b} beside the refused one')
    t = table.copy()
    t[2, 17] = bad                                             # the first entry BEHIND its valid frames: never read
    _same(_rows_call(bare, rows_dev, t, n_frames, tokens, n_tokens), good, 'behind n_frames')


def test_refusals_by_name(bare):
    from masr_amd._lib import MasrError
    one = np.zeros(1, np.int32)
    with pytest.raises(MasrError, match='masr_ctc_align_rows.*MASR_ALIGN_MAX_TOKENS'):
        _rows_call(bare, _dev(bare, np.zeros((4, 8)), np.float32), np.zeros((1, MAX_TOKENS + 8), np.int64), one,
                   np.ones((1, MAX_TOKENS + 1), np.int32), one)
    with pytest.raises(MasrError, match='masr_ctc_align_rows: V > 16384'):
        _rows_call(bare, _dev(bare, np.zeros((2, 16385)), np.float32), np.zeros((1, 2), np.int64), one, np.ones((1, 1), np.int32), one)
    with pytest.raises(MasrError, match="Lmax 3 > T' 2"):
        _rows_call(bare, _dev(bare, np.zeros((4, 8)), np.float32), np.zeros((1, 2), np.int64), one, np.ones((1, 3), np.int32), one)
    with pytest.raises(ValueError, match='int64'):
        bare.ctc_align_rows(_dev(bare, np.zeros((4, 8)), np.float32), _dev(bare, np.zeros((1, 2)), np.int32), _dev(bare, one, np.int32),
                            _dev(bare, np.ones((1, 1)), np.int32), _dev(bare, one, np.int32))


def test_rows_beyond_two_gigabytes_are_addressed_in_64_bits(bare):
    """V = 16384, 32 800 rows: 2.15 GB, so the byte offset of the last rows exceeds 2^31 (and 2^31 / 4 elements is crossed at row
    32 768).  The matrix is allocated uninitialised; only the 20 rows used are written."""
    big_v, n_rows, T = 16384, 32800, 20
    rng = np.random.default_rng(12)
    used = _log_softmax32(rng.standard_normal((T, big_v)) * 3)
    hyp = np.array([[1, big_v - 1, big_v - 1, 7, 1, 9000]], np.int32)
    small = _rows_call(bare, _dev(bare, used, np.float32), np.arange(T)[None], [T], hyp, [6])
    assert small[4][0] == 0
    try:
        big = torch.empty(n_rows, big_v, dtype=torch.float32, device=bare.device)
    except RuntimeError as exc:            # (torch.cuda.OutOfMemoryError is one)
        pytest.skip(f'no room for the {n_rows * big_v * 4 / 2 ** 30:.2f} GiB row matrix: {exc}')
    try:
        where = np.arange(n_rows - 1, n_rows - 1 - T, -1)          # the last rows, backwards
        assert (where.min() * big_v * 4) > 2 ** 31
        big[_dev(bare, where, np.int64)] = _dev(bare, used, np.float32)
        _same(_rows_call(bare, big, where[None], [T], hyp, [6]), small, 'the same rows at the end of 2.15 GB')
    finally:
        del big
        torch.cuda.empty_cache()


# ---- the pool ---------------------------------------------------------------------------------------------------------------------
EFF_CONF = {'output_size': 256, 'attention_heads': 4, 'linear_units': 256, 'num_blocks': 5, 'cnn_module_kernel': 15,
            'efficient_conf': {'stride_layer_idx': [3], 'stride': [2], 'group_layer_idx': [0, 1, 2, 3], 'group_size': 3,
                               'stride_kernel': True}}


def _predictor(tmp, family, decoder):
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    os.makedirs(tmp, exist_ok=True)
    vpath = os.path.join(tmp, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(V):
            f.write(f'{t}\t1\n')
    if family == 'conformer':
        enc, sd = {'num_blocks': 2, 'linear_units': 256}, synthetic.conformer_state_dict(0, V, d_ff=256, num_blocks=2)
    else:
        enc, sd = dict(EFF_CONF), synthetic.efficient_conformer_state_dict(0, V, d_ff=256, num_blocks=5)
    cfg = {'encoder_conf': enc,
           'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000, 'use_dB_normalization': True,
                               'target_dB': -20},
           'ctc_beam_search_decoder_conf': {'alpha': 0, 'beta': 0, 'beam_size': 8, 'cutoff_prob': 0.99, 'cutoff_top_n': 20,
                                            'num_processes': 2, 'language_model_path': None},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': family, 'streaming': True, 'decoder': decoder, 'metrics_type': 'cer'}
    return MASRPredictor(configs=cfg, use_gpu=True, state_dict=sd)


def _pcm():
    return np.load(os.path.join(GOLDEN, 'testwav.npz'))['pcm']


def _schedule():
    """three sessions: 0 fed in one piece (1.6 s, not ended: full windows only), 1 in 0.2 s pieces (2.2 s, ended: its last window is
    short), 2 in 0.64 s pieces of which the last is short and ends the stream (2.78 s) -> per step [(session, samples, is_end)].
    Step 0 encodes session 0 alone (two windows), step 3 sessions 1 and 2 in one lock-step call, the last steps short windows."""
    pcm = _pcm()
    feeds = {0: [(pcm[:25600], False)],
             1: [(pcm[20000 + s:20000 + min(s + 3200, 35200)], s + 3200 >= 35200) for s in range(0, 35200, 3200)],
             2: [(pcm[50000 + s:50000 + min(s + 10240, 44480)], s + 10240 >= 44480) for s in range(0, 44480, 10240)]}
    steps = []
    for k in range(max(len(f) for f in feeds.values())):
        steps.append([(i, *feeds[i][k]) for i in sorted(feeds) if k < len(feeds[i])])
    return steps


def _kernel_log(eng, p):
    """float32 logf of the probabilities ``p`` [F, V] exactly as the aligner takes it (a value that is not > 0 is the sentinel), read
    off the DENSE kernel, masr_ctc_align with input_is_log = 0: F * V one-frame utterances, the one of (f, v) holding row f and
    the hypothesis [v] -- its score is the logarithm of p[f, v] and nothing else (v = 0: the empty hypothesis, whose one path is the
    blank).  numpy's and torch's float32 log differ from the device's logf in the last bit here and there."""
    F, V_ = p.shape
    post = p.repeat_interleave(V_, 0).view(F * V_, 1, V_).contiguous()
    tok = torch.arange(V_, dtype=torch.int32, device=p.device).repeat(F).view(F * V_, 1).contiguous()
    ones = torch.ones(F * V_, dtype=torch.int32, device=p.device)
    _, _, _, score, status = eng.ctc_align(post, ones, tok, (tok.view(-1) > 0).to(torch.int32), input_is_log=False)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    return score.view(F, V_).cpu().numpy()


def _expected_tokens(pool, h, fed_samples):
    """``utterance_tokens`` of the CPU alignment (tests/ctc_align_ref.py, float32) of the session's own history and hypothesis"""
    from masr_amd.decoders import ctc_alignment as ca
    p = pool.posteriors(h)
    lp = _kernel_log(pool.engine, p)
    with np.errstate(divide='ignore', invalid='ignore'):
        true = np.maximum(np.log(p.cpu().numpy().astype(np.float64)), ca.SENTINEL)
    assert (np.abs(lp - true) <= 1e-6 * np.maximum(1.0, np.abs(true))).all()          # (it IS the logarithm: 8 float32 ulps)
    ids = list(pool.last_tokens(h))
    if len(ids) > min(lp.shape[0], ca.MAX_TOKENS):
        return None
    r = ar.align(lp, ids, np.float32)
    return ca.utterance_tokens(ids, r['start'], r['end'], r['peak'], r['score'], r['status'], pool.engine.frame_reduction(), 16000,
                               fed_samples / 16000.0, pool.vocab)


def _drive(pool, steps, check=None):
    """run the schedule -> (handles, per step {session: result}); ``check(session, handle, result, samples fed)`` after every step"""
    handles = {}
    fed = {}
    out = []
    for step in steps:
        for i, x, end in step:
            if i not in handles:
                handles[i] = pool.open()
            pool.feed(handles[i], x.tobytes(), end)
            fed[i] = fed.get(i, 0) + len(x)
        res = pool.step()
        got = {}
        for i, _, _ in step:
            got[i] = res[handles[i]]
            if check is not None and got[i] is not None:
                check(i, handles[i], got[i], fed[i])
        out.append(got)
    return handles, out


@pytest.mark.parametrize('family,decoder', [('conformer', 'ctc_greedy'), ('conformer', 'ctc_beam_search'),
                                            ('efficient_conformer', 'ctc_greedy'), ('efficient_conformer', 'ctc_beam_search')])
def test_tokens_of_every_step_equal_the_cpu_alignment_of_the_kept_posteriors(tmp_path, family, decoder):
    from masr_amd.serving import StreamPool
    pred = _predictor(str(tmp_path), family, decoder)
    pool = StreamPool(pred, timestamps=True)
    assert pool.framing == 'python' and pool.engine.frame_reduction() == (4 if family == 'conformer' else 8)
    seen = {'results': 0, 'tokens': 0}

    def check(i, h, res, samples):
        assert set(res) == {'text', 'score', 'tokens'}
        rows = pool.posterior_rows(h)
        assert rows.dtype == np.int64 and len(set(rows.tolist())) == len(rows) == pool.posteriors(h).shape[0]
        want = _expected_tokens(pool, h, samples)
        assert res['tokens'] == want, (family, decoder, i, res, want)          # starts, ends and scores equal as floats
        if res['tokens']:
            assert ''.join(t['token'] for t in res['tokens']) == res['text']
            assert all(0 <= t['start'] < t['end'] <= samples / 16000.0 for t in res['tokens'])
            seen['tokens'] += len(res['tokens'])
        else:
            assert res['tokens'] == [] and res['text'] == '' or res['tokens'] is None
        seen['results'] += 1

    handles, out = _drive(pool, _schedule(), check)
    assert seen['results'] >= 8 and seen['tokens'] > 0
    tq = 16 if family == 'conformer' else 8
    # session 0: 1.6 s in one piece = 158 feature frames = two full windows; the sessions' rows are disjoint
    assert len(pool.posterior_rows(handles[0])) == 2 * tq
    allrows = np.concatenate([pool.posterior_rows(h) for h in handles.values()])
    assert len(set(allrows.tolist())) == len(allrows)
    # a session that was not fed returns nothing; a beam-search session fed too little to advance returns None as before
    assert handles[0] not in pool.step()
    for h in handles.values():
        pool.close(h)
    assert pool._alloc.in_use == 0
    pool.shutdown()


def test_history_is_what_the_head_wrote(tmp_path):
    """the pool's posteriors against a second engine on the same checkpoint, driven with the same windows in the same lock-step calls"""
    from masr_amd.serving import StreamPool
    pred = _predictor(os.path.join(str(tmp_path), 'a'), 'conformer', 'ctc_greedy')
    other = _predictor(os.path.join(str(tmp_path), 'b'), 'conformer', 'ctc_greedy').predictor.engine
    pool = StreamPool(pred, timestamps=True)
    eng = pool.engine
    calls = []
    real = eng.encode_chunk

    def recording(stream_ids, feats, **kw):
        calls.append((list(stream_ids), feats.clone()))
        return real(stream_ids, feats, **kw)
    eng.encode_chunk = recording
    try:
        handles, _ = _drive(pool, _schedule())
    finally:
        del eng.encode_chunk
    assert len({len(c[0]) for c in calls}) > 1 and {c[1].shape[1] for c in calls} > {67}          # several groupings, a short window
    twin = {h: other.stream_open(0) for h in handles.values()}
    parts = {h: [] for h in handles.values()}
    for sids, feats in calls:
        probs, _, _ = other.encode_chunk([twin[s] for s in sids], feats, want_probs=True)
        for j, s in enumerate(sids):
            parts[s].append(probs[j])
    lengths = set()
    for h in handles.values():
        want, got = torch.cat(parts[h]), pool.posteriors(h)
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), h
        lengths.add(got.shape[0])
    assert len(lengths) == 3                                    # three sessions of different lengths
    pool.shutdown()


def test_reset_frees_the_rows_and_the_clock_restarts(tmp_path):
    from masr_amd.serving import StreamPool
    pred = _predictor(str(tmp_path), 'conformer', 'ctc_greedy')
    pool = StreamPool(pred, timestamps=True)
    pcm = _pcm()
    two = 400 + 130 * 160                                       # 131 feature frames: exactly two full windows
    a, b = pool.open(), pool.open()

    def run(h, x):
        pool.feed(h, x.tobytes(), False)
        res = pool.step()[h]
        assert res['tokens'] == _expected_tokens(pool, h, len(x))
        return res
    first = run(a, pcm[:two])
    rows_a = pool.posterior_rows(a)
    assert len(rows_a) == 32 and len(pool.posterior_rows(b)) == 0
    pool.reset(a)
    assert len(pool.posterior_rows(a)) == 0
    rb = run(b, pcm[40000:40000 + two])
    assert set(pool.posterior_rows(b).tolist()) == set(rows_a.tolist())          # B sits in the rows A gave back ...
    assert pool.posterior_rows(b).tolist() != sorted(pool.posterior_rows(b).tolist())          # ... which are not in increasing order
    again = run(a, pcm[:two])
    assert not set(pool.posterior_rows(a).tolist()) & set(rows_a.tolist())
    assert again == first and first['tokens']                   # the same audio after the reset: the same tokens at the same times
    assert all(t['end'] <= two / 16000.0 for t in again['tokens'])
    assert rb['tokens'] == _expected_tokens(pool, b, two)       # B is untouched by A's second run
    pool.shutdown()


@pytest.mark.parametrize('decoder', ['ctc_greedy', 'ctc_beam_search'])
def test_without_the_flag_nothing_changes(tmp_path, decoder):
    from masr_amd._lib import MasrError
    from masr_amd.serving import StreamPool
    pred = _predictor(str(tmp_path), 'conformer', decoder)
    plain, timed = StreamPool(pred), StreamPool(pred, timestamps=True)
    assert not plain.timestamps and (plain.framing == 'c') == (decoder == 'ctc_greedy') and timed.framing == 'python'
    _, want = _drive(timed, _schedule())
    _, got = _drive(plain, _schedule())
    n = 0
    for w, g in zip(want, got):
        assert set(w) == set(g)
        for i in w:
            if w[i] is None:
                assert g[i] is None
                continue
            assert set(g[i]) == {'text', 'score'} and g[i]['text'] == w[i]['text'] and g[i]['score'] == w[i]['score'], (i, g[i], w[i])
            n += 1
    assert n >= 8
    with pytest.raises(MasrError, match='timestamps=True'):
        plain.posterior_rows(0)
    plain.shutdown()
    timed.shutdown()
    # the facade: the default is today's dict; the flag adds 'tokens'; inside an utterance it cannot change
    pcm = _pcm()
    r0 = pred.predict_stream(audio_data=pcm[:25600].tobytes())
    assert set(r0) == {'text', 'score'} and not pred._pool.timestamps
    with pytest.raises(MasrError, match='reset_stream'):
        pred.predict_stream(audio_data=pcm[25600:30000].tobytes(), timestamps=True)
    pred.reset_stream()
    r1 = pred.predict_stream(audio_data=pcm[:25600].tobytes(), timestamps=True)
    assert set(r1) == {'text', 'score', 'tokens'} and (r1['text'], r1['score']) == (r0['text'], r0['score']) and pred._pool.timestamps
    pred.reset_stream()
