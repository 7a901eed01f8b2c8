"""GPU, end to end: ``decoder: attention_rescoring`` on streaming sessions with ``attention_rescoring_decoder_conf.on_streams:
'rescore_at_end'`` (serving.LockStepPool).  The partial results are those of a ``ctc_beam_search`` predictor without a language
model and with the same beam and cutoffs; the result of the step that ends an utterance is reproduced offline from what the pool
kept (its encoder rows, the n-best it rescored) and held to the float64 budget of tests/budget.py.

The synthetic model of tests/test_gpu_rescoring.py: V = 50, d = 256, decoder 2 + 2 blocks."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import budget            # noqa: E402
import rescoring_ref as rr            # noqa: E402
from test_gpu_rescoring import _cfg, _sd            # noqa: E402
from masr_amd.serving import token_text            # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 10240                    # 0.64 s
LENS = [32000, 24000, 41000]     # two sessions fed in chunks (4 and 3 feeds, a short last one), one fed whole
E = rr.E2E
RCONF = {'beam_size': E['beam_size'], 'ctc_weight': E['ctc_weight'], 'cutoff_prob': E['cutoff_prob'], 'cutoff_top_n': E['cutoff_top_n']}


@pytest.fixture(scope='module')
def sd():
    return _sd()


@pytest.fixture(scope='module')
def pcm():
    from masr_amd.utils import synthetic
    x = synthetic.synthetic_pcm(len(LENS), max(LENS), seed=E['pcm_seed'])
    return [x[i, :n].copy() for i, n in enumerate(LENS)]


def _predictor(tmp, sd, decoder, **more):
    from masr_amd.predict import MASRPredictor
    return MASRPredictor(configs=_cfg(str(tmp), decoder, **more), use_gpu=True, state_dict=sd)


@pytest.fixture(scope='module')
def resc(tmp_path_factory, sd):
    """the predictor under test: the second pass at the end of streams asked for"""
    return _predictor(tmp_path_factory.mktemp('resc'), sd, 'attention_rescoring',
                      attention_rescoring_decoder_conf=dict(RCONF, on_streams='rescore_at_end'))


@pytest.fixture(scope='module')
def ctc(tmp_path_factory, sd):
    """the first pass alone: ctc_beam_search with alpha = beta = 0, the same beam and cutoffs"""
    conf = {'alpha': 0, 'beta': 0, 'beam_size': E['beam_size'], 'cutoff_prob': E['cutoff_prob'], 'cutoff_top_n': E['cutoff_top_n'],
            'num_processes': 2, 'language_model_path': None}
    return _predictor(tmp_path_factory.mktemp('ctc'), sd, 'ctc_beam_search', ctc_beam_search_decoder_conf=conf)


def _feeds(pcm):
    """[(session index, bytes, is_end)] per step: sessions 0 and 1 in 0.64 s chunks, session 2 whole in the first step"""
    steps = []
    for k in range(-(-max(LENS[:2]) // CHUNK)):
        step = []
        for i in (0, 1):
            if k * CHUNK < LENS[i]:
                step.append((i, pcm[i][k * CHUNK:(k + 1) * CHUNK].tobytes(), (k + 1) * CHUNK >= LENS[i]))
        if k == 0:
            step.append((2, pcm[2].tobytes(), True))
        steps.append(step)
    return steps


def _run(pool, pcm, handles=None):
    """-> (handles, [{session index: (result, is_end)} per step])"""
    handles = handles or [pool.open() for _ in LENS]
    seen = []
    for step in _feeds(pcm):
        for i, data, end in step:
            pool.feed(handles[i], data, end)
        out = pool.step()
        seen.append({i: (out[handles[i]], end) for i, _, end in step})
    return handles, seen


def _table(nbest):
    L = max(1, max(len(t) for t in nbest))
    hyps, lens = np.zeros((1, len(nbest), L), np.int32), np.array([[len(t) for t in nbest]], np.int32)
    for n, t in enumerate(nbest):
        hyps[0, n, :len(t)] = t
    return hyps, lens


def _check_end(pool, h, res, sd, dec, name):
    """the result ``res`` of the step that ended session ``h``, reproduced offline from what the pool kept: its gathered encoder
    rows through masr_rescore (att / r_att bit for bit the record's), combine + pick on the host (the returned text and score),
    and att / r_att under the float64 budget on that memory"""
    from masr_amd.decoders.attention_rescoring import combine, pick
    eng, rec = pool.engine, pool.last_rescoring(h)
    assert 1 <= len(rec['nbest']) <= E['beam_size'] and len({tuple(t) for t in rec['nbest']}) == len(rec['nbest'])
    rows = pool.encoder_rows(h)
    memory = pool.encoder_output(h)
    assert rows.dtype == np.int64 and len(rows) == memory.shape[0] > 0 and len(set(rows.tolist())) == len(rows)
    hyps, lens = _table(rec['nbest'])
    fr = torch.tensor([memory.shape[0]], dtype=torch.int32, device=eng.device)
    att, r_att = eng.rescore(memory[None].contiguous(), fr, torch.from_numpy(hyps).to(eng.device),
                             torch.from_numpy(lens).to(eng.device), with_right=dec.reverse_weight > 0)
    att, r_att = att.cpu().numpy()[0], r_att.cpu().numpy()[0]
    assert np.array_equal(att, np.asarray(rec['att'], np.float32)), (name, att, rec['att'])
    assert np.array_equal(r_att, np.asarray(rec['r_att'], np.float32)), (name, r_att, rec['r_att'])
    total = combine(att, r_att, np.asarray(rec['ctc'], np.float32), dec.ctc_weight, dec.reverse_weight)
    w = pick(total)
    assert w == rec['winner'] and total.tolist() == rec['total']
    assert res == {'text': token_text(pool.vocab, rec['nbest'][w]), 'score': float(total[w])}, (name, res)
    assert pool.last_tokens(h) == rec['nbest'][w]
    mem = memory.cpu().numpy()[None]
    a64 = rr.scores(rr.to64(sd), mem, [mem.shape[1]], hyps, lens)
    a32 = rr.scores(sd, mem, [mem.shape[1]], hyps, lens)
    budget.check(f'{name} att', a64[0], a32[0], att[None])
    budget.check(f'{name} r_att', a64[1], a32[1], r_att[None])


def test_partials_are_the_first_pass_and_the_end_is_reproduced_offline(resc, ctc, sd, pcm):
    from masr_amd.serving import LockStepPool, StreamPool
    pool, first = StreamPool(resc), StreamPool(ctc)
    assert isinstance(pool, LockStepPool) and pool.framing == 'python' and pool.rescoring
    dec = resc.rescoring_decoder
    try:
        hs, got = _run(pool, pcm)
        _, want = _run(first, pcm)
        ended = 0
        for step, (g, w) in enumerate(zip(got, want)):
            assert g.keys() == w.keys()
            for i in g:
                (res, end), (ref, _) = g[i], w[i]
                if not end:                                     # a partial result: the first pass's, text and score exact
                    assert res == ref, (step, i, res, ref)
                    continue
                ended += 1
                rec = pool.last_rescoring(hs[i])
                # the first pass behind the last window is the CTC predictor's final result
                assert ref is not None and token_text(pool.vocab, rec['nbest'][0]) == ref['text'] and rec['ctc'][0] == ref['score'], \
                    (i, rec, ref)
                _check_end(pool, hs[i], res, sd, dec, f'session {i}')
        assert ended == 3 and dec.reverse_weight > 0
        assert pool._enc_alloc.in_use == sum(len(pool.encoder_rows(h)) for h in hs) > 0
        for h in hs:
            pool.close(h)
        assert pool._enc_alloc.in_use == 0
    finally:
        pool.shutdown()
        first.shutdown()


def test_an_end_without_a_window_rescores_the_live_set_and_no_frames_is_the_ctc_path(resc, sd, pcm):
    from masr_amd.serving import StreamPool
    pool = StreamPool(resc)
    try:
        h, empty = pool.open(), pool.open()
        pool.feed(h, pcm[2][:10960].tobytes(), False)            # 67 feature frames: one full window, 3 frames carried over
        pool.feed(empty, pcm[1][:800].tobytes(), True)          # 3 feature frames: below the context, never an encoder frame
        out = pool.step()
        partial = out[h]
        assert partial is not None and out[empty] is None and pool.last_rescoring(empty) is None
        assert len(pool.encoder_rows(empty)) == 0
        n = len(pool.encoder_rows(h))
        assert n == pool.engine.out_frames(67)
        pool.feed(h, pcm[2][10960:11120].tobytes(), True)       # one more frame, 4 pending: below the context, no window
        res = pool.step()[h]
        rec = pool.last_rescoring(h)
        assert len(pool.encoder_rows(h)) == n and token_text(pool.vocab, rec['nbest'][0]) == partial['text']
        assert rec['ctc'][0] == partial['score']
        _check_end(pool, h, res, sd, resc.rescoring_decoder, 'live set')
    finally:
        pool.shutdown()


def test_rows_are_released_timestamps_compose_and_predict_stream_is_a_pool_of_one(resc, pcm):
    from masr_amd.serving import StreamPool
    pool = StreamPool(resc, timestamps=True)
    try:
        hs, got = _run(pool, pcm)
        finals = {i: r for g in got for i, (r, end) in g.items() if end}
        recs = {i: pool.last_rescoring(hs[i]) for i in finals}
        for i, res in finals.items():                          # the winner's tokens are what is aligned
            assert res['tokens'] is not None and ''.join(t['token'] for t in res['tokens']) == res['text'], (i, res)
            assert len(res['tokens']) == len(recs[i]['nbest'][recs[i]['winner']])
        for g in got:                                          # the partial results carry the first pass's alignment
            for i, (r, end) in g.items():
                if r is not None and not end:
                    assert ''.join(t['token'] for t in r['tokens']) == r['text']
        rows = {i: pool.encoder_rows(hs[i]).copy() for i in finals}
        assert all(len(pool.posterior_rows(hs[i])) == len(rows[i]) for i in finals)
        # reset: the rows go back, and the same audio on the same handles gives the same bits
        for h in hs:
            pool.reset(h)
        assert pool._enc_alloc.in_use == 0 and pool._alloc.in_use == 0
        _, again = _run(pool, pcm, hs)
        for g, a in zip(got, again):
            assert g == a
        for i in finals:
            assert pool.last_rescoring(hs[i]) == recs[i]
            assert sorted(pool.encoder_rows(hs[i]).tolist()) != [] and len(pool.encoder_rows(hs[i])) == len(rows[i])
        for h in hs:
            pool.close(h)
        assert pool._enc_alloc.in_use == 0 and pool._alloc.in_use == 0
    finally:
        pool.shutdown()
    # the single-session path: predict_stream(..., is_end=True) is the pool's result
    resc.reset_stream()
    for k in range(-(-LENS[0] // CHUNK)):
        end = (k + 1) * CHUNK >= LENS[0]
        one = resc.predict_stream(pcm[0][k * CHUNK:(k + 1) * CHUNK].tobytes(), is_end=end)
        want = {key: v for key, v in got[k][0][0].items() if key != 'tokens'} if got[k][0][0] is not None else None
        assert one == want, (k, one, want)
    resc.reset_stream()


def test_without_the_key_streams_are_refused_as_before(tmp_path, sd):
    from masr_amd.decoders.attention_rescoring import STREAM_REFUSAL
    from masr_amd.serving import StreamPool
    plain = _predictor(tmp_path, sd, 'attention_rescoring')
    with pytest.raises(Exception) as err:
        StreamPool(plain)
    assert str(err.value) == STREAM_REFUSAL
    with pytest.raises(Exception) as err:
        plain.predict_stream(b'\x00' * 3200)
    assert str(err.value) == STREAM_REFUSAL and plain._pool is None


def test_still_refused_by_name_with_the_key(resc):
    """nbest= (as offline) and the sharded pool"""
    from masr_amd.parallel import ShardedStreamPool
    from masr_amd.serving import StreamPool
    with pytest.raises(ValueError, match="nbest=2 with decoder='attention_rescoring'"):
        StreamPool(resc, nbest=2)
    with pytest.raises(ValueError, match="nbest=2 with decoder='attention_rescoring'"):
        resc.predict_stream(b'\x00' * 3200, nbest=2)
    pool = StreamPool(resc)
    try:
        with pytest.raises(Exception, match='ShardedStreamPool does not take'):
            ShardedStreamPool(pool)
    finally:
        pool.shutdown()
