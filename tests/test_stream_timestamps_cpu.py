"""CPU: the host side of token timestamps on streaming sessions -- the row bookkeeping of the posterior pool
(masr_amd/posterior_rows.py), the times of a partial stream (decoders/ctc_alignment.py) and the ``timestamps`` flag of
``MASRPredictor.predict_stream``.  The kernel and the pool itself: tests/test_gpu_stream_timestamps.py."""
import numpy as np
import pytest

from masr_amd.decoders import ctc_alignment as ca
from masr_amd.posterior_rows import RowAllocator


# ---- the row allocator ------------------------------------------------------------------------------------------------------------
def _owned(alloc, owners):
    rows = [r for o in owners for r in alloc.rows_of(o)]
    assert len(rows) == len(set(rows)), 'a row is owned twice'
    assert all(0 <= r < alloc.capacity for r in rows)
    assert alloc.in_use == len(rows)
    return rows


def test_rows_interleave_free_reuse_and_grow_by_slabs():
    a = RowAllocator(slab=64)
    assert a.capacity == 0
    mine = {1: [], 2: [], 3: []}
    # three sessions advance in lock-step, 16 rows each per call, then at different speeds
    for owner in (1, 2, 3, 1, 2, 1):
        got = a.take(owner, 16)
        assert got.dtype == np.int64 and got.shape == (16,)
        mine[owner].extend(got.tolist())
        assert a.rows_of(owner) == mine[owner]                 # frame order = the order in which the rows were taken
    assert a.capacity == 128 and a.fresh == 96                 # two slabs of 64 hold the 96 rows
    _owned(a, (1, 2, 3))
    assert a.rows_of(1)[16:32] != list(range(16, 32))          # interleaved: session 1's second chunk lies behind 2's and 3's first
    # reset of session 2: its rows are free, its list is empty, the others keep theirs
    assert a.release(2) == 32 and a.rows_of(2) == [] and a.in_use == 64
    freed = set(mine[2])
    # session 3 takes a short window (8) and a full one: both land in the freed rows before any fresh row is touched
    got = np.concatenate([a.take(3, 8), a.take(3, 16)])
    assert set(got.tolist()) <= freed and a.fresh == 96
    mine[3].extend(got.tolist())
    assert a.rows_of(3) == mine[3] and sorted(mine[3]) != mine[3]          # neither contiguous nor increasing
    # session 2 runs again: the 8 freed rows that are left, then fresh ones
    got = a.take(2, 16).tolist()
    assert set(got[:8]) <= freed and got[8:] == list(range(96, 104))
    _owned(a, (1, 2, 3))
    # close of session 1, then a take larger than everything free: a slab more
    a.release(1)
    before = a.capacity
    a.take(4, 48 + (before - a.fresh) + 1)
    assert a.capacity == before + 64 and a.capacity % 64 == 0
    _owned(a, (2, 3, 4))
    assert a.release(99) == 0                                   # a session that never advanced
    with pytest.raises(ValueError):
        RowAllocator(0)


def test_a_take_of_nothing_and_many_slabs_at_once():
    a = RowAllocator(slab=10)
    assert a.take('s', 0).shape == (0,) and a.capacity == 0 and a.rows_of('s') == []
    assert a.take('s', 35).tolist() == list(range(35)) and a.capacity == 40


# ---- times of a partial stream ----------------------------------------------------------------------------------------------------
VOCAB = ['<blank>', '<unk>', '<space>', 'a', 'b', 'c']


def test_partial_stream_times_come_from_frames_and_end_is_clamped_to_the_audio_fed():
    # 20 encoder frames of a conv2d model (reduction 4: 40 ms per frame) decoded, 0.79 s of audio fed so far
    ids = [3, 2, 4]
    start, end = np.array([2, 7, 18, -1], np.int32), np.array([4, 7, 19, -1], np.int32)
    peak = np.log(np.array([0.5, 0.25, 1.0, 1.0], np.float32))
    toks = ca.utterance_tokens(ids, start, end, peak, np.float32(-3.0), 0, 4, 16000, 0.79, VOCAB)
    assert [t['token'] for t in toks] == ['a', ' ', 'b']
    assert [t['start'] for t in toks] == [2 * 0.04, 7 * 0.04, 18 * 0.04]
    assert [t['end'] for t in toks] == [5 * 0.04, 8 * 0.04, 0.79]          # (19 + 1) * 0.04 = 0.8 > 0.79: clamped
    assert toks[0]['score'] == pytest.approx(0.5) and toks[2]['score'] == 1.0
    # the Efficient-Conformer's frames are 80 ms; a model at 8 kHz has 20 ms feature frames
    assert ca.utterance_tokens([3], [1], [1], [0.0], -1.0, 0, 8, 16000, 10.0, VOCAB)[0]['end'] == 2 * 0.08
    assert ca.utterance_tokens([3], [1], [1], [0.0], -1.0, 0, 4, 8000, 10.0, VOCAB)[0]['start'] == 0.08


def test_empty_no_path_and_the_token_cap():
    assert ca.utterance_tokens([], [], [], [], 0.0, 0, 4, 16000, 1.0, VOCAB) == []
    assert ca.utterance_tokens([3], [-1], [-1], [0.0], 0.0, 1, 4, 16000, 1.0, VOCAB) is None
    assert ca.utterance_tokens([3], [0], [0], [0.0], ca.SENTINEL, 0, 4, 16000, 1.0, VOCAB) is None
    # three sessions of one step: the longest history has 3000 frames; a hypothesis beyond MASR_ALIGN_MAX_TOKENS goes in empty
    long = [3, 4] * 513
    flat, lmax, ok = ca.pack_hypotheses([[3, 4, 4], [], long], 3000)
    assert ok.tolist() == [True, True, False] and lmax == 3 and flat.tolist() == [3, 4, 4, 0, 0, 0, 0, 0, 0, 3, 0, 0]
    # ... and comes out as None whatever the kernel said about the empty stand-in
    assert ca.utterance_tokens(long, [-1], [-1], [0.0], 0.0, 0 if ok[2] else 1, 4, 16000, 99.0, VOCAB) is None
    # exactly at the cap it is kept
    assert ca.pack_hypotheses([[3] * ca.MAX_TOKENS], 3000)[2].tolist() == [True]


# ---- the flag of predict_stream ---------------------------------------------------------------------------------------------------
class _Pool:
    made = []

    def __init__(self, timestamps):
        self.timestamps, self.log, self.alive = timestamps, [], True
        _Pool.made.append(self)

    def open(self):
        return 7

    def feed(self, handle, audio, is_end, **kw):
        self.log.append(('feed', handle, is_end))

    def step(self):
        return {7: {'text': 'x', 'score': 1.0, **({'tokens': []} if self.timestamps else {})}}

    def reset(self, handle):
        self.log.append(('reset', handle))

    def close(self, handle):
        self.log.append(('close', handle))

    def shutdown(self):
        self.alive = False


@pytest.fixture
def facade(monkeypatch):
    from masr_amd.predict import MASRPredictor

    class Cfg:
        streaming, decoder, use_model = True, 'ctc_greedy', 'conformer'

    class Inner:
        def reset_stream(self):
            pass
    _Pool.made = []
    p = object.__new__(MASRPredictor)
    p.configs, p.predictor = Cfg, Inner()
    p._pool, p._session, p._pool_timestamps, p._stream_running = None, None, False, False
    monkeypatch.setattr(MASRPredictor, '_new_stream_pool', lambda self, timestamps: _Pool(timestamps))
    monkeypatch.setattr(MASRPredictor, '_no_itn', lambda self, is_itn: None)
    return p


def test_the_first_call_of_an_utterance_decides(facade):
    from masr_amd._lib import MasrError
    assert set(facade.predict_stream(b'\0\0', timestamps=True)) == {'text', 'score', 'tokens'}
    assert facade.predict_stream(b'\0\0', timestamps=True) is not None and len(_Pool.made) == 1 and _Pool.made[0].timestamps
    with pytest.raises(MasrError, match='reset_stream'):
        facade.predict_stream(b'\0\0')                          # the default is False: a mismatch
    with pytest.raises(MasrError, match='reset_stream'):
        facade.predict_stream(b'\0\0', timestamps=False)
    assert len(_Pool.made) == 1 and _Pool.made[0].alive           # the refusal left the running utterance alone
    facade.reset_stream()
    assert set(facade.predict_stream(b'\0\0')) == {'text', 'score'}          # the other value is accepted now: a new pool
    assert len(_Pool.made) == 2 and not _Pool.made[1].timestamps
    assert not _Pool.made[0].alive and ('close', 7) in _Pool.made[0].log
    with pytest.raises(MasrError, match='reset_stream'):
        facade.predict_stream(b'\0\0', timestamps=True)
    facade.reset_stream()
    facade.predict_stream(b'\0\0', timestamps=True)
    assert len(_Pool.made) == 3 and _Pool.made[2].timestamps


def test_without_the_flag_no_timestamps_pool_is_ever_made(facade):
    for _ in range(3):
        facade.predict_stream(b'\0\0')
        facade.predict_stream(b'\0\0', is_end=True)
        facade.reset_stream()
    assert len(_Pool.made) == 1 and not _Pool.made[0].timestamps            # one pool, reset between the utterances
    assert [e for e in _Pool.made[0].log if e[0] == 'reset'] == [('reset', 7)] * 3


def test_the_real_factory_passes_the_flag_on(monkeypatch):
    """``_new_stream_pool``: StreamPool(self) exactly as before without the flag, StreamPool(self, timestamps=True) with it"""
    import masr_amd.serving as serving
    from masr_amd.predict import MASRPredictor
    seen = []
    monkeypatch.setattr(serving, 'StreamPool', lambda *a, **kw: seen.append((len(a), kw)))
    p = object.__new__(MASRPredictor)
    p._new_stream_pool(False)
    p._new_stream_pool(True)
    assert seen == [(1, {}), (1, {'timestamps': True})]
