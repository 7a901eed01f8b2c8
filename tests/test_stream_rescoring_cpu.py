"""CPU: what ``attention_rescoring_decoder_conf.on_streams`` needs no GPU for -- the key's validation, the refusal streams get
without it, the refusals of masr_rescore_rows before it needs a device, and the row bookkeeping of the pool's second
``RowAllocator`` (the encoder rows of ``'rescore_at_end'`` sessions) across reset and close."""
import ctypes as C

import numpy as np
import pytest
import torch

from masr_amd import _lib
from masr_amd.decoders import attention_rescoring as ar


def test_validate_rescoring_conf_takes_the_two_values_and_refuses_a_third_by_name():
    assert 'on_streams' not in ar.validate_rescoring_conf(None)                      # not named: what the decoder always got
    assert 'on_streams' not in ar.validate_rescoring_conf({'beam_size': 4})
    for value in ('refuse', 'rescore_at_end'):
        assert ar.validate_rescoring_conf({'on_streams': value})['on_streams'] == value
        dec_kw = ar.validate_rescoring_conf({'on_streams': value, 'beam_size': 4})
        assert dec_kw['beam_size'] == 4 and set(dec_kw) - {'on_streams'} == set(ar.validate_rescoring_conf({'beam_size': 4}))
    for bad in ('rescore', True, None, 1, 'Refuse'):
        with pytest.raises(_lib.MasrError, match=r'attention_rescoring_decoder_conf\.on_streams=.* is not supported: one of'):
            ar.validate_rescoring_conf({'on_streams': bad})
    assert ar.ON_STREAMS == ('refuse', 'rescore_at_end')


def test_the_refusal_keeps_its_pinned_words_and_names_the_key():
    assert 'predict_stream' in ar.STREAM_REFUSAL and 'left out' in ar.STREAM_REFUSAL
    assert 'attention_rescoring_decoder_conf.on_streams' in ar.STREAM_REFUSAL and 'rescore_at_end' in ar.STREAM_REFUSAL


def _configs(**block):
    from masr_amd.utils.utils import dict_to_object
    cfg = {'streaming': True, 'use_model': 'conformer', 'decoder': 'attention_rescoring'}
    if block:
        cfg['attention_rescoring_decoder_conf'] = block.get('conf')
    return dict_to_object(cfg)


def test_on_streams_of_a_configuration():
    assert ar.on_streams(_configs()) == 'refuse'                                     # no block at all
    assert ar.on_streams(_configs(conf=None)) == 'refuse'
    assert ar.on_streams(_configs(conf={'beam_size': 4})) == 'refuse'
    assert ar.on_streams(_configs(conf={'on_streams': 'refuse'})) == 'refuse'
    assert ar.on_streams(_configs(conf={'on_streams': 'rescore_at_end'})) == 'rescore_at_end'
    with pytest.raises(_lib.MasrError, match="on_streams='at_end' is not supported"):
        ar.on_streams(_configs(conf={'on_streams': 'at_end'}))


@pytest.mark.parametrize('conf', [None, {'beam_size': 4}, {'on_streams': 'refuse'}])
def test_pool_and_predict_stream_refuse_without_the_opt_in_before_anything_is_built(conf):
    from masr_amd.predict import MASRPredictor
    from masr_amd.serving import StreamPool

    class Stub:
        configs = _configs(conf=conf)
    with pytest.raises(Exception) as err:
        StreamPool(Stub())
    assert str(err.value) == ar.STREAM_REFUSAL
    pred = object.__new__(MASRPredictor)
    pred.configs, pred._pool = Stub.configs, None
    with pytest.raises(Exception) as err:
        pred.predict_stream(b'\x00' * 3200)
    assert str(err.value) == ar.STREAM_REFUSAL and pred._pool is None


def test_a_first_pass_beyond_the_device_search_is_refused_by_name_at_pool_construction():
    """beam_size 1 has no device-resident prefix search, so no live n-best to rescore"""
    from masr_amd.serving import StreamPool

    class Featurizer:
        vocab_list = ['<blank>'] + [chr(97 + i) for i in range(20)]

    class Pruner:
        cutoff_top_n = 40

        def gpu_search_supported(self, T, V):
            return False

    class Dec:
        beam_size, _pruner = 1, Pruner()

    class Stub:
        configs = _configs(conf={'on_streams': 'rescore_at_end', 'beam_size': 1})
        rescoring_decoder, _text_featurizer = Dec(), Featurizer()
    with pytest.raises(_lib.MasrError, match="on_streams='rescore_at_end' with beam_size=1, cutoff_top_n=40"):
        StreamPool(Stub())
    from masr_amd.decoders.beam_search_decoder import BeamSearchDecoder
    real = object.__new__(BeamSearchDecoder)
    real.cutoff_top_n, real.beam_size, real._ext_scorer = 40, 1, None
    assert not real.gpu_search_supported(1, 50)
    real.beam_size = 6
    assert real.gpu_search_supported(1, 50)


def test_rescore_rows_refuses_by_name_before_it_needs_a_device():
    lib = _lib.lib()
    err = lambda: lib.masr_last_error().decode()
    buf = np.ones(64, np.int32)
    p = buf.ctypes.data_as(C.c_void_p)
    call = lambda *a: lib.masr_rescore_rows(None, *a)
    # (rows, n_rows, frame_row, n_frames, B, Tmax, hyp, hyp_lens, N, Lmax, with_right, att, r_att, stream)
    assert call(p, 0, p, p, 1, 4, p, p, 1, 2, 1, p, p, None) != 0 and 'masr_rescore_rows: n_rows = 0' in err()
    assert call(p, -3, p, p, 1, 4, p, p, 1, 2, 1, p, p, None) != 0 and 'masr_rescore_rows: n_rows = -3' in err()
    assert call(p, 8, p, p, 1, 0, p, p, 1, 2, 1, p, p, None) != 0 and 'masr_rescore_rows: Tmax = 0' in err()
    assert call(p, 8, p, p, 1, 4, p, p, 65, 2, 1, p, p, None) != 0 and 'masr_rescore_rows: N = 65' in err() and 'outside 1 .. 64' in err()
    assert call(p, 8, p, p, 1, 4, p, p, 0, 2, 1, p, p, None) != 0 and 'outside 1 .. 64' in err()
    assert call(p, 8, p, p, 0, 4, p, p, 1, 2, 1, p, p, None) != 0 and 'B and Tp must be positive' in err()
    assert call(p, 8, p, p, 1, 4, p, p, 1, 0, 1, p, p, None) != 0 and 'Lmax must be at least 1' in err()
    assert call(p, 8, None, p, 1, 4, p, p, 1, 2, 1, p, p, None) != 0 and 'null argument' in err()
    assert call(None, 8, p, p, 1, 4, p, p, 1, 2, 1, p, p, None) != 0 and 'null argument' in err()
    assert call(p, 1 << 40, p, p, 1 << 15, 1 << 17, p, p, 1, 2, 1, p, p, None) != 0 and 'B * Tmax' in err()
    # accepted sizes fail only for want of an engine (a device); masr_rescore's own message is untouched
    assert call(p, 1 << 40, p, p, 1, 4, p, p, 1, 2, 1, p, p, None) != 0 and err() == 'engine not finalized'
    assert lib.masr_rescore(None, p, p, 1, 4, p, p, 1, 2, 1, p, p, None) != 0 and err() == 'engine not finalized'
    assert lib.masr_encode_chunk_enc(None, None, 1, p, 67, p, p, p, p, None) != 0 and err() == 'engine not finalized'


class _Engine:
    """what LockStepPool's constructor and session life cycle ask of an engine"""
    device, d_model, vocab_size = torch.device('cpu'), 256, 50

    def __init__(self):
        self.open, self.next = set(), 0

    def stream_open(self, max_frames_out=0):
        self.next += 1
        self.open.add(self.next)
        return self.next

    def stream_close(self, sid):
        self.open.remove(sid)

    def stream_reset(self, sid):
        assert sid in self.open

    def frame_reduction(self):
        return 4


class _Search:
    closed = resets = 0

    def fork(self):
        return _Search()

    def gpu_search_supported(self, T, V):
        return True

    def close(self):
        self.closed += 1

    def reset_decoder(self):
        self.resets += 1


@pytest.fixture
def pool(monkeypatch):
    """a rescore_at_end LockStepPool on a stand-in engine (no pinned staging area: the CPU build of torch has none)"""
    from masr_amd import serving
    from masr_amd.utils.utils import dict_to_object
    monkeypatch.setattr(serving, '_HostStage', lambda device: None)

    class Predictor:
        configs = dict_to_object({'streaming': True, 'use_model': 'conformer', 'decoder': 'attention_rescoring',
                                  'attention_rescoring_decoder_conf': {'on_streams': 'rescore_at_end'},
                                  'preprocess_conf': {'feature_method': 'fbank', 'use_dB_normalization': True, 'target_dB': -20}})

        class predictor:
            engine = _Engine()

        class _text_featurizer:
            vocab_list = ['<blank>'] + [chr(97 + i) for i in range(49)]

        class rescoring_decoder:
            beam_size, _pruner = 6, _Search()

        def _nbest(self, nbest):
            return None
    return serving.StreamPool(Predictor(), timestamps=True)


def test_the_second_allocator_releases_on_reset_and_close(pool):
    from masr_amd.serving import LockStepPool
    assert isinstance(pool, LockStepPool) and pool.rescoring and pool.beam and pool.timestamps
    assert pool._enc.shape == (0, 256) and pool._post.shape == (0, 50) and pool._enc_alloc is not pool._alloc
    a, b = pool.open(), pool.open()
    assert isinstance(pool.sessions[a].decoder, _Search) and pool.sessions[a].decoder is not pool.sessions[b].decoder
    assert pool.encoder_rows(a).tolist() == [] and pool.last_rescoring(a) is None
    # two lock-step calls of 16 frames per session, as the step appends them (the device index is the host's on this stand-in)
    pool._dev_index = lambda idx: torch.as_tensor(np.asarray(idx, np.int64))
    items = [(pool.sessions[a], None), (pool.sessions[b], None)]
    for call in range(2):
        enc = torch.full((2, 16, 256), float(call + 1))
        enc[1] += 10
        pool._enc = pool._append_rows(pool._enc_alloc, pool._enc, items, enc)
        pool._keep_posteriors(items, torch.zeros(2, 16, 50))
    assert pool._enc_alloc.in_use == 64 == pool._alloc.in_use and pool._enc.shape[0] == pool.ROW_SLAB
    ra, rb = pool.encoder_rows(a), pool.encoder_rows(b)
    assert ra.tolist() == list(range(16)) + list(range(32, 48)) and rb.tolist() == list(range(16, 32)) + list(range(48, 64))
    assert pool._enc[ra][:, 0].tolist() == [1.0] * 16 + [2.0] * 16 and pool._enc[rb][:, 0].tolist() == [11.0] * 16 + [12.0] * 16
    pool.reset(a)                                             # a new utterance: both histories go back, the session stays
    assert pool.encoder_rows(a).tolist() == [] and pool.posterior_rows(a).tolist() == []
    assert pool._enc_alloc.in_use == 32 == pool._alloc.in_use and pool.sessions[a].decoder.resets == 1
    assert pool.encoder_rows(b).tolist() == rb.tolist()
    pool._enc = pool._append_rows(pool._enc_alloc, pool._enc, items[:1], torch.full((1, 16, 256), 5.0))
    reused = pool.encoder_rows(a)
    assert set(reused.tolist()) <= set(ra.tolist()) and pool._enc[reused][:, 0].tolist() == [5.0] * 16      # freed rows first
    assert pool._enc[rb][:, 0].tolist() == [11.0] * 16 + [12.0] * 16                                         # b's rows untouched
    pool.close(a)
    pool.close(b)
    assert pool._enc_alloc.in_use == 0 == pool._alloc.in_use and not pool.engine.open


def test_pools_of_other_decoders_keep_no_encoder_rows():
    from masr_amd import serving
    base = object.__new__(serving.StreamPool)
    for fn in (base.encoder_rows, base.last_rescoring, base.encoder_output):
        with pytest.raises(_lib.MasrError, match="keeps no encoder rows"):
            fn(1)
