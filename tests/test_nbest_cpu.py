"""CPU: the n-best arguments of BeamSearchDecoder and the validation of masr_op_beam_nbest -- refusals by name, the unpacking of the
packed n-best rows [B, N, max_len + 2] + counts on a hand-made array, and the LM-free host-thread n-best next to the host search's
own result.  Nothing here needs a GPU: the op validates every index before it touches its engine."""
import types

import numpy as np
import pytest

from tests import beam_nbest_ref as ref
from tests.test_gpu_beam_nbest_op import _refused


def _decoder(beam=8, V=12):
    from masr_amd.decoders.beam_search_decoder import BeamSearchDecoder
    vocab = ['<blank>'] + [chr(ord('a') + i) for i in range(V - 2)] + ['<space>']
    return BeamSearchDecoder(alpha=0, beta=0, beam_size=beam, cutoff_prob=1.0, cutoff_top_n=40, vocab_list=vocab, num_processes=2,
                             language_model_path=None)


def test_nbest_must_be_an_integer_in_1_to_beam_size(built_lib):
    dec = _decoder(beam=8)
    assert dec.check_nbest(None) is None and dec.check_nbest(1) == 1 and dec.check_nbest(np.int32(8)) == 8
    for bad in (0, 9, -1, True, False, 2.0, '3'):
        with pytest.raises(ValueError, match=r'nbest must be an integer in 1 \.\. beam_size = 8'):
            dec.check_nbest(bad)
    with pytest.raises(ValueError, match='nbest must be an integer'):
        dec._batch([np.full((3, 12), 1 / 12, np.float32)], nbest=0)
    with pytest.raises(ValueError, match='nbest must be an integer'):
        dec.decode_chunk(np.full((1, 3, 12), 1 / 12, np.float32), [3], nbest=9)


def test_packed_nbest_rows_unpack_to_count_results_per_utterance(built_lib):
    dec = _decoder()
    B, N, max_len = 2, 3, 4
    rows = np.full((B, N, max_len + 2), -7, np.int32)
    scores = np.array([[-1.5, -2.25, -np.inf], [-0.5, -np.inf, -np.inf]], np.float32)
    rows[:, :, max_len + 1] = scores.view(np.int32)
    rows[0, 0, :3], rows[0, 0, max_len] = [1, 2, 11], 3
    rows[0, 1, :0], rows[0, 1, max_len] = [], 0                        # the empty prefix
    rows[0, 2, max_len] = 0                                            # past count
    rows[1, 0, :4], rows[1, 0, max_len] = [3, 3, 4, 5], 4
    rows[1, 1:, max_len] = 0
    flat = np.concatenate([rows.reshape(-1), np.array([2, 1], np.int32)])
    assert dec._unpacked_nbest(flat, B, N, max_len, True) == [[([1, 2, 11], -1.5), ([], -2.25)], [([3, 3, 4, 5], -0.5)]]
    assert dec._unpacked_nbest(flat, B, N, max_len, False) == [[(-1.5, 'ab '), (-2.25, '')], [(-0.5, 'ccde')]]


def test_host_thread_nbest_is_lm_free_and_entry_0_is_the_host_result(built_lib):
    from oracle import beam_search as obs
    dec = _decoder(beam=6)
    rng = np.random.default_rng(3)
    probs = rng.dirichlet(np.ones(12) * 0.4, size=15).astype(np.float32)
    T, K = 15, 12
    idx, logp, cnt = np.zeros((T, K), np.int32), np.zeros((T, K), np.float32), np.zeros(T, np.int32)
    for t in range(T):
        c = obs.pruned_log_probs(probs[t], 1.0, 40)
        cnt[t] = len(c)
        for k, (i, lp) in enumerate(c):
            idx[t, k], logp[t, k] = i, lp
    frames = np.array([T], np.int32)
    best = dec._search_host(idx, logp, cnt, None, frames, 1, T, K, True)[0]
    many = dec._search_host_nbest(idx, logp, cnt, frames, 1, T, K, 4, True)[0]
    assert len(many) == 4 and many[0] == best
    assert [s for _, s in many] == sorted((s for _, s in many), reverse=True) and len({tuple(t) for t, _ in many}) == 4
    # with a scorer bound the host-thread search has no n-best: refused by name, word-based and character-based alike
    for character_based, kind in ((False, 'word-based'), (True, 'character-based')):
        dec._ext_scorer = types.SimpleNamespace(is_character_based=character_based)
        try:
            with pytest.raises(ValueError, match=f'nbest is not available from the host-thread search.*{kind}'):
                dec._search_host_nbest(idx, logp, cnt, frames, 1, T, K, 4, True)
        finally:
            dec._ext_scorer = None


def test_host_streaming_search_refuses_nbest_by_name(built_lib):
    dec = _decoder()
    dec.use_gpu_search = False
    with pytest.raises(ValueError, match='nbest of a streaming search comes from the device-resident search'):
        dec.decode_chunk(np.full((1, 3, 12), 1 / 12, np.float32), [3], nbest=2)


def _stub_predictor(decoder, dec=None):
    """a MASRPredictor with nothing but what the argument checks read (they come before any audio or engine is touched)"""
    from masr_amd.predict import MASRPredictor
    pred = object.__new__(MASRPredictor)
    pred.configs = types.SimpleNamespace(decoder=decoder, streaming=True, use_model='conformer')
    pred.beam_search_decoder = dec
    return pred


def _every_call(pred, nbest):
    yield lambda: pred.predict(audio_data=np.zeros(16000, np.int16), nbest=nbest)
    yield lambda: pred.predict_batch([np.zeros(16000, np.int16)], nbest=nbest)
    yield lambda: pred.predict_batch_deferred([np.zeros(16000, np.int16)], nbest=nbest)
    yield lambda: pred.predict_long(audio_data=np.zeros(16000, np.int16), nbest=nbest)
    yield lambda: pred.predict_stream(np.zeros(1600, np.int16).tobytes(), nbest=nbest)


def test_the_predictor_refuses_nbest_by_name_before_it_touches_audio(built_lib):
    for decoder, words in (('ctc_greedy', "only decoder='ctc_beam_search' keeps more than one hypothesis"),
                           ('attention_rescoring', 'the n-best of attention_rescoring .* is not this one'),
                           ('attention', 'the n-best of attention .* is not this one')):
        for call in _every_call(_stub_predictor(decoder), 3):
            with pytest.raises(ValueError, match=words):
                call()
    pred = _stub_predictor('ctc_beam_search', _decoder(beam=8))
    for bad in (0, True, 9, 2.5):
        for call in _every_call(pred, bad):
            with pytest.raises(ValueError, match=r'nbest must be an integer in 1 \.\. beam_size = 8'):
                call()
    pred.beam_search_decoder._ext_scorer = types.SimpleNamespace(is_character_based=False)
    try:
        for call in _every_call(pred, 3):
            with pytest.raises(ValueError, match='nbest with a word-based language model'):
                call()
    finally:
        pred.beam_search_decoder._ext_scorer = None
    # the pass itself refuses what its caller should have: no n-best for another decoder or for token results (the sharded path)
    from masr_amd.offline_pass import empty_result
    assert empty_result(False, False, 3) == {'text': '', 'score': 0, 'nbest': [{'text': '', 'score': 0}]}
    assert empty_result(False, False) == {'text': '', 'score': 0}


def test_first_pass_is_host_by_default_and_an_unknown_value_is_refused_by_name(built_lib):
    from masr_amd._lib import MasrError
    from masr_amd.decoders.attention_rescoring import AttentionRescoringDecoder, validate_rescoring_conf
    assert 'first_pass' not in validate_rescoring_conf(None)          # not named: the decoder's default below
    assert validate_rescoring_conf({'first_pass': 'host'})['first_pass'] == 'host'
    assert validate_rescoring_conf({'first_pass': 'gpu'})['first_pass'] == 'gpu'
    for bad in ('device', 'GPU', None, 1):
        with pytest.raises(MasrError, match='attention_rescoring_decoder_conf.first_pass=.* is not supported'):
            validate_rescoring_conf({'first_pass': bad})
    vocab = ['<blank>'] + [chr(ord('a') + i) for i in range(20)]
    assert AttentionRescoringDecoder(vocab, beam_size=4).first_pass == 'host'
    assert AttentionRescoringDecoder(vocab, beam_size=4, first_pass='gpu').first_pass == 'gpu'
    with pytest.raises(MasrError, match="first_pass='gpu' with beam_size=1.* is beyond the GPU prefix search"):
        AttentionRescoringDecoder(vocab, beam_size=1, first_pass='gpu')
    with pytest.raises(MasrError, match="first_pass='gpu' with beam_size=4, cutoff_top_n=80 is beyond the GPU prefix search"):
        AttentionRescoringDecoder(vocab + [str(i) for i in range(100)], beam_size=4, cutoff_top_n=80, first_pass='gpu')
    AttentionRescoringDecoder(vocab, beam_size=1, first_pass='host')
    with pytest.raises(MasrError, match='first_pass'):
        AttentionRescoringDecoder(vocab, beam_size=4, first_pass='device')


def test_the_test_op_validates_every_index_before_it_touches_an_engine(built_lib):
    """(no engine at all: a call that passed validation would fail with 'null engine', which names no index; the reference the
    op is held to on the GPU is checked on a hand-made case first)"""
    score = np.array([-1.0, -np.inf, -1.0, 0.0, -1.0, -np.inf], np.float32)
    ch = np.array([5, 1, 2, 9, 2, 0], np.int32)
    assert ref.rank_order(score, ch) == [3, 2, 4, 0, 5, 1]
    parent = np.array([-1, 0, 1, 1, 3], np.int32)
    pch = np.array([-1, 7, 8, 9, 4], np.int32)
    toks, lens, out, count = ref.nbest(3, [4, 0, 2], [4, -1, 8], np.array([-2.0, -1.0, -2.0], np.float32), parent, pch, 4, 2)
    assert count == 3 and lens.tolist() == [0, 3, 2, 0] and toks[1].tolist() == [7, 9] and toks[2].tolist() == [7, 8]
    assert out[:3].tolist() == [-1.0, -2.0, -2.0] and np.isneginf(out[3]) and (toks[3] == -7).all() and (toks[0] == -7).all()

    _refused(None, 'nbest = 0', nbest=0)
    _refused(None, 'nbest = 9', nbest=9)
    _refused(None, 'max_len', max_len=0)
    _refused(None, 'n_live', n_live=(9,))
    _refused(None, 'n_live', n_live=(4, -1))
    _refused(None, 'beam_size', beam=513, nbest=3)

    def node_out(node, parent):
        node[0, 2] = 700
    _refused(None, 'outside the pool', edit=node_out)

    def parent_up(node, parent):
        parent[0, 40] = 41
    _refused(None, 'parent of pool node 40', edit=parent_up)
