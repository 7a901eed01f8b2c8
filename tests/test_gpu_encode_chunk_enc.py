"""GPU: masr_encode_chunk_enc -- the chunk step that also hands out its encoder rows -- against masr_encode_chunk on a twin stream
fed the same chunks (every other output bit for bit, over consecutive steps), and the rows themselves through masr_ctc_probs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 50


def _engine(family):
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    if family == 'conformer':
        return HipEngine(synthetic.conformer_state_dict(1, V, d_ff=256, num_blocks=2), encoder_conf=dict(num_blocks=2, linear_units=256),
                         vocab_size=V)
    if family == 'conformer512':         # the width-generic path
        sd = synthetic.conformer_state_dict(5, V, d=512, heads=8, d_ff=256, num_blocks=1)
        return HipEngine(sd, encoder_conf=dict(output_size=512, attention_heads=8, num_blocks=1, linear_units=256), vocab_size=V)
    if family == 'squeezeformer':        # the streaming-trained build: the step's rows are written by the last FFN, n * T0 of them
        return HipEngine(synthetic.squeezeformer_state_dict(3, V, streaming=True), vocab_size=V, use_model='squeezeformer', streaming=True)
    return HipEngine(synthetic.efficient_conformer_state_dict(2, V, num_blocks=12), vocab_size=V, use_model='efficient_conformer',
                     streaming=True)


@pytest.fixture(scope='module', params=['conformer', 'conformer512', 'squeezeformer', 'efficient_conformer'])
def eng(request):
    e = _engine(request.param)
    yield e
    e.close()


@pytest.mark.parametrize('n', [1, 3])
def test_twin_streams_agree_bit_for_bit_and_the_rows_reproduce_the_probabilities(eng, n):
    """three consecutive steps, the last a short window (35 frames); n streams per call"""
    rng = np.random.default_rng(10 + n)
    plain = [eng.stream_open() for _ in range(n)]
    twin = [eng.stream_open() for _ in range(n)]
    try:
        for step, Tc in enumerate((67, 67, 35)):
            x = torch.from_numpy((rng.standard_normal((n, Tc, 80)) * 3 + 13).astype(np.float32)).to(eng.device)
            probs, idx, mp = eng.encode_chunk(plain, x, want_probs=True, want_argmax=True)
            out = eng.encode_chunk(twin, x, want_probs=True, want_argmax=True, want_enc=True)
            assert len(out) == 4
            probs2, idx2, mp2, enc = out
            assert enc.shape == (n, probs.shape[1], eng.d_model) and probs.shape[1] == eng.out_frames(Tc) > 0
            assert torch.equal(probs, probs2) and torch.equal(idx, idx2) and torch.equal(mp, mp2), (step, Tc)
            assert bool(torch.isfinite(enc).all()) and bool(enc.abs().sum() > 0)
            # the rows are what the step's CTC head read: the same head on them (the same M) gives the same bits
            again, idx3, mp3 = eng.ctc_probs(enc, want_argmax=True)
            assert torch.equal(again, probs) and torch.equal(idx3.view_as(idx), idx) and torch.equal(mp3.view_as(mp), mp), (step, Tc)
        assert [eng.stream_offset(s) for s in plain] == [eng.stream_offset(s) for s in twin]
        # without the probabilities (what a greedy caller asks for): argmax / maxprob as ever, and the same rows
        x = torch.from_numpy((rng.standard_normal((n, 67, 80)) * 3 + 13).astype(np.float32)).to(eng.device)
        _, idx, mp = eng.encode_chunk(plain, x, want_probs=False, want_argmax=True)
        none, idx2, mp2, enc = eng.encode_chunk(twin, x, want_probs=False, want_argmax=True, want_enc=True)
        assert none is None and torch.equal(idx, idx2) and torch.equal(mp, mp2)
        assert torch.equal(eng.ctc_probs(enc, want_argmax=True)[1].view_as(idx), idx)
    finally:
        for s in plain + twin:
            eng.stream_close(s)


def test_deepspeech2_is_refused_by_name():
    from masr_amd._lib import MasrError
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sd = synthetic.deepspeech2_state_dict(0, 64, rnn_size=256, num_rnn_layers=1, bidirectional=False)
    e = HipEngine(sd, encoder_conf={'num_rnn_layers': 1, 'rnn_size': 256}, vocab_size=64, streaming=True, use_model='deepspeech2')
    try:
        sid = e.stream_open()
        x = torch.zeros(1, 67, 80, device=e.device)
        with pytest.raises(MasrError, match='masr_encode_chunk_enc: use_model deepspeech2'):
            e.encode_chunk([sid], x, want_enc=True)
        probs, _, _ = e.encode_chunk([sid], x)                 # the step without the rows runs as ever
        assert probs.shape[0] == 1
        e.stream_close(sid)
    finally:
        e.close()
