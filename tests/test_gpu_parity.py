"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle, the committed golden
fixtures generated from the real reference, and size-independent properties at BASELINE sizes.

Tolerances (north_star): fbank <= 1e-3 in the log domain, encoder / probabilities <= 1e-3 fp32,
greedy transcript identical, integer outputs bit-exact (up to the documented +-1 LSB gain effect).
"""
import os

import numpy as np
import pytest
import torch

from masr_amd._lib import debug_keys
from tests import budget

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


def g(name):
    return np.load(os.path.join(GOLDEN, name))


@pytest.fixture(scope='module')
def oracle_mods():
    from oracle import conformer as oc, decoders as od, fbank as ofb, weights
    from oracle.make_golden import golden_inputs
    return oc, od, ofb, weights, golden_inputs


@pytest.fixture(scope='module')
def eng512(oracle_mods):
    from masr_amd.engine import HipEngine
    oc, od, ofb, weights, _ = oracle_mods
    sd = weights.conformer_state_dict(0, 512)
    e = HipEngine(sd, vocab_size=512)
    yield e, sd
    e.close()


@pytest.fixture(scope='module')
def eng4233(oracle_mods):
    from masr_amd.engine import HipEngine
    oc, od, ofb, weights, _ = oracle_mods
    sd = weights.conformer_state_dict(0, 4233)
    e = HipEngine(sd, vocab_size=4233)
    yield e, sd
    e.close()


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def valid_frames(a, lens, rate=4):
    """[B, T', ...] array / tensor with the PADDED encoder frames (rate * t >= feature length) set to zero -- the Squeezeformer engine
    does not compute the row blocks of padded frames (masr_debug_set key 38) and returns zeros there"""
    a = np.array(a.cpu().numpy() if torch.is_tensor(a) else a, copy=True)
    for b in range(a.shape[0]):
        a[b, min(a.shape[1], -(-int(lens[b]) // rate)):] = 0
    return a


def computing_padded_frames(e, **keys):
    """with computing_padded_frames(engine): the padded frames are computed like the reference computes them (key 38 = 0)"""
    return debug_keys(e, skip_padding=0, **keys)


def acceptable_texts(probs, vocab, od, margin=2e-3, limit=12):
    return od.acceptable_texts(probs, vocab, margin, limit)


# ---------------------------------------------------------------------------------------------------
# single kernels
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N,K,act', [(300, 256, 256, 0), (257, 768, 256, 0), (1000, 2048, 256, 2), (500, 256, 2048, 0),
                                       (130, 4233, 256, 0), (64, 256, 4864, 1), (7, 512, 64, 0), (8000, 256, 256, 2)])
def test_gemm_against_fp64(eng512, M, N, K, act):
    e, _ = eng512
    gen = torch.Generator().manual_seed(M * 7 + N)
    a = torch.randn(M, K, generator=gen)
    w = torch.randn(N, K, generator=gen) / np.sqrt(K)
    b = torch.randn(N, generator=gen)
    r = torch.randn(M, N, generator=gen)
    ref = a.double() @ w.double().T + b.double()
    if act == 1:
        ref = torch.relu(ref)
    elif act == 2:
        ref = ref * torch.sigmoid(ref)
    ref = r.double() + 0.5 * ref
    out = e.op_gemm(dev(a), dev(w), dev(b), dev(r), act=act, alpha=0.5).cpu().double()
    err = (out - ref).abs().max().item()
    assert err < 2e-5 * max(1.0, np.sqrt(K) / 16), f'gemm {M}x{N}x{K} act={act}: max err {err}'


def test_layernorm(eng512):
    e, _ = eng512
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(1003, 256, generator=gen) * 3 + 1
    w = torch.randn(256, generator=gen)
    b = torch.randn(256, generator=gen)
    ref = torch.nn.functional.layer_norm(x.double(), (256,), w.double(), b.double(), 1e-5)
    out = e.op_layernorm(dev(x), dev(w), dev(b)).cpu().double()
    assert (out - ref).abs().max() < 2e-5


# ---------------------------------------------------------------------------------------------------
# features
# ---------------------------------------------------------------------------------------------------
def test_fbank_testwav_against_reference_fixture(eng512, oracle_mods):
    e, _ = eng512
    oc, od, ofb, weights, _ = oracle_mods
    z = g('testwav.npz')
    pcm = dev(z['pcm'][None, :])
    n = dev(np.array([z['pcm'].shape[0]], np.int32))
    feats, frames, norm = e.fbank_batch(pcm, n, True, -20.0, return_norm=True)
    assert int(frames[0]) == 837 and feats.shape == (1, 837, 80)
    mine_i16 = norm[0].cpu().numpy()
    diff = (mine_i16.astype(np.int32) - z['norm_i16'].astype(np.int32))
    # The linear gain is float32(10 ** (gain_dB / 20)) with gain_dB from a float32 log10: numpy
    # evaluates both with machine-dependent SIMD/libm routines that are NOT correctly rounded (50 %
    # of float32 log10 results differ from the correctly rounded value on the build host), so the
    # reference itself is only reproducible to a few ulp of gain.  mean(x^2) is bit-exact (numpy's
    # buffered pairwise order is replicated), the transcendental steps are correctly rounded here.
    # => int16 samples may differ by 1 LSB where x*gain*32768 sits on an integer boundary.
    assert np.abs(diff).max() <= 1 and (diff != 0).mean() < 5e-3, f'int16: max {np.abs(diff).max()} frac {(diff != 0).mean()}'
    out = feats[0].cpu().numpy()
    # FFT / mel numerics in isolation: float64 oracle fbank of the SAME int16 samples
    f64 = ofb.kaldi_fbank(mine_i16, 80, np.float64)
    assert np.abs(out - f64).max() < 1e-3, np.abs(out - f64).max()
    budget.check('fbank test.wav, own samples', f64, ofb.kaldi_fbank(mine_i16, 80, np.float32), out)
    # against the reference fixture: frames whose 400 samples are identical must agree to 1e-3,
    # frames containing a +-1 LSB sample (near-silent frames amplify it) to 0.1
    bad = np.flatnonzero(diff)
    touched = np.zeros(837, bool)
    for i in bad:
        lo = max(0, (i - 400) // 160 + 1)
        touched[lo:min(837, i // 160 + 1)] = True
    err = np.abs(out - z['fbank']).max(axis=1)
    assert err[~touched].max() < 1e-3, err[~touched].max()
    assert err.max() < 0.1, err.max()


def test_fbank_ragged_batch(eng512, oracle_mods):
    e, _ = eng512
    oc, od, ofb, weights, _ = oracle_mods
    lens = [16000, 400, 399, 5000, 23456]
    n_max = max(lens)
    pcm = weights.synthetic_pcm(len(lens), n_max, seed=11)
    for i, l in enumerate(lens):
        pcm[i, l:] = 0
    feats, frames = e.fbank_batch(dev(pcm), dev(np.array(lens, np.int32)), True, -20.0)
    feats = feats.cpu().numpy()
    for i, l in enumerate(lens):
        T = ofb.num_frames(l)
        assert int(frames[i]) == T
        if T:
            ref, _ = ofb.featurize_pcm16(pcm[i, :l], dtype=np.float64)
            assert np.abs(feats[i, :T] - ref).max() < 1e-3, (i, np.abs(feats[i, :T] - ref).max())
        assert np.all(feats[i, T:] == 0.0)          # collate_fn zero padding
    # without dB normalisation
    feats2, _ = e.fbank_batch(dev(pcm[:1]), dev(np.array(lens[:1], np.int32)), False, -20.0)
    ref = ofb.kaldi_fbank(pcm[0, :lens[0]], 80, np.float64)
    assert np.abs(feats2[0].cpu().numpy()[:ref.shape[0]] - ref).max() < 1e-3
    budget.check('fbank synthetic_pcm 16000, no dB', ref, ofb.kaldi_fbank(pcm[0, :lens[0]], 80, np.float32), feats2[0].cpu().numpy()[:ref.shape[0]])


# ---------------------------------------------------------------------------------------------------
# encoder: golden fixtures of the real reference (B=3, ragged) + oracle
# ---------------------------------------------------------------------------------------------------
def test_encoder_full_against_reference_fixture(eng512, oracle_mods):
    e, sd = eng512
    oc, od, ofb, weights, golden_inputs = oracle_mods
    z = g('conformer_v512.npz')
    feats, lens = golden_inputs()
    enc = e.encode_full(dev(feats), dev(lens, torch.int32), -1)
    err = np.abs(enc.cpu().numpy() - z['enc']).max()
    assert err < 1e-3, f'encoder_out max err {err}'
    probs = e.ctc_probs(enc).cpu().numpy()
    perr = np.abs(probs - z['probs']).max()
    assert perr < 1e-3, f'probs max err {perr}'
    assert np.abs(probs.sum(-1) - 1).max() < 1e-4
    # pre-softmax logits (north_star: "logits within 1e-3")
    with torch.no_grad():
        ref_logits = oc.ctc_logits(sd, torch.from_numpy(z['enc']))
        my_logits = oc.ctc_logits(sd, enc.cpu())
    assert (ref_logits - my_logits).abs().max() < 1e-3


def test_encoder_chunk_mask_against_reference_fixture(eng512, oracle_mods):
    e, sd = eng512
    _, _, _, _, golden_inputs = oracle_mods
    z = g('conformer_v512.npz')
    feats, lens = golden_inputs()
    enc = e.encode_full(dev(feats), dev(lens, torch.int32), 16)
    err = np.abs(enc.cpu().numpy() - z['enc16']).max()
    assert err < 1e-3, f'chunk-16 encoder_out max err {err}'


def test_v4233_top4_against_reference_fixture(eng4233, oracle_mods):
    e, sd = eng4233
    _, _, _, _, golden_inputs = oracle_mods
    z = g('conformer_v4233.npz')
    feats, lens = golden_inputs()
    enc = e.encode_full(dev(feats), dev(lens, torch.int32), -1)
    probs, idx, mp = e.ctc_probs(enc, want_argmax=True)
    top = torch.topk(probs, 4, dim=-1)
    assert np.abs(top.values.cpu().numpy() - z['top_p']).max() < 1e-3
    margin = z['top_p'][..., 0] - z['top_p'][..., 1]
    safe = margin > 2e-3
    assert (idx.cpu().numpy().reshape(3, -1)[safe] == z['top_i'][..., 0][safe]).all()
    assert np.abs(mp.cpu().numpy().reshape(3, -1) - z['top_p'][..., 0]).max() < 1e-3
    idx2, mp2 = e.ctc_greedy_frames(enc)
    assert torch.equal(idx2.reshape(-1), idx) and torch.allclose(mp2.reshape(-1), mp, atol=1e-6)


def test_vocabulary_of_12000_against_oracle(oracle_mods):
    """V = 12 000 (beyond the 8 192 one 256-thread workgroup held in registers until round 6; limit now 16 384): softmax
    probabilities, fused greedy head (argmax / max probability without materialising the probabilities) and vocabulary pruning
    against the oracle's CTC head (loss/ctc.py:62-70) on the reference's golden inputs; V = 16 385 is refused with a message"""
    import ctypes as C
    from masr_amd.engine import HipEngine
    from masr_amd.decoders.beam_search_decoder import BeamSearchDecoder
    oc, weights, golden_inputs = oracle_mods[0], oracle_mods[3], oracle_mods[4]
    V = 12000
    sd = weights.conformer_state_dict(0, V)
    e = HipEngine(sd, vocab_size=V)
    try:
        feats, lens = golden_inputs()
        with torch.no_grad():
            ref_enc = oc.encoder_full(sd, torch.as_tensor(feats), torch.as_tensor(lens))
            ref = oc.ctc_probs(sd, ref_enc).numpy()
        enc = e.encode_full(dev(feats), dev(lens, torch.int32), -1)
        probs, idx, mp = e.ctc_probs(enc, want_argmax=True)
        got = probs.cpu().numpy()
        assert got.shape == ref.shape and np.abs(got - ref).max() < 1e-3
        srt = np.sort(ref, axis=-1)
        safe = (srt[..., -1] - srt[..., -2]) > 2e-3
        assert (idx.cpu().numpy().reshape(ref.shape[:2])[safe] == ref.argmax(-1)[safe]).all()
        assert np.abs(mp.cpu().numpy().reshape(ref.shape[:2]) - ref.max(-1)).max() < 1e-3
        idx2, mp2 = e.ctc_greedy_frames(enc)                       # fused head: the probabilities are never written
        assert torch.equal(idx2.reshape(-1), idx) and torch.allclose(mp2.reshape(-1), mp, atol=1e-6)
        # vocabulary pruning (cutoff_prob 0.99, top 40) of the same rows against numpy on the engine's own probabilities
        vocab = ['<blank>'] + [chr(0x4e00 + i) for i in range(V - 1)]
        dec = BeamSearchDecoder(0, 0, 20, 0.99, 40, vocab, language_model_path=None)
        ci, cl, cc, _, K = dec._candidates(probs[0])
        for t in range(0, got.shape[1], 7):
            order = np.argsort(-got[0, t], kind='stable')[:K]
            cum = np.cumsum(got[0, t][order])
            n = int(min(K, np.searchsorted(cum, 0.99) + 1))
            assert cc[t] == n and list(ci[t, :n]) == list(order[:n])
            assert np.abs(cl[t, :n] - np.log(got[0, t][order[:n]] + np.finfo(np.float32).tiny)).max() < 1e-5
    finally:
        e.close()
    big = HipEngine(weights.conformer_state_dict(0, 16385), vocab_size=16385)
    try:
        with pytest.raises(Exception, match='16384'):
            big.ctc_probs(big.encode_full(dev(feats), dev(lens, torch.int32), -1))
    finally:
        big.close()


def test_streaming_chunks_against_reference_fixture(eng512, oracle_mods):
    e, sd = eng512
    _, _, _, _, golden_inputs = oracle_mods
    z = g('conformer_v512.npz')
    feats, lens = golden_inputs()
    x = dev(feats[:1])
    sid = e.stream_open(400)
    for k, cur in enumerate(range(0, 331 - 67 + 1, 64)):
        probs, _, _ = e.encode_chunk([sid], x[:, cur:cur + 67].contiguous())
        err = np.abs(probs[0].cpu().numpy() - z['chunk_probs'][k]).max()
        assert err < 1e-3, f'chunk {k}: max err {err}'
    assert e.stream_offset(sid) == int(z['att_shape'][2])
    att, cnn = e.stream_export_cache(sid)
    assert list(att.shape) == list(z['att_shape'])
    assert np.abs(att[:, :, -16:].cpu().numpy() - z['att_tail']).max() < 1e-3
    assert np.abs(cnn.cpu().numpy() - z['cnn']).max() < 1e-3
    # reset -> identical first chunk again (reset_stream, inference_predictor.py:97-102)
    e.stream_reset(sid)
    probs, _, _ = e.encode_chunk([sid], x[:, 0:67].contiguous())
    assert np.abs(probs[0].cpu().numpy() - z['chunk_probs'][0]).max() < 1e-3
    e.stream_close(sid)


def test_streaming_multi_stream_lockstep(eng512, oracle_mods):
    """n streams batched per chunk step == each stream alone (streams are independent)."""
    e, sd = eng512
    gen = torch.Generator().manual_seed(9)
    feats = torch.randn(3, 195, 80, generator=gen) * 3 + 13
    x = dev(feats)
    sids = [e.stream_open(200) for _ in range(3)]
    solo = e.stream_open(200)
    outs = []
    for cur in range(0, 195 - 67 + 1, 64):
        p, _, _ = e.encode_chunk(sids, x[:, cur:cur + 67].contiguous())
        outs.append(p)
    for cur_i, cur in enumerate(range(0, 195 - 67 + 1, 64)):
        p, _, _ = e.encode_chunk([solo], x[1:2, cur:cur + 67].contiguous())
        assert (p[0] - outs[cur_i][1]).abs().max() < 1e-5
    for s in sids + [solo]:
        e.stream_close(s)


def test_streaming_many_streams_take_the_throughput_kernels(eng512, oracle_mods):
    """>= 256 lock-step streams (M >= 4096 rows per chunk step) run on the row-block / query-tiled kernels with the separate
    cache-append launch; up to that the latency-cut small-M kernels do the same work -- same results either way."""
    e, sd = eng512
    gen = torch.Generator().manual_seed(12)
    feats = torch.randn(2, 131, 80, generator=gen) * 3 + 13
    n = 260                                                   # 4160 rows = 130 row blocks: above both small-M thresholds
    x = dev(feats[torch.arange(n) % 2])                       # streams alternate between two inputs
    sids = [e.stream_open(40) for _ in range(n)]
    solo = [e.stream_open(40) for _ in range(2)]
    for cur in (0, 64):
        many, _, _ = e.encode_chunk(sids, x[:, cur:cur + 67].contiguous())
        few, _, _ = e.encode_chunk(solo, dev(feats[:, cur:cur + 67]))
        assert (many[0::2] - few[0]).abs().max() < 1e-5 and (many[1::2] - few[1]).abs().max() < 1e-5
    for s_ in sids + solo:
        e.stream_close(s_)


def test_short_last_chunk(eng512, oracle_mods):
    """is_end chunks are shorter than 67 frames (predict.py:296-305)."""
    e, sd = eng512
    oc, _, _, _, _ = oracle_mods
    gen = torch.Generator().manual_seed(4)
    feats = torch.randn(1, 67 + 64 + 23, 80, generator=gen) * 3 + 13
    sid = e.stream_open(100)
    att = torch.zeros(0, 0, 0, 0)
    cnn = torch.zeros(0, 0, 0, 0)
    off = 0
    for cur, end in ((0, 67), (64, 131), (128, 154)):
        ch = feats[:, cur:end]
        with torch.no_grad():
            ref, att, cnn = oc.get_encoder_out_chunk(sd, ch, off, -16, att, cnn)
        off += ref.shape[1]
        p, _, _ = e.encode_chunk([sid], dev(ch))
        assert p.shape == ref.shape
        assert (p.cpu() - ref).abs().max() < 1e-3
    e.stream_close(sid)


# ---------------------------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------------------------
def test_ctc_collapse_against_oracle(eng512, oracle_mods):
    e, _ = eng512
    _, od, _, _, _ = oracle_mods
    rng = np.random.default_rng(5)
    B, T, V = 7, 93, 12
    probs = rng.dirichlet(np.ones(V) * 0.2, size=(B, T)).astype(np.float32)
    probs[0, :, 0] = 1.0                      # an all-blank utterance -> score 0, empty text
    vocab = ['<blank>'] + [chr(97 + i) for i in range(V - 1)]
    idx, mp = e.argmax_rows(dev(probs.reshape(B * T, V)))
    assert np.array_equal(idx.cpu().numpy().reshape(B, T), probs.argmax(-1))
    assert np.array_equal(mp.cpu().numpy().reshape(B, T), probs.max(-1))
    nfr = np.array([T, T, 50, 1, 0, T, 77], np.int32)
    tok, ntok, score = e.ctc_collapse(idx.reshape(B, T), mp.reshape(B, T), dev(nfr))
    tok, ntok, score = tok.cpu().numpy(), ntok.cpu().numpy(), score.cpu().numpy()
    for b in range(B):
        s_ref, t_ref = od.greedy_decoder(probs[b, :nfr[b]], vocab) if nfr[b] else (0, '')
        text = ''.join(vocab[i] for i in tok[b, :ntok[b]])
        assert text == t_ref
        assert float(score[b]) * 100.0 == s_ref      # bit-identical sequential fp32 mean
        assert (tok[b, ntok[b]:] == -1).all()


# ---------------------------------------------------------------------------------------------------
# end to end + properties at BASELINE size
# ---------------------------------------------------------------------------------------------------
def test_transcribe_batch_against_oracle(eng4233, oracle_mods):
    """Ragged padded batch.  The oracle runs the SAME padded batch (collate_fn zero padding +
    get_encoder_out, trainer.py:632): the reference's pad mask keeps key j while 4*j < len, i.e.
    one more key than an utterance has when decoded alone, so batch != single by construction."""
    e, sd = eng4233
    oc, od, ofb, weights, _ = oracle_mods
    lens = [48000, 31000, 16000, 40123]
    n_max = max(lens)
    pcm = weights.synthetic_pcm(len(lens), n_max, seed=21)
    for i, l in enumerate(lens):
        pcm[i, l:] = 0
    tok, ntok, score = e.transcribe_batch(dev(pcm), dev(np.array(lens, np.int32)))
    tok, ntok, score = tok.cpu().numpy(), ntok.cpu().numpy(), score.cpu().numpy()
    vocab = weights.synthetic_vocab(4233)
    T = ofb.num_frames(n_max)
    feats = np.zeros((len(lens), T, 80), np.float32)
    frames = []
    for i, l in enumerate(lens):
        f, _ = ofb.featurize_pcm16(pcm[i, :l])
        feats[i, :f.shape[0]] = f
        frames.append(f.shape[0])
    with torch.no_grad():
        probs = oc.get_encoder_out(sd, torch.from_numpy(feats), torch.tensor(frames)).numpy()
    for i in range(len(lens)):
        n_enc = oc.subsampled_len(frames[i])
        s_ref, t_ref = od.greedy_decoder(probs[i, :n_enc], vocab)
        text = ''.join(vocab[j] for j in tok[i, :ntok[i]]).replace('<space>', ' ')
        ok, n_open = acceptable_texts(probs[i, :n_enc], vocab, od)   # decided frames exact; 0 undecided: == t_ref
        assert text in ok and (n_open or text == t_ref), (i, n_open, text, t_ref)
        assert abs(float(score[i]) * 100.0 - s_ref) < 0.1
    # decode_all_frames reproduces the reference batch quirk (trainer.py:340: padded frames decoded too)
    tok2, ntok2, _ = e.transcribe_batch(dev(pcm), dev(np.array(lens, np.int32)), decode_all_frames=True)
    for i in range(len(lens)):
        text = ''.join(vocab[j] for j in tok2[i, :int(ntok2[i])].cpu().numpy()).replace('<space>', ' ')
        assert text in acceptable_texts(probs[i], vocab, od)[0], (i, text)


def test_baseline_size_properties(eng4233, oracle_mods):
    """B=32 x 10 s (BASELINE config 2): finite, deterministic, batch-invariant."""
    e, sd = eng4233
    oc, od, ofb, weights, _ = oracle_mods
    pcm = dev(weights.synthetic_pcm(32, 160000, seed=1234))
    n = dev(np.full(32, 160000, np.int32))
    t1, n1, s1 = e.transcribe_batch(pcm, n)
    t2, n2, s2 = e.transcribe_batch(pcm, n)
    assert torch.equal(t1, t2) and torch.equal(n1, n2) and torch.equal(s1, s2)       # idempotent / deterministic
    assert torch.isfinite(s1).all() and (n1 >= 0).all() and (n1 <= 248).all()
    # an utterance decoded alone == the same utterance inside the batch (no cross-utterance math)
    ta, na, sa = e.transcribe_batch(pcm[5:6].contiguous(), n[5:6].contiguous())
    assert int(na[0]) == int(n1[5]) and torch.equal(ta[0, :int(na[0])], t1[5, :int(na[0])])
    assert abs(float(sa[0]) - float(s1[5])) < 1e-5
    # oracle on one utterance of the batch
    feat, _ = ofb.featurize_pcm16(pcm[5].cpu().numpy())
    with torch.no_grad():
        probs = oc.get_encoder_out(sd, torch.from_numpy(feat)[None], torch.tensor([feat.shape[0]]))[0].numpy()
    s_ref, t_ref = od.greedy_decoder(probs, weights.synthetic_vocab(4233))
    vocab = weights.synthetic_vocab(4233)
    text = ''.join(vocab[j] for j in t1[5, :int(n1[5])].cpu().numpy()).replace('<space>', ' ')
    assert text in acceptable_texts(probs, vocab, od)[0] and abs(float(s1[5]) * 100 - s_ref) < 0.1


def test_contract_route_is_bit_exact_at_baseline_size(eng4233, oracle_mods):
    """BASELINE configs[1] on the route bench.py times (masr_transcribe_rows, use_db_normalization = 2): with the gains of
    ``reference_gains`` (the reference's scalar numpy expressions on the device's numpy-ordered mean squares) the int16
    samples the fbank kernel consumes are the reference's for ALL 32 utterances, bit for bit (audio.py:287-304,549-574), and
    every transcript is the reference's wherever its frames are numerically decided (no CER allowance)."""
    from masr_amd import parallel
    e, sd = eng4233
    oc, od, ofb, weights, _ = oracle_mods
    B, N = 32, 160000
    pcm = weights.synthetic_pcm(B, N, seed=1234)
    xs, ns = dev(pcm), dev(np.full(B, N, np.int32))
    gains = e.host_gains(xs, ns, -20.0)
    # step by step against the reference's expressions on this host (audio.py:519-529,287-304): the device's mean squares ARE
    # numpy's, the batch gains ARE the scalar expressions' -- then the int16 samples must be
    ms_dev = e.mean_square(xs, ns).cpu().numpy()
    fl = [ofb.pcm16_to_float32(pcm[i]) for i in range(B)]
    ms_np = np.array([np.mean(f ** 2) for f in fl], np.float32)
    assert np.array_equal(ms_dev, ms_np), f'mean squares differ for utterances {np.nonzero(ms_dev != ms_np)[0].tolist()}'
    g_np = np.array([10. ** (min(300.0, -20 - ofb.rms_db(f)) / 20.) for f in fl], np.float32)
    g_dev = gains.cpu().numpy()
    assert np.array_equal(g_dev, g_np), f'gains differ for utterances {np.nonzero(g_dev != g_np)[0].tolist()}: {g_dev[g_dev != g_np]} vs {g_np[g_dev != g_np]}'
    _, _, norm = e.fbank_batch(xs, ns, True, -20.0, return_norm=True, gain_in=gains)
    norm = norm.cpu().numpy()
    feats = []
    for i in range(B):
        f, i16 = ofb.featurize_pcm16(pcm[i])
        assert np.array_equal(norm[i], i16), f'utterance {i}: {int((norm[i] != i16).sum())} int16 samples differ'
        feats.append(f)
    rows = e.transcribe_rows(xs, ns, True, -20.0, gain_in=gains)
    tok, nt, score = parallel.unpack_hypothesis_rows(rows.cpu().numpy())
    with torch.no_grad():
        probs = oc.get_encoder_out(sd, torch.from_numpy(np.stack(feats)), torch.full((B,), feats[0].shape[0])).numpy()
    vocab = weights.synthetic_vocab(4233)
    n_exact = 0
    for i in range(B):
        s_ref, t_ref = od.greedy_decoder(probs[i], vocab)
        text = ''.join(vocab[j] for j in tok[i, :nt[i]]).replace('<space>', ' ')
        ok, n_open = acceptable_texts(probs[i], vocab, od)
        assert text in ok and (n_open or text == t_ref), (i, n_open, text, t_ref)
        n_exact += n_open == 0
        assert abs(float(score[i]) * 100.0 - s_ref) < 0.1
    print(f'{n_exact} of {B} utterances fully decided: transcripts identical; the rest identical on every decided frame')
    assert n_exact >= B // 2


# ---------------------------------------------------------------------------------------------------
# Squeezeformer (configs/squeezeformer.yml, streaming: False)
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sq512(oracle_mods):
    from masr_amd.engine import HipEngine
    _, _, _, weights, _ = oracle_mods
    sd = weights.squeezeformer_state_dict(0, 512)
    e = HipEngine(sd, vocab_size=512, streaming=False, use_model='squeezeformer',
                  encoder_conf={'encoder_dim': 256, 'attention_heads': 4, 'num_blocks': 12, 'reduce_idx': 5,
                                'recover_idx': 11, 'feed_forward_expansion_factor': 8, 'cnn_module_kernel': 31})
    yield e, sd
    e.close()


def test_squeezeformer_against_reference_fixture(sq512, oracle_mods):
    e, sd = sq512
    _, _, _, _, golden_inputs = oracle_mods
    z = g('squeezeformer_v512.npz')
    feats, lens = golden_inputs()
    # default: the row blocks of padded frames are not computed (masr_debug_set key 38) -- the VALID frames must match the reference;
    # key 38 = 0 computes the padded frames as the reference does: then every row must
    enc = e.encode_full(dev(feats), dev(lens, torch.int32), -1)
    got = enc.cpu().numpy()
    for b in range(got.shape[0]):
        v = min(got.shape[1], -(-int(lens[b]) // 4))
        err = np.abs(got[b, :v] - z['enc'][b, :v]).max()
        assert err < 1e-3, f'squeezeformer encoder_out max err {err} on the valid frames of utterance {b}'
    with computing_padded_frames(e):
        full = e.encode_full(dev(feats), dev(lens, torch.int32), -1)
    err = np.abs(full.cpu().numpy() - z['enc']).max()
    assert err < 1e-3, f'squeezeformer encoder_out max err {err}'
    for b in range(got.shape[0]):       # skipping changes nothing on a valid frame: identical bits
        v = min(got.shape[1], -(-int(lens[b]) // 4))
        assert np.array_equal(got[b, :v], full.cpu().numpy()[b, :v])
    enc = full
    probs = e.ctc_probs(enc).cpu().numpy()
    assert np.abs(probs - z['probs']).max() < 1e-3
    idx, mp = e.ctc_greedy_frames(enc)
    margin = np.sort(z['probs'], axis=-1)
    safe = (margin[..., -1] - margin[..., -2]) > 2e-3
    assert (idx.cpu().numpy()[safe] == z['probs'].argmax(-1)[safe]).all()


def test_conformer_nonstreaming_build_against_reference_fixture(oracle_mods):
    """conformer.yml with streaming: False: symmetric conv module (zero rows on both sides of the GLU output)"""
    from masr_amd.engine import HipEngine
    weights, golden_inputs = oracle_mods[3], oracle_mods[4]
    sd = weights.conformer_state_dict(0, 512)
    e = HipEngine(sd, vocab_size=512, streaming=False)
    z = g('conformer_nonstreaming_v512.npz')
    feats, lens = golden_inputs()
    enc = e.encode_full(dev(feats), dev(lens, torch.int32))
    assert np.abs(enc.cpu().numpy() - z['enc']).max() < 1e-3
    assert np.abs(e.ctc_probs(enc).cpu().numpy() - z['probs']).max() < 1e-3
    # chunk masks do not exist in this build; chunked streaming is refused
    enc16 = e.encode_full(dev(feats), dev(lens, torch.int32), decoding_chunk_size=16)
    assert torch.equal(enc16, enc)
    with pytest.raises(Exception):
        e.stream_open(0)
    e.close()


@pytest.mark.parametrize('streaming', [False, True])
def test_conformer_batch_norm_conv_module_against_oracle(oracle_mods, streaming):
    """conformer.yml with encoder_conf.cnn_module_norm: batch_norm (conformer/convolution.py:60-67): eval-mode BatchNorm folded
    into the depthwise kernel's scale / shift variant; full-context forward of both builds against the oracle (which
    tests/test_oracle_golden.py pins to the live reference model with that option), one long and one ragged batch; chunked
    streaming is refused with a message; a checkpoint / config mismatch is refused at construction"""
    from masr_amd.engine import HipEngine
    oc, weights, golden_inputs = oracle_mods[0], oracle_mods[3], oracle_mods[4]
    sd = weights.conformer_state_dict(0, 512, cnn_module_norm='batch_norm')
    e = HipEngine(sd, vocab_size=512, streaming=streaming, encoder_conf={'cnn_module_norm': 'batch_norm'})
    try:
        feats, lens = golden_inputs()
        with torch.no_grad():
            ref = oc.encoder_full(sd, torch.as_tensor(feats), torch.as_tensor(lens), streaming=streaming)
            ref_p = oc.ctc_probs(sd, ref).numpy()
        enc = e.encode_full(dev(feats), dev(lens, torch.int32), -1)
        assert np.abs(enc.cpu().numpy() - ref.numpy()).max() < 1e-3
        assert np.abs(e.ctc_probs(enc).cpu().numpy() - ref_p).max() < 1e-3
        g = torch.Generator().manual_seed(3)                 # 32 x <= 10 s: the row-block kernels' regime
        x = torch.randn(32, 998, 80, generator=g) * 3 + 13
        l2 = torch.randint(300, 999, (32,), generator=g)
        l2[0] = 998
        x = x * (torch.arange(998)[None, :, None] < l2[:, None, None])
        with torch.no_grad():
            ref2 = oc.encoder_full(sd, x[:3], l2[:3], streaming=streaming).numpy()
        got2 = e.encode_full(dev(x), dev(l2, torch.int32), -1).cpu().numpy()
        for b in range(3):                                   # (the oracle runs three utterances as their own padded batch)
            v = int(e.enc_frames(l2[b:b + 1])[0])
            assert np.abs(got2[b, :v] - ref2[b, :v]).max() < 1e-3
        if streaming:
            with pytest.raises(Exception, match='batch_norm'):
                e.stream_open(0)
    finally:
        e.close()
    with pytest.raises(Exception, match='cnn_module_norm'):   # LayerNorm config on a BatchNorm checkpoint
        HipEngine(sd, vocab_size=512, streaming=streaming)
    with pytest.raises(Exception, match='cnn_module_norm'):
        HipEngine(weights.conformer_state_dict(0, 512), vocab_size=512, encoder_conf={'cnn_module_norm': 'batch_norm'})


def test_squeezeformer_streaming_build_against_reference_fixture(oracle_mods):
    """squeezeformer.yml as shipped (streaming: True): causal conv module (history rows = glu(bias)) + stream time reduction"""
    from masr_amd.engine import HipEngine
    from oracle import squeezeformer as osq
    weights, golden_inputs = oracle_mods[3], oracle_mods[4]
    sd = weights.squeezeformer_state_dict(0, 512, streaming=True)
    enc_conf = {'encoder_dim': 256, 'attention_heads': 4, 'num_blocks': 12, 'reduce_idx': 5, 'recover_idx': 11,
                'feed_forward_expansion_factor': 8, 'cnn_module_kernel': 31}
    e = HipEngine(sd, encoder_conf=enc_conf, vocab_size=512, streaming=True, use_model='squeezeformer')
    z = g('squeezeformer_streaming_v512.npz')
    feats, lens = golden_inputs()
    enc = e.encode_full(dev(feats), dev(lens, torch.int32))
    assert np.abs(valid_frames(enc, lens) - valid_frames(z['enc'], lens)).max() < 1e-3
    with computing_padded_frames(e):
        enc = e.encode_full(dev(feats), dev(lens, torch.int32))
        assert np.abs(enc.cpu().numpy() - z['enc']).max() < 1e-3
        probs = e.ctc_probs(enc).cpu().numpy()
        assert np.abs(probs - z['probs']).max() < 1e-3
    # odd frame counts (time reduction / recovery edge) against the oracle
    torch.manual_seed(4)
    x = torch.randn(2, 203, 80) * 3 + 13
    l2 = torch.tensor([203, 150])
    x = x * (torch.arange(203)[None, :, None] < l2[:, None, None])
    with torch.no_grad():
        ref = osq.encoder_full(sd, x, l2, causal=True).numpy()
    got = e.encode_full(dev(x), dev(l2, torch.int32)).cpu().numpy()
    assert np.abs(valid_frames(got, l2) - valid_frames(ref, l2)).max() < 1e-3
    with computing_padded_frames(e):
        got = e.encode_full(dev(x), dev(l2, torch.int32)).cpu().numpy()
    assert np.abs(got - ref).max() < 1e-3
    e.close()


@pytest.mark.parametrize('streaming', [False, True])
def test_squeezeformer_fused_layer_is_bit_identical_to_the_separate_launches(oracle_mods, streaming):
    """sqz_layer.hip (attention + two fused stage kernels per layer, the next layer's QKV projection riding on the last one)
    against the twelve launches it replaces (masr_debug_set key 36 = 0): the same operations in the same order, so the encoder
    output must be IDENTICAL -- ragged batch of 26 x <= 20 s (405 row blocks at the full rate, 203 behind the time reduction:
    both resolutions take the fused path), symmetric and causal conv builds; and within 1e-3 of the oracle on two utterances."""
    from masr_amd.engine import HipEngine
    from oracle import squeezeformer as osq
    weights = oracle_mods[3]
    sd = weights.squeezeformer_state_dict(0, 512, streaming=streaming)
    enc_conf = {'encoder_dim': 256, 'attention_heads': 4, 'num_blocks': 12, 'reduce_idx': 5, 'recover_idx': 11,
                'feed_forward_expansion_factor': 8, 'cnn_module_kernel': 31}
    e = HipEngine(sd, encoder_conf=enc_conf, vocab_size=512, streaming=streaming, use_model='squeezeformer')
    try:
        gen = torch.Generator().manual_seed(77)
        B, T = 26, 1998
        lens = torch.randint(300, T + 1, (B,), generator=gen)
        lens[0], lens[1] = T, 1001                                   # a full-length and an odd-length utterance
        x = torch.randn(B, T, 80, generator=gen) * 3 + 13
        x = x * (torch.arange(T)[None, :, None] < lens[:, None, None])
        xd, ld = dev(x), dev(lens, torch.int32)
        skipping = e.encode_full(xd, ld).cpu()                      # default: row blocks of padded frames are not computed
        with computing_padded_frames(e):
            fused = e.encode_full(xd, ld).cpu()
        with computing_padded_frames(e, sqz_fused_blocks=0):
            plain = e.encode_full(xd, ld).cpu()
        assert torch.isfinite(fused).all() and torch.isfinite(skipping).all()
        assert torch.equal(fused, plain), f'max |fused - separate| = {(fused - plain).abs().max().item():.3e}'
        # skipping the padded row blocks changes no bit of a valid frame, and the padded frames of the output read zero
        assert np.array_equal(skipping.numpy(), valid_frames(fused, lens))
        with torch.no_grad():
            ref = osq.encoder_full(sd, x[:2], lens[:2], causal=streaming)
        n0, n1 = int(e.enc_frames(lens[:1])[0]), int(e.enc_frames(lens[1:2])[0])
        # (the oracle runs the two utterances as their own padded batch: the same rows up to each one's valid frames)
        err = max((fused[0, :n0] - ref[0, :n0]).abs().max().item(), (fused[1, :n1] - ref[1, :n1]).abs().max().item())
        assert err < 1e-3, err
    finally:
        e.close()


def test_squeezeformer_stream_chunks_against_reference_fixture(oracle_mods):
    """Squeezeformer forward_chunk (streaming build): half-rate layers keep their own caches, stream time reduction"""
    from masr_amd.engine import HipEngine
    from oracle import squeezeformer as osq
    weights, golden_inputs = oracle_mods[3], oracle_mods[4]
    sd = weights.squeezeformer_state_dict(0, 512, streaming=True)
    enc_conf = {'encoder_dim': 256, 'attention_heads': 4, 'num_blocks': 12, 'reduce_idx': 5, 'recover_idx': 11,
                'feed_forward_expansion_factor': 8, 'cnn_module_kernel': 31}
    e = HipEngine(sd, encoder_conf=enc_conf, vocab_size=512, streaming=True, use_model='squeezeformer')
    z = g('squeezeformer_streaming_v512.npz')
    feats, _ = golden_inputs()
    sid = e.stream_open(0)
    outs = []
    for cur, n in [(c, 67) for c in range(0, 331 - 67 + 1, 64)] + [(320, 11)]:
        p, _, _ = e.encode_chunk([sid], dev(feats[:1, cur:cur + n]))
        outs.append(p[0].cpu().numpy())
    got = np.concatenate(outs)
    assert got.shape == z['chunk_probs'].shape == (82, 512)
    assert np.abs(got - z['chunk_probs']).max() < 1e-3
    att, cnn = e.stream_export_cache(sid)
    lay = z['att_layers']                      # the fixture keeps the caches of four representative layers
    assert att.shape == (12, 4, 82, 128) and np.abs(att.cpu().numpy()[lay] - z['att']).max() < 1e-3
    assert np.abs(cnn.cpu().numpy()[lay] - z['cnn']).max() < 1e-3
    # two streams in lock-step (different audio) == the oracle run stream by stream
    torch.manual_seed(5)
    xa, xb = torch.randn(1, 131, 80) * 3 + 13, torch.randn(1, 131, 80) * 3 + 13
    s0, s1 = e.stream_open(0), e.stream_open(0)
    ca = cb = (torch.zeros(0, 0, 0, 0), torch.zeros(0, 0, 0, 0))
    oa = ob = 0
    for cur in (0, 64):
        both = torch.cat([xa[:, cur:cur + 67], xb[:, cur:cur + 67]])
        p, _, _ = e.encode_chunk([s0, s1], dev(both))
        with torch.no_grad():
            pa, *ca = osq.get_encoder_out_chunk(sd, xa[:, cur:cur + 67], oa, -16, *ca)
            pb, *cb = osq.get_encoder_out_chunk(sd, xb[:, cur:cur + 67], ob, -16, *cb)
        oa += pa.shape[1]
        ob += pb.shape[1]
        assert np.abs(p[0].cpu().numpy() - pa[0].numpy()).max() < 1e-3
        assert np.abs(p[1].cpu().numpy() - pb[0].numpy()).max() < 1e-3
    e.close()


def test_squeezeformer_odd_lengths_against_oracle(sq512, oracle_mods):
    """odd T' (time reduction trims, recovery slices) and a ragged batch."""
    from oracle import squeezeformer as osq
    e, sd = sq512
    gen = torch.Generator().manual_seed(12)
    feats = torch.randn(2, 203, 80, generator=gen) * 3 + 13        # T' = 49 (odd)
    lens = torch.tensor([203, 120])
    feats = feats * (torch.arange(203)[None, :, None] < lens[:, None, None])
    with torch.no_grad():
        ref = osq.encoder_full(sd, feats, lens)
    enc = e.encode_full(dev(feats), dev(lens, torch.int32), -1).cpu()
    assert ref.shape == enc.shape and np.abs(valid_frames(ref, lens) - valid_frames(enc, lens)).max() < 1e-3
    with computing_padded_frames(e):
        enc = e.encode_full(dev(feats), dev(lens, torch.int32), -1).cpu()
    assert (ref - enc).abs().max() < 1e-3


# ---------------------------------------------------------------------------------------------------
# Efficient Conformer (configs/efficient_conformer.yml), full-context get_encoder_out
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def eff512(oracle_mods):
    from masr_amd.engine import HipEngine
    _, _, _, weights, _ = oracle_mods
    sd = weights.efficient_conformer_state_dict(0, 512)
    e = HipEngine(sd, vocab_size=512, streaming=True, use_model='efficient_conformer',
                  encoder_conf={'output_size': 256, 'attention_heads': 4, 'linear_units': 2048, 'num_blocks': 12,
                                'cnn_module_kernel': 15,
                                'efficient_conf': {'stride_layer_idx': [3], 'stride': [2], 'group_layer_idx': [0, 1, 2, 3],
                                                   'group_size': 3, 'stride_kernel': True}})
    yield e, sd
    e.close()


def test_efficient_conformer_against_reference_fixture(eff512, oracle_mods):
    e, sd = eff512
    _, _, _, _, golden_inputs = oracle_mods
    z = g('efficient_conformer_v512.npz')
    feats, lens = golden_inputs()
    enc = e.encode_full(dev(feats), dev(lens, torch.int32), -1)
    assert tuple(enc.shape) == z['enc'].shape
    err = np.abs(enc.cpu().numpy() - z['enc']).max()
    assert err < 1e-3, f'efficient conformer encoder_out max err {err}'
    probs = e.ctc_probs(enc).cpu().numpy()
    assert np.abs(probs - z['probs']).max() < 1e-3


def test_efficient_conformer_stream_chunks_against_reference_fixture(eff512, oracle_mods):
    """EfficientConformerEncoder.forward_chunk: grouped attention over cache + chunk, stride layer with cnn cache, half-rate
    layers with their own caches; probabilities and the exported caches against the reference run"""
    from oracle import efficient_conformer as oe
    e, sd = eff512
    z = g('efficient_conformer_v512.npz')
    feats, _ = oracle_mods[4]()
    sid = e.stream_open(0)
    outs = []
    for cur, n in [(c, 67) for c in range(0, 331 - 67 + 1, 64)] + [(320, 11)]:
        p, _, _ = e.encode_chunk([sid], dev(feats[:1, cur:cur + n]))
        outs.append(p[0].cpu().numpy())
    got = np.concatenate(outs)
    assert got.shape == z['chunk_probs'].shape == (41, 512)
    assert np.abs(got - z['chunk_probs']).max() < 1e-3
    att, cnn = e.stream_export_cache(sid)
    lay = z['att_layers']                      # the fixture keeps the caches of four representative layers
    assert att.shape == (12, 4, 82, 128) and np.abs(att.cpu().numpy()[lay] - z['att']).max() < 1e-3
    assert cnn.shape == (12, 1, 256, 14) and np.abs(cnn.cpu().numpy()[lay] - z['cnn']).max() < 1e-3
    e.stream_close(sid)
    # two streams with different histories in one lock-step call (one joins a chunk later) == the oracle stream by stream
    torch.manual_seed(6)
    xa, xb = torch.randn(1, 195, 80) * 3 + 13, torch.randn(1, 131, 80) * 3 + 13
    s0, s1 = e.stream_open(0), e.stream_open(0)
    ca = cb = (torch.zeros(0, 0, 0, 0), torch.zeros(0, 0, 0, 0))
    with torch.no_grad():
        pa, *ca = oe.get_encoder_out_chunk(sd, xa[:, :67], 0, -16, *ca)
    p, _, _ = e.encode_chunk([s0], dev(xa[:, :67]))
    assert np.abs(p[0].cpu().numpy() - pa[0].numpy()).max() < 1e-3
    oa, ob = pa.shape[1], 0
    for k, cur in enumerate((64, 128)):
        both = torch.cat([xa[:, cur:cur + 67], xb[:, cur - 64:cur - 64 + 67]])
        p, _, _ = e.encode_chunk([s0, s1], dev(both))
        with torch.no_grad():
            pa, *ca = oe.get_encoder_out_chunk(sd, xa[:, cur:cur + 67], oa, -16, *ca)
            pb, *cb = oe.get_encoder_out_chunk(sd, xb[:, cur - 64:cur - 64 + 67], ob, -16, *cb)
        oa += pa.shape[1]
        ob += pb.shape[1]
        assert np.abs(p[0].cpu().numpy() - pa[0].numpy()).max() < 1e-3
        assert np.abs(p[1].cpu().numpy() - pb[0].numpy()).max() < 1e-3
    e.stream_close(s0)
    e.stream_close(s1)


@pytest.mark.parametrize('T', [203, 204, 205, 331])
def test_efficient_conformer_lengths_against_oracle(eff512, oracle_mods, T):
    """T' mod 3 = 0/1/2 (grouping pad) and odd / even T' (stride layer, AvgPool ceil mode), ragged batch."""
    from oracle import efficient_conformer as oe
    e, sd = eff512
    gen = torch.Generator().manual_seed(T)
    feats = torch.randn(2, T, 80, generator=gen) * 3 + 13
    lens = torch.tensor([T, T // 2 + 9])
    feats = feats * (torch.arange(T)[None, :, None] < lens[:, None, None])
    with torch.no_grad():
        ref = oe.encoder_full(sd, feats, lens)
    enc = e.encode_full(dev(feats), dev(lens, torch.int32), -1).cpu()
    assert ref.shape == enc.shape and (ref - enc).abs().max() < 1e-3


# ---------------------------------------------------------------------------------------------------
# DeepSpeech2 (configs/deepspeech2.yml: conv front-end + 5 x LSTM-1024 + LayerNorm, CTC head)
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ds2_engines(oracle_mods):
    from masr_amd.engine import HipEngine
    weights = oracle_mods[3]
    enc_conf = {'num_rnn_layers': 5, 'rnn_size': 1024}
    sd_bi = weights.deepspeech2_state_dict(0, 300, bidirectional=True)
    sd_uni = weights.deepspeech2_state_dict(0, 300, bidirectional=False)
    e_bi = HipEngine(sd_bi, encoder_conf=enc_conf, streaming=False, use_model='deepspeech2')
    e_uni = HipEngine(sd_uni, encoder_conf=enc_conf, streaming=True, use_model='deepspeech2')
    yield e_bi, e_uni, sd_bi, sd_uni
    e_bi.close()
    e_uni.close()


def test_deepspeech2_against_reference_fixture(ds2_engines, oracle_mods):
    e_bi, e_uni, _, _ = ds2_engines
    z = g('deepspeech2_v300.npz')
    feats, lens = oracle_mods[4]()
    for e, key in ((e_bi, 'bi_probs'), (e_uni, 'uni_probs')):
        enc = e.encode_full(dev(feats), dev(lens, torch.int32))
        probs = e.ctc_probs(enc).cpu().numpy()
        ref = z[key]                                   # [3, 82, 300]; padded rows of the shorter utterances included
        assert probs.shape == ref.shape
        assert np.abs(probs - ref).max() < 1e-3
        valid = [82, 49, 23]
        for b in range(3):
            assert (probs[b, :valid[b]].argmax(-1) == ref[b, :valid[b]].argmax(-1)).mean() > 0.995
        idx, mp = e.ctc_greedy_frames(enc)
        assert np.array_equal(idx.cpu().numpy(), probs.argmax(-1))
        np.testing.assert_allclose(mp.cpu().numpy(), probs.max(-1), atol=1e-6)


def test_deepspeech2_stream_chunks_against_reference_fixture(ds2_engines, oracle_mods):
    _, e, _, _ = ds2_engines
    z = g('deepspeech2_v300.npz')
    feats, _ = oracle_mods[4]()
    sid = e.stream_open(0)
    for i, cur in enumerate(range(0, 331 - 67 + 1, 64)):
        probs, _, _ = e.encode_chunk([sid], dev(feats[:1, cur:cur + 67]))
        assert np.abs(probs[0].cpu().numpy() - z['chunk_probs'][i]).max() < 1e-3
    h, c = e.stream_export_cache(sid)
    assert np.abs(h.cpu().numpy() - z['h']).max() < 1e-3
    assert np.abs(c.cpu().numpy() - z['c']).max() < 1e-3
    # reset -> the first chunk repeats bit-for-bit
    e.stream_reset(sid)
    p0, _, _ = e.encode_chunk([sid], dev(feats[:1, :67]))
    assert np.abs(p0[0].cpu().numpy() - z['chunk_probs'][0]).max() < 1e-3
    e.stream_close(sid)


def test_deepspeech2_two_streams_against_oracle(ds2_engines, oracle_mods):
    # two interleaved streams with different audio == each one alone (state isolation), and == the oracle
    from oracle import deepspeech2 as ods
    _, e, _, sd = ds2_engines
    torch.manual_seed(11)
    xa = torch.randn(1, 131, 80) * 3 + 13
    xb = torch.randn(1, 131, 80) * 3 + 13
    s0, s1 = e.stream_open(0), e.stream_open(0)
    ha = ca = hb = cb = None
    for cur in (0, 64):
        both = torch.cat([xa[:, cur:cur + 67], xb[:, cur:cur + 67]])
        probs, _, _ = e.encode_chunk([s0, s1], dev(both))
        with torch.no_grad():
            pa, _, ha, ca = ods.get_encoder_out_chunk(sd, xa[:, cur:cur + 67], torch.tensor([67]), ha, ca)
            pb, _, hb, cb = ods.get_encoder_out_chunk(sd, xb[:, cur:cur + 67], torch.tensor([67]), hb, cb)
        assert np.abs(probs[0].cpu().numpy() - pa[0].numpy()).max() < 1e-3
        assert np.abs(probs[1].cpu().numpy() - pb[0].numpy()).max() < 1e-3
    e.stream_close(s0)
    e.stream_close(s1)


def test_deepspeech2_transcribe_batch_against_oracle(ds2_engines, oracle_mods):
    from oracle import deepspeech2 as ods
    oc, od, ofb, weights, _ = oracle_mods
    e, _, sd, _ = ds2_engines
    n = [32000, 21000, 9000]
    pcm = np.zeros((3, max(n)), np.int16)
    for b in range(3):
        pcm[b, :n[b]] = weights.synthetic_pcm(1, n[b], seed=20 + b)[0]
    tok, ntok, score = e.transcribe_batch(dev(pcm), dev(np.array(n, np.int32)))
    feats, frames = e.fbank_batch(dev(pcm), dev(np.array(n, np.int32)))
    with torch.no_grad():
        probs = ods.get_encoder_out(sd, feats.cpu(), frames.cpu().long()).numpy()
    xl = ((frames.cpu().numpy() - 1) // 2 - 1) // 2
    vocab = weights.synthetic_vocab(300)
    for b in range(3):
        s_ref, t_ref = od.greedy_decoder(probs[b, :xl[b]], vocab)
        ids = tok[b, :int(ntok[b])].cpu().numpy()
        assert ''.join(vocab[i] for i in ids).replace('<space>', ' ') == t_ref


# ---------------------------------------------------------------------------------------------------
# engine reuse: grow-only workspaces, stream slots, mixed call sequences
# ---------------------------------------------------------------------------------------------------
def test_engine_reuse_across_shapes_and_streams(eng512, oracle_mods):
    """one engine, changing batch sizes / lengths / stream counts: results do not depend on the call history"""
    e, _ = eng512
    torch.manual_seed(21)
    x_small = torch.randn(1, 131, 80) * 3 + 13
    l_small = torch.tensor([131], dtype=torch.int32)
    ref = e.encode_full(dev(x_small), dev(l_small)).cpu()
    for B, T in ((5, 400), (2, 67), (9, 203), (1, 998)):
        x = torch.randn(B, T, 80) * 3 + 13
        lens = torch.randint(T // 2, T + 1, (B,), dtype=torch.int32)
        lens[0] = T
        enc = e.encode_full(dev(x), dev(lens))
        assert torch.isfinite(enc).all()
    again = e.encode_full(dev(x_small), dev(l_small)).cpu()
    assert torch.equal(ref, again)
    # streams: open / close many times, ids are recycled, a fresh stream behaves like the first one
    chunk = dev(x_small[:, :67])
    sid = e.stream_open(0)
    first, _, _ = e.encode_chunk([sid], chunk)
    first = first.cpu()
    e.stream_close(sid)
    seen = set()
    for _ in range(6):
        ids = [e.stream_open(64) for _ in range(5)]
        seen.update(ids)
        p, _, _ = e.encode_chunk(ids, chunk.repeat(5, 1, 1))
        for k in range(5):
            # (the d_ff / K splits depend on the number of rows: same values up to the summation order)
            assert (p[k].cpu() - first[0]).abs().max() < 1e-5
        for i in ids:
            e.stream_close(i)
    assert len(seen) <= 5                      # slots are reused
    with pytest.raises(Exception):
        e.encode_chunk([sid + 100], chunk)      # unknown stream id fails loudly


@pytest.mark.parametrize('B', [7, 20])
def test_deepspeech2_batched_recurrence_against_oracle(ds2_engines, oracle_mods, B):
    """batches above 4 sequences run the recurrence on the matrix cores (lstm_step_mfma_kernel): ragged batch vs the oracle"""
    from oracle import deepspeech2 as ods
    e_bi, e_uni, sd_bi, sd_uni = ds2_engines
    torch.manual_seed(B)
    T = 131
    lens = torch.randint(40, T + 1, (B,))
    lens[0] = T
    x = (torch.randn(B, T, 80) * 3 + 13) * (torch.arange(T)[None, :, None] < lens[:, None, None])
    for e, sd in ((e_bi, sd_bi), (e_uni, sd_uni)):
        enc = e.encode_full(dev(x), dev(lens, torch.int32))
        probs = e.ctc_probs(enc).cpu().numpy()
        with torch.no_grad():
            ref = ods.get_encoder_out(sd, x, lens).numpy()
        assert probs.shape == ref.shape and np.abs(probs - ref).max() < 1e-3


# ---------------------------------------------------------------------------------------------------
# feature_method linear / mfcc: masr_linear_batch / masr_mfcc_batch and the encoder with input size 161 / 40
# ---------------------------------------------------------------------------------------------------
def test_linear_spectrogram_against_reference_fixture(eng512, oracle_mods):
    e, _ = eng512
    oc, od, ofb, weights, _ = oracle_mods
    z = g('features.npz')
    pcm = z['pcm']
    # int16 PCM in, dB normalisation on (the reference featurizer's path, audio_featurizer.py:36-53)
    feats, frames = e.linear_batch(dev(pcm[None, :]), dev(np.array([len(pcm)], np.int32)), True, -20.0)
    assert int(frames[0]) == 199 and feats.shape == (1, 199, 161)
    # the gain is only reproducible to a few ulp of float32 (see test_fbank_testwav_...): a 1-ulp change of the samples moves
    # the weakest bins of a frame (80 dB below its peak) by up to ~1e-3 in the log domain, the typical bin by ~1e-6
    err = np.abs(feats[0].cpu().numpy() - z['linear'])
    assert err.max() < 3e-3 and err.mean() < 1e-5, (err.max(), err.mean())
    # ragged float32 batch without normalisation: exact same samples -> float64 DFT vs numpy's FFT
    lens = [16000, 320, 319, 5000, 12345]
    x = (weights.synthetic_pcm(len(lens), max(lens), seed=5).astype(np.float32) / 32768.0).astype(np.float32)
    for i, l in enumerate(lens):
        x[i, l:] = 0
    feats, frames = e.linear_batch(dev(x), dev(np.array(lens, np.int32)), False, -20.0)
    feats = feats.cpu().numpy()
    for i, l in enumerate(lens):
        ref = ofb.linear_spectrogram(x[i, :l])
        assert int(frames[i]) == ref.shape[0]
        if ref.shape[0]:
            assert np.abs(feats[i, :ref.shape[0]] - ref).max() < 2e-5, (i, np.abs(feats[i, :ref.shape[0]] - ref).max())
        assert np.all(feats[i, ref.shape[0]:] == 0.0)
    # silence: log(0 + 1e-14)
    feats, _ = e.linear_batch(dev(np.zeros((1, 800), np.float32)), dev(np.array([800], np.int32)), False, -20.0)
    assert np.allclose(feats.cpu().numpy(), np.log(1e-14), atol=1e-5)


def test_mfcc_against_oracle(eng512, oracle_mods):
    e, _ = eng512
    oc, od, ofb, weights, _ = oracle_mods
    z = g('features.npz')
    pcm = z['pcm']
    n = dev(np.array([len(pcm)], np.int32))
    mf, frames = e.mfcc_batch(dev(pcm[None, :]), n, 40, True, -20.0)
    fbk, _ = e.fbank_batch(dev(pcm[None, :]), n, True, -20.0)
    assert int(frames[0]) == 198 and mf.shape == (1, 198, 40)
    mf, fbk = mf[0].cpu().numpy(), fbk[0].cpu().numpy().astype(np.float64)
    # the DCT + lifter stage in isolation (float64 on the kernel's own log-mel energies)
    want = (fbk @ ofb.dct_matrix(40, 80).astype(np.float64)) * ofb.lifter_coeffs(40).astype(np.float64)
    assert np.abs(mf - want).max() / np.abs(want).max() < 1e-6
    # end to end against the restated kaldi.mfcc: frames holding a +-1 LSB int16 sample differ by up to 0.1 in the log-mel
    # domain (test_fbank_testwav_...), times the lifter (<= 12); everything else agrees to ~1e-4
    err = np.abs(mf - z['mfcc'])
    assert err.max() < 1.0 and np.median(err) < 1e-3, (err.max(), np.median(err))
    # other n_ceps, ragged batch
    lens = [8000, 400, 100]
    x = weights.synthetic_pcm(3, 8000, seed=9)
    for i, l in enumerate(lens):
        x[i, l:] = 0
    mf, frames = e.mfcc_batch(dev(x), dev(np.array(lens, np.int32)), 13, True, -20.0)
    assert frames.cpu().tolist() == [48, 1, 0] and mf.shape == (3, 48, 13)
    ref = ofb.featurize_samples(ofb.pcm16_to_float32(x[0]), 'mfcc', n_mfcc=13)
    err = np.abs(mf[0].cpu().numpy() - ref)
    assert err.max() < 1.0 and np.median(err) < 1e-3, (err.max(), np.median(err))
    assert np.all(mf[2].cpu().numpy() == 0.0)


@pytest.mark.parametrize('method,dim', [('linear', 161), ('mfcc', 40)])
def test_encoder_with_linear_and_mfcc_input(oracle_mods, method, dim):
    """the reference ConformerModel(input_dim=161 / 40) on the reference featurizer's output (fixture) vs the engine"""
    from masr_amd.engine import HipEngine
    oc, od, ofb, weights, _ = oracle_mods
    z = g('features.npz')
    sd = weights.conformer_state_dict(0, 512, n_mels=dim)
    sd['encoder.global_cmvn.mean'] = torch.from_numpy(z[method + '_cmvn'][0])
    sd['encoder.global_cmvn.istd'] = torch.from_numpy(z[method + '_cmvn'][1])
    e = HipEngine(sd, vocab_size=512, n_mels=dim)
    x = dev(z[method][None])
    enc = e.encode_full(x, dev(np.array([x.shape[1]], np.int32)), -1)
    probs = e.ctc_probs(enc)[0].cpu().numpy()
    assert probs.shape == z[method + '_probs'].shape
    assert np.abs(probs - z[method + '_probs']).max() < 1e-3
    assert (probs.argmax(-1) == z[method + '_probs'].argmax(-1)).mean() > 0.97
    # whole chain on the device: PCM -> features -> encoder
    feats, frames = e.features_batch(method, dev(z['pcm'][None, :]), dev(np.array([len(z['pcm'])], np.int32)), True, -20.0,
                                     n_mfcc=40)
    probs2 = e.ctc_probs(e.encode_full(feats, frames, -1))[0].cpu().numpy()
    assert np.abs(probs2 - z[method + '_probs']).max() < 2e-2
    e.close()


def test_ffn_tail_stage_matches_separate_launches(eng512):
    """offline Conformer layers: QKV projection + deferred norm_final inside the first FFN launch (ffn_pc TAIL) vs the separate
    rowgemm / layernorm launches -- same arithmetic, so the encoder output must be bit-identical; ragged batch whose last
    32-row block is partial (9 x 250 = 2250 rows)."""
    e, _ = eng512
    gen = torch.Generator().manual_seed(21)
    feats = torch.randn(9, 1003, 80, generator=gen) * 3 + 13
    lens = torch.tensor([1003, 990, 700, 1003, 512, 333, 1003, 801, 67], dtype=torch.int32)
    feats = feats * (torch.arange(1003)[None, :, None] < lens[:, None, None])
    x, n = dev(feats), dev(lens)
    fused = e.encode_full(x, n, -1).clone()
    with debug_keys(e, no_ffn_tail=1):
        plain = e.encode_full(x, n, -1).clone()
    assert fused.shape == (9, 250, 256)
    assert torch.equal(fused, plain)
    assert torch.isfinite(fused).all()


@pytest.mark.parametrize('streaming', [True, False])
def test_ffn_head_stage_matches_separate_launches(oracle_mods, streaming):
    """offline Conformer layers: depthwise conv + LayerNorm + SiLU + pointwise_conv2 + residual as the HEAD stage of the second
    FFN launch (ffn_pc HEADK) vs dwconv_ln_silu_kernel + the row-block GEMM -- same arithmetic in the same order, so the encoder
    output must be bit-identical.  Ragged batch (pad masks), sequence boundaries inside 32-row blocks (T' = 250), a partial last
    block; the causal build (constant history rows) and the streaming: False build (symmetric zero padding)."""
    from masr_amd.engine import HipEngine
    weights = oracle_mods[3]
    sd = weights.conformer_state_dict(0, 512)
    e = HipEngine(sd, vocab_size=512, streaming=streaming)
    try:
        gen = torch.Generator().manual_seed(22)
        feats = torch.randn(9, 1003, 80, generator=gen) * 3 + 13
        lens = torch.tensor([1003, 990, 700, 1003, 512, 333, 1003, 801, 67], dtype=torch.int32)
        feats = feats * (torch.arange(1003)[None, :, None] < lens[:, None, None])
        x, n = dev(feats), dev(lens)
        fused = e.encode_full(x, n, -1).clone()
        with debug_keys(e, no_ffn_head=1):
            plain = e.encode_full(x, n, -1).clone()
        assert fused.shape == (9, 250, 256) and torch.isfinite(fused).all()
        assert torch.equal(fused, plain), (fused - plain).abs().max().item()
        oc = oracle_mods[0]
        with torch.no_grad():
            ref = oc.encoder_full(sd, feats[:3], lens[:3].long(), -1, streaming=streaming)
        assert (fused[:3].cpu() - ref).abs().max() < 1e-3
    finally:
        e.close()


@pytest.mark.parametrize('chunk', [-1, 16])
def test_attention_folded_positional_keys_match_two_term_scores(oracle_mods, chunk):
    """offline attention_kernel: scores as q.(k + p) + (u.k + v.p) (FOLD, the default) vs the two-term contraction
    (q + u).k + (q + v).p (masr_debug_set key 14 = 0) -- the same value up to fp32 rounding: encoder outputs within 5e-5 of each
    other (bar vs the oracle: 1e-3), both within 1e-3 of the oracle; ragged batch, full context and the chunk-16 mask."""
    from masr_amd.engine import HipEngine
    weights = oracle_mods[3]
    sd = weights.conformer_state_dict(0, 512)
    e = HipEngine(sd, vocab_size=512)
    try:
        gen = torch.Generator().manual_seed(23)
        feats = torch.randn(6, 1003, 80, generator=gen) * 3 + 13
        lens = torch.tensor([1003, 990, 700, 512, 333, 67], dtype=torch.int32)
        feats = feats * (torch.arange(1003)[None, :, None] < lens[:, None, None])
        x, n = dev(feats), dev(lens)
        folded = e.encode_full(x, n, chunk).clone()
        with debug_keys(e, attention_fold=0):
            two_term = e.encode_full(x, n, chunk).clone()
        diff = (folded - two_term).abs().max().item()
        print(f'attention fold vs two-term (chunk {chunk}): max |enc| diff {diff:.2e}')
        assert torch.isfinite(folded).all() and diff < 5e-5
        assert diff > 0 or chunk == 0          # the switch does select two different kernels
        oc = oracle_mods[0]
        with torch.no_grad():
            ref = oc.encoder_full(sd, feats[:2], lens[:2].long(), chunk)
        assert (folded[:2].cpu() - ref).abs().max() < 1e-3 and (two_term[:2].cpu() - ref).abs().max() < 1e-3
    finally:
        e.close()
