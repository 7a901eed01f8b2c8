"""GPU: the attention decoder of the second pass (masr_rescore / masr_op_decoder_scores, csrc/decoder.hip) against the plain-torch
restatement (tests/rescoring_ref.py) under the float64 budget rule of tests/budget.py (C = 8 unchanged: truth = the restatement in
float64, reference = the restatement in float32), bit-for-bit invariance of a hypothesis' scores, parity with the live reference's
record (tests/golden/rescoring_v50.npz) and the decoder end to end through MASRPredictor.

V = 50, d = 256 / 4 heads, decoder 2 + 2 blocks, linear_units 384 unless a case says otherwise."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import budget            # noqa: E402
import rescoring_ref as rr            # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
V = 50
DEC = dict(linear_units=384, num_blocks=2, r_num_blocks=2)
DEC_CONF = dict(attention_heads=4, **DEC)
ENC_CONF = dict(num_blocks=2, linear_units=256)


def _fixture():
    z = np.load(os.path.join(GOLDEN, 'rescoring_v50.npz'))
    return {k: z[k] for k in z.files}


def _sd(decoder=DEC, **kw):
    from masr_amd.utils import synthetic
    R = json.loads(str(_fixture()['recipe']))
    return synthetic.conformer_state_dict(R['seed'], V, d_ff=256, num_blocks=2, decoder=decoder, **kw)


@pytest.fixture(scope='module')
def fx():
    return _fixture()


@pytest.fixture(scope='module')
def sd():
    return _sd()


@pytest.fixture(scope='module')
def eng(sd):
    from masr_amd.engine import HipEngine
    e = HipEngine(sd, encoder_conf=ENC_CONF, vocab_size=V, attention_decoder=True, decoder_conf=DEC_CONF)
    yield e
    e.close()


@pytest.fixture(scope='module')
def truth(fx, sd):
    """the restatement on the fixture's table, once: float64 truth and float32 reference"""
    a64 = rr.scores(rr.to64(sd), fx['memory'], fx['mem_lens'], fx['hyps'], fx['hyp_lens'])
    a32 = rr.scores(sd, fx['memory'], fx['mem_lens'], fx['hyps'], fx['hyp_lens'])
    return a64, a32


def _check(name, sd_, eng_, memory, mem_lens, hyps, lens, heads=4, with_right=True):
    a64 = rr.scores(rr.to64(sd_), memory, mem_lens, hyps, lens, heads, with_right)
    a32 = rr.scores(sd_, memory, mem_lens, hyps, lens, heads, with_right)
    got = eng_.op_decoder_scores(torch.as_tensor(memory).to(eng_.device), mem_lens, hyps, lens, with_right)
    budget.check(name + ' att', a64[0], a32[0], got[0])
    if with_right and rr.blocks(sd_, 'right'):
        budget.check(name + ' r_att', a64[1], a32[1], got[1])
    else:
        assert not got[1].any()
    return got


def test_ragged_batch_mixed_lengths_and_last_token(fx, eng, truth):
    """lens [131, 99, 67]; N = 4 with hypothesis lengths {0, 1, 15, 17} mixed per utterance (empty hypothesis, one token, L + 1 =
    16 and 18); one hypothesis made only of token V - 2 and one ending in it -- through masr_op_decoder_scores"""
    assert fx['feat_lens'].tolist() == [131, 99, 67] and sorted(fx['hyp_lens'][0].tolist()) == [0, 1, 15, 17]
    assert (fx['hyps'][0, 2, :15] == V - 2).all() and fx['hyps'][1, 0, 16] == V - 2
    got = eng.op_decoder_scores(torch.from_numpy(fx['memory']).to(eng.device), fx['mem_lens'], fx['hyps'], fx['hyp_lens'])
    (a64, r64), (a32, r32) = truth
    budget.check('ragged att', a64, a32, got[0])
    budget.check('ragged r_att', r64, r32, got[1])


def test_fixture_parity_with_the_live_reference_record(fx, eng):
    """att / r_att against the live reference's float64 record; the bar is the float32 record's own distance from it times C"""
    got = eng.op_decoder_scores(torch.from_numpy(fx['memory']).to(eng.device), fx['mem_lens'], fx['hyps'], fx['hyp_lens'])
    budget.check('fixture att', fx['att64'], fx['att32'], got[0])
    budget.check('fixture r_att', fx['r_att64'], fx['r_att32'], got[1])


def test_same_table_through_rescore_and_through_the_op(fx, eng):
    mem = torch.from_numpy(fx['memory']).to(eng.device)
    op = eng.op_decoder_scores(mem, fx['mem_lens'], fx['hyps'], fx['hyp_lens'])
    att, r_att = eng.rescore(mem, torch.from_numpy(fx['mem_lens']).to(eng.device), torch.from_numpy(fx['hyps']).to(eng.device),
                             torch.from_numpy(fx['hyp_lens']).to(eng.device))
    assert np.array_equal(att.cpu().numpy(), op[0]) and np.array_equal(r_att.cpu().numpy(), op[1])


def test_short_and_long_utterance(sd, eng):
    """one utterance of 67 frames (T' = 16) and one of 403 (T' = 100), memory from the engine's own encoder"""
    rng = np.random.default_rng(3)
    feats = (rng.standard_normal((2, 403, 80)) * 3 + 13).astype(np.float32)
    feats[1, 67:] = 0
    lens = torch.tensor([403, 67], dtype=torch.int32)
    enc = eng.encode_full(torch.from_numpy(feats).to(eng.device), lens.to(eng.device), -1)
    mem_lens = eng.enc_frames(lens.numpy()).astype(np.int32)
    assert enc.shape[1] == 100 and mem_lens.tolist() == [100, 16]
    hyps = rng.integers(1, V - 1, (2, 3, 9)).astype(np.int32)
    _check('T100/T16', sd, eng, enc.cpu().numpy(), mem_lens, hyps, np.array([[9, 4, 0], [1, 9, 5]], np.int32))


def test_n1_and_reverse_weight_zero(fx, sd, eng, truth):
    one = _check('N=1', sd, eng, fx['memory'], fx['mem_lens'], fx['hyps'][:, 3:4], fx['hyp_lens'][:, 3:4])
    full = eng.op_decoder_scores(torch.from_numpy(fx['memory']).to(eng.device), fx['mem_lens'], fx['hyps'], fx['hyp_lens'])
    assert np.array_equal(one[0][:, 0], full[0][:, 3]) and np.array_equal(one[1][:, 0], full[1][:, 3])
    left = _check('reverse_weight=0', sd, eng, fx['memory'], fx['mem_lens'], fx['hyps'], fx['hyp_lens'], with_right=False)
    assert np.array_equal(left[0], full[0])


def test_checkpoint_without_right_decoder(fx):
    from masr_amd._lib import MasrError
    from masr_amd.engine import HipEngine
    dec = dict(DEC, r_num_blocks=0)
    sd0 = _sd(dec)
    e = HipEngine(sd0, encoder_conf=ENC_CONF, vocab_size=V, attention_decoder=True, decoder_conf=dict(attention_heads=4, **dec))
    try:
        _check('r_num_blocks=0', sd0, e, fx['memory'], fx['mem_lens'], fx['hyps'], fx['hyp_lens'], with_right=False)
        with pytest.raises(MasrError, match='reverse_weight > 0'):
            e.op_decoder_scores(torch.from_numpy(fx['memory']).to(e.device), fx['mem_lens'], fx['hyps'], fx['hyp_lens'], True)
    finally:
        e.close()


def test_width_512_heads_8():
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    sdw = synthetic.conformer_state_dict(5, V, d=512, heads=8, d_ff=256, num_blocks=1, decoder=DEC)
    e = HipEngine(sdw, encoder_conf=dict(output_size=512, attention_heads=8, num_blocks=1, linear_units=256), vocab_size=V,
                  attention_decoder=True, decoder_conf=dict(attention_heads=8, **DEC))
    try:
        rng = np.random.default_rng(4)
        memory = rng.standard_normal((2, 21, 512)).astype(np.float32)
        hyps = rng.integers(1, V - 1, (2, 2, 17)).astype(np.int32)
        _check('512/8', sdw, e, memory, np.array([21, 13], np.int32), hyps, np.array([[17, 3], [0, 16]], np.int32), heads=8)
    finally:
        e.close()


@pytest.mark.parametrize('family', ['squeezeformer', 'efficient_conformer'])
def test_other_families_use_the_same_decoder_keys(family):
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
        enc = eng_enc = e.encode_full(torch.from_numpy(feats).to(e.device), lens.to(e.device), -1)
        mem_lens = np.asarray(e.enc_frames(lens.numpy())).astype(np.int32)
        hyps = rng.integers(1, V - 1, (2, 2, 7)).astype(np.int32)
        _check(family, sdf, e, eng_enc.cpu().numpy(), mem_lens, hyps, np.array([[7, 2], [0, 5]], np.int32))
        assert enc.shape[2] == 256
    finally:
        e.close()


def test_scores_do_not_depend_on_table_padding_or_lane(fx, eng):
    """bit for bit: a hypothesis' scores do not depend on the other hypotheses of its table, on N, on B, on the ids past its length
    or on the lane"""
    mem = torch.from_numpy(fx['memory']).to(eng.device)
    full = eng.op_decoder_scores(mem, fx['mem_lens'], fx['hyps'], fx['hyp_lens'])
    # alone: B = 1, N = 1, Lmax = its own length
    for b, n in ((0, 3), (1, 2), (2, 1), (1, 1)):
        L = int(fx['hyp_lens'][b, n])
        h = fx['hyps'][b:b + 1, n:n + 1, :max(L, 1)].copy()
        one = eng.op_decoder_scores(mem[b:b + 1].contiguous(), fx['mem_lens'][b:b + 1], h, fx['hyp_lens'][b:b + 1, n:n + 1])
        assert one[0][0, 0] == full[0][b, n] and one[1][0, 0] == full[1][b, n], (b, n)
    # other neighbours, a wider table, other ids past every length
    rng = np.random.default_rng(9)
    B, N, Lmax = fx['hyps'].shape
    wide = rng.integers(0, V, (B, N + 3, Lmax + 5)).astype(np.int32)
    wlens = rng.integers(0, Lmax + 5, (B, N + 3)).astype(np.int32)
    for b in range(B):
        for n in range(N):
            L = fx['hyp_lens'][b, n]
            wide[b, n + 2, :L] = fx['hyps'][b, n, :L]
            wlens[b, n + 2] = L
    got = eng.op_decoder_scores(mem, fx['mem_lens'], wide, wlens)
    assert np.array_equal(got[0][:, 2:2 + N], full[0]) and np.array_equal(got[1][:, 2:2 + N], full[1])
    # the other lane (its own workspaces, the library's lane stream)
    eng.select_lane(1)
    try:
        with torch.cuda.stream(eng.side_stream(4)):
            lane1 = eng.op_decoder_scores(mem, fx['mem_lens'], fx['hyps'], fx['hyp_lens'])
    finally:
        eng.select_lane(0)
    assert np.array_equal(lane1[0], full[0]) and np.array_equal(lane1[1], full[1])


def test_refusals_on_a_live_engine(fx, eng):
    from masr_amd._lib import MasrError
    mem = torch.from_numpy(fx['memory']).to(eng.device)
    bad = fx['hyp_lens'].copy()
    bad[0, 0] = fx['hyps'].shape[2] + 1
    with pytest.raises(MasrError, match='outside 0 .. Lmax'):
        eng.op_decoder_scores(mem, fx['mem_lens'], fx['hyps'], bad)
    with pytest.raises(MasrError, match='max_pos - 1'):
        eng.op_decoder_scores(mem[:1].contiguous(), fx['mem_lens'][:1], np.ones((1, 1, 5000), np.int32), np.array([[5000]], np.int32))
    with pytest.raises(MasrError, match='outside 1 .. 64'):
        eng.op_decoder_scores(mem[:1].contiguous(), fx['mem_lens'][:1], np.ones((1, 65, 2), np.int32), np.ones((1, 65), np.int32))


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
           'attention_rescoring_decoder_conf': {'beam_size': rr.E2E['beam_size'], 'ctc_weight': rr.E2E['ctc_weight']},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'conformer', 'streaming': True, 'decoder': decoder,
           'metrics_type': 'cer'}
    cfg.update(more)
    return cfg


def test_predict_batch_picks_what_the_float64_restatement_picks(tmp_path, sd):
    """end to end: for every utterance whose float64 top-2 margin of the combined score exceeds 2 C max|e_ref| the facade returns
    the hypothesis the float64 restatement picks from the same n-best; at most a quarter of the utterances may be left out"""
    from masr_amd.predict import MASRPredictor
    from masr_amd.utils import synthetic
    pred = MASRPredictor(configs=_cfg(str(tmp_path), 'attention_rescoring'), use_gpu=True, state_dict=sd)
    dec = pred.rescoring_decoder
    seen = []
    inner = dec.rescore_launch

    def spy(eng_, enc, enc_lens, nbest):
        collect = inner(eng_, enc, enc_lens, nbest)

        def collect_and_record():
            out = collect()
            seen.append((enc.cpu().numpy(), enc_lens.cpu().numpy(), nbest, out))
            return out
        return collect_and_record
    dec.rescore_launch = spy
    lens = rr.E2E['lens']
    pcm = synthetic.synthetic_pcm(8, max(lens), seed=rr.E2E['pcm_seed'])
    res = pred.predict_batch([pcm[i, :n].copy() for i, n in enumerate(lens)])
    assert len(seen) == 1 and len(res) == 8
    memory, mem_lens, nbest, out = seen[0]
    order = list(range(8))          # one pass, in input order
    kept = 0
    for j, i in enumerate(order):
        toks = [t for t, _ in nbest[j]]
        ctc = np.array([s for _, s in nbest[j]], np.float64)
        Lmax = max(1, max(len(t) for t in toks))
        hyps = np.zeros((1, len(toks), Lmax), np.int32)
        hl = np.array([[len(t) for t in toks]], np.int32)
        for n, t in enumerate(toks):
            hyps[0, n, :len(t)] = t
        a64 = rr.scores(rr.to64(sd), memory[j:j + 1], mem_lens[j:j + 1], hyps, hl)
        a32 = rr.scores(sd, memory[j:j + 1], mem_lens[j:j + 1], hyps, hl)
        t64 = rr.combine(a64[0][0], a64[1][0], ctc, dec.ctc_weight, dec.reverse_weight)
        t32 = rr.combine(a32[0][0], a32[1][0], ctc, dec.ctc_weight, dec.reverse_weight)
        e_ref = float(np.abs(t32 - t64).max())
        top = np.sort(t64)
        margin = top[-1] - top[-2] if len(top) > 1 else np.inf
        print(f'E2E utterance {i}: n-best {len(toks)}, margin {margin:.3e}, 2 C max|e_ref| {2 * budget.C * e_ref:.3e}', flush=True)
        if margin <= 2 * budget.C * e_ref:
            continue
        kept += 1
        want = toks[rr.pick(t64)]
        assert out[j][0] == want, (i, out[j][0], want)
        assert res[i]['text'] == pred._text(want)
        assert abs(res[i]['score'] - t64[rr.pick(t64)]) <= budget.C * max(e_ref, budget.ULP32 * abs(t64).max())
    assert kept >= 6, kept
    with pytest.raises(Exception, match='attention_rescoring'):
        pred.predict_stream(pcm[0, :16000].tobytes())


def test_duplicated_hypotheses_the_earlier_one_wins(fx, eng):
    from masr_amd.decoders.attention_rescoring import AttentionRescoringDecoder
    from masr_amd.utils import synthetic
    dec = AttentionRescoringDecoder(synthetic.synthetic_vocab(V), beam_size=4, ctc_weight=0.5, reverse_weight=0.3)
    # the duplicates hold the best combined score by a wide margin: short, with a CTC score the competitors are 1e3 below
    h = fx['hyps'][0, 1, :1].tolist()
    nbest = [[([3, 4], -1e3), (h, -1.0), (h, -1.0), ([5], -1e3)]]
    mem = torch.from_numpy(fx['memory'][:1]).to(eng.device)
    out = dec.rescore(eng, mem, torch.from_numpy(fx['mem_lens'][:1]).to(eng.device), nbest)
    att, r_att, total = out[0][3]
    assert att[1] == att[2] and r_att[1] == r_att[2]
    assert total[1] == total[2] == total.max() and total[0] < total[1] and total[3] < total[1]
    assert out[0][2] == 1 and out[0][0] == h


def test_greedy_engine_is_what_it_was(sd, eng):
    """an engine built WITHOUT the decoder from the same checkpoint: the parent's outputs bit for bit (the encoder and greedy
    rows do not depend on the decoder tensors being loaded) and no decoder workspace or weights"""
    from masr_amd.engine import HipEngine
    from masr_amd.utils import synthetic
    plain_sd = {k: v for k, v in sd.items() if not k.startswith(('decoder.left_decoder.', 'decoder.right_decoder.'))}
    g = HipEngine(sd, encoder_conf=ENC_CONF, vocab_size=V)
    p = HipEngine(plain_sd, encoder_conf=ENC_CONF, vocab_size=V)
    try:
        info = g.decoder_info()
        assert info == {'enabled': False, 'num_blocks': 0, 'r_num_blocks': 0, 'weight_bytes': 0, 'workspace_bytes': 0}
        pcm = torch.from_numpy(synthetic.synthetic_pcm(2, 24000, seed=3)).to(g.device)
        ns = torch.tensor([24000, 17000], dtype=torch.int32, device=g.device)
        rows = [x.transcribe_rows(pcm, ns, True, -20.0).cpu().numpy() for x in (g, p, eng)]
        assert np.array_equal(rows[0], rows[1]) and np.array_equal(rows[0], rows[2])
        assert g.decoder_info()['workspace_bytes'] == 0
        with pytest.raises(Exception, match='no attention decoder'):
            g.op_decoder_scores(torch.zeros(1, 4, 256, device=g.device), [4], np.ones((1, 1, 2), np.int32), np.ones((1, 1), np.int32))
        assert eng.decoder_info()['enabled'] and eng.decoder_info()['weight_bytes'] > 0
    finally:
        g.close()
        p.close()
