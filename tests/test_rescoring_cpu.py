"""CPU: the attention-rescoring decoder's restatement, fixture, configuration checks and tie rule (no GPU anywhere here)."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rescoring_ref as rr            # noqa: E402

from masr_amd import _lib
from masr_amd import engine as eng_mod
from masr_amd.decoders import attention_rescoring as ar
from masr_amd.utils import synthetic
from oracle import shims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 50
DEC = dict(linear_units=384, num_blocks=2, r_num_blocks=2)


def _tool():
    spec = importlib.util.spec_from_file_location('make_rescoring_golden', os.path.join(ROOT, 'tools', 'make_rescoring_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def fx():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'rescoring_v50.npz'))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def sd(fx):
    R = json.loads(str(fx['recipe']))
    return synthetic.conformer_state_dict(R['seed'], R['vocab_size'], d_ff=R['d_ff'], num_blocks=R['num_blocks'], decoder=R['decoder'])


def test_restatement_equals_the_live_references_record(fx, sd):
    """float64: the restatement IS the reference's arithmetic (1e-9); float32: per position the Conformer pins' atol of
    tests/test_oracle_golden.py (2e-5), summed over the L + 1 positions of a hypothesis"""
    a64 = rr.scores(rr.to64(sd), fx['memory'], fx['mem_lens'], fx['hyps'], fx['hyp_lens'])
    assert np.abs(a64[0] - fx['att64']).max() < 1e-9 and np.abs(a64[1] - fx['r_att64']).max() < 1e-9
    a32 = rr.scores(sd, fx['memory'], fx['mem_lens'], fx['hyps'], fx['hyp_lens'])
    bar = 2e-5 * (fx['hyp_lens'] + 1)
    assert (np.abs(a32[0] - fx['att32']) <= bar).all() and (np.abs(a32[1] - fx['r_att32']) <= bar).all()
    assert a32[0].dtype == np.float32 and a64[0].dtype == np.float64


def test_fixture_equals_its_recipe(fx):
    tool = _tool()
    feats, flens, hyps, hlens = tool.recipe_inputs()
    assert json.loads(str(fx['recipe'])) == tool.RECIPE
    assert np.array_equal(fx['feats'], feats) and np.array_equal(fx['feat_lens'], flens)
    assert np.array_equal(fx['hyps'], hyps) and np.array_equal(fx['hyp_lens'], hlens)
    # (the reference's subsampled mask keeps frame t while 4 t < len: ceil(len / 4) valid encoder frames)
    assert fx['mem_lens'].tolist() == [32, 25, 17] and fx['memory'].shape == (3, 32, 256)
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'rescoring_v50.npz')) < (1 << 20)


@pytest.mark.skipif(not shims.reference_available(), reason='the reference checkout is not present')
def test_fixture_against_the_live_reference(fx, tmp_path, monkeypatch):
    """the recorded encoder output and scores, recomputed by the live reference model"""
    tool = _tool()
    monkeypatch.setattr(tool, 'ROOT', str(tmp_path))
    os.makedirs(os.path.join(tmp_path, 'tests', 'golden'))
    monkeypatch.setattr(sys, 'argv', ['make_rescoring_golden.py'])
    tool.main()
    z = np.load(os.path.join(tmp_path, 'tests', 'golden', 'rescoring_v50.npz'))
    np.testing.assert_allclose(z['memory'], fx['memory'], atol=2e-5)
    for k in ('att64', 'r_att64', 'att32', 'r_att32'):
        np.testing.assert_allclose(z[k], fx[k], rtol=2e-6, atol=2e-5 * 18)


def test_default_synthetic_checkpoints_hold_no_decoder(sd):
    plain = synthetic.conformer_state_dict(11, V, d_ff=256, num_blocks=2)
    assert not any(k.startswith('decoder.') for k in plain)
    assert all(torch.equal(plain[k], sd[k]) for k in plain) and len(sd) > len(plain)


def test_decoder_conf_acceptance_and_refusals(sd):
    ok = dict(attention_heads=4, **DEC)
    assert eng_mod._validate_decoder_conf('conformer', ok, sd, 256) == (4, 384, 2, 2)
    assert eng_mod._validate_decoder_conf('squeezeformer', dict(ok, normalize_before=True, concat_after=False), sd, 256)[2:] == (2, 2)

    def refused(match, conf=ok, model='conformer', state=sd, d=256):
        with pytest.raises(_lib.MasrError, match=match):
            eng_mod._validate_decoder_conf(model, conf, state, d)
    refused('deepspeech2 has no attention decoder', model='deepspeech2')
    refused('no decoder.left_decoder', state={k: v for k, v in sd.items() if not k.startswith('decoder.')})
    refused('decoder_conf.normalize_before=False', dict(ok, normalize_before=False))
    refused('decoder_conf.concat_after=True', dict(ok, concat_after=True))
    refused('decoder_conf.use_output_layer=False', dict(ok, use_output_layer=False))
    refused('decoder_conf.attention_heads=8', dict(ok, attention_heads=8))
    refused('decoder_conf.linear_units=1024 but the checkpoint was trained with linear_units=384', dict(ok, linear_units=1024))
    refused('decoder_conf.num_blocks=3 but the checkpoint holds 2', dict(ok, num_blocks=3))
    refused('decoder_conf.num_blocks=1 but the checkpoint holds 2', dict(ok, num_blocks=1))
    refused('decoder_conf.r_num_blocks=0 but the checkpoint holds 2', dict(ok, r_num_blocks=0))
    refused('decoder_conf.r_num_blocks=3 but the checkpoint holds 2', dict(ok, r_num_blocks=3))
    refused('decoder_conf.linear_units=2048', {})               # the reference's defaults are not this checkpoint's
    refused('decoder_conf.num_blocks=6', dict(attention_heads=4, linear_units=384))


def test_rescoring_conf_defaults_and_refusals():
    c = ar.validate_rescoring_conf(None, {'ctc_weight': 0.3, 'reverse_weight': 0.3}, 3)
    assert c == {'beam_size': 10, 'ctc_weight': 0.5, 'reverse_weight': 0.3, 'cutoff_prob': 0.99, 'cutoff_top_n': 40,
                 'num_processes': 10}
    assert ar.validate_rescoring_conf({'reverse_weight': 0.0, 'beam_size': 64}, {'reverse_weight': 0.3}, 0)['reverse_weight'] == 0
    assert ar.validate_rescoring_conf({'beam_size': 1}, None, 0)['reverse_weight'] == 0
    for bad in (0, 65, 2.5, True, '10'):
        with pytest.raises(_lib.MasrError, match='beam_size'):
            ar.validate_rescoring_conf({'beam_size': bad})
    with pytest.raises(_lib.MasrError, match='reverse_weight=0.3 needs the right-to-left decoder'):
        ar.validate_rescoring_conf(None, {'reverse_weight': 0.3}, 0)
    with pytest.raises(_lib.MasrError, match='cutoff_top_n'):
        ar.validate_rescoring_conf({'cutoff_top_n': 0})
    with pytest.raises(_lib.MasrError, match='not a known key'):
        ar.validate_rescoring_conf({'alpha': 1.0})
    with pytest.raises(_lib.MasrError, match='longer than max_pos - 1'):
        ar.build_table([[list(range(1, 12))]], max_pos=11)
    assert 'predict_stream' in ar.STREAM_REFUSAL and 'left out' in ar.STREAM_REFUSAL


def test_c_abi_refuses_by_name_before_it_needs_a_device():
    lib = _lib.lib()
    err = lambda: lib.masr_last_error().decode()
    for args, match in (((3, 384, 2, 2), 'decoder_conf.attention_heads=3'), ((4, 100, 2, 2), 'decoder_conf.linear_units=100'),
                        ((4, 384, 0, 2), 'decoder_conf.num_blocks=0'), ((4, 384, 2, -1), 'decoder_conf.r_num_blocks=-1')):
        assert lib.masr_decoder_enable(None, *args) != 0 and match in err(), (args, err())
    # accepted numbers fail only for want of an engine (a device)
    assert lib.masr_decoder_enable(None, 4, 384, 2, 2) != 0 and err() == 'null engine'
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data_as(C.c_void_p)
    for fn in (lib.masr_rescore, lib.masr_op_decoder_scores):
        assert fn(None, p, p, 1, 4, p, p, 0, 2, 1, p, p, None) != 0 and 'outside 1 .. 64' in err()
        assert fn(None, p, p, 1, 4, p, p, 65, 2, 1, p, p, None) != 0 and 'outside 1 .. 64' in err()
        assert fn(None, p, p, 1, 4, None, p, 1, 2, 1, p, p, None) != 0 and 'null argument' in err()
    buf[:] = 1
    assert lib.masr_op_decoder_scores(None, p, p, 1, 4, p, p, 1, 2, 1, p, p, None) != 0 and err() == 'engine not finalized'
    buf[0] = 9                                   # (enc_lens, hyps and hyp_lens alias: 9 frames > Tp)
    assert lib.masr_op_decoder_scores(None, p, p, 1, 4, p, p, 1, 2, 1, p, p, None) != 0 and 'outside 1 .. Tp' in err()
    assert lib.masr_rescore(None, p, p, 1, 4, p, p, 1, 2, 1, p, p, None) != 0 and err() == 'engine not finalized'


class _FakeLib:
    """records every C-ABI call of an engine's construction"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _construct(monkeypatch, sd, **kw):
    fake = _FakeLib()
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    monkeypatch.setattr(_lib, 'lib', lambda: fake)
    monkeypatch.setattr(eng_mod, '_stream', lambda: None)
    monkeypatch.setattr(eng_mod, 'check', lambda rc: None)
    e = eng_mod.HipEngine(sd, encoder_conf=dict(num_blocks=2, linear_units=256), vocab_size=V, **kw)
    e.h = None                                   # nothing to destroy
    return [a[1].decode() for n, a in fake.calls if n == 'masr_load_tensor'], [n for n, _ in fake.calls], fake


def test_greedy_and_beam_construction_never_touch_the_decoder(monkeypatch, sd):
    """the engine of ``ctc_greedy`` / ``ctc_beam_search`` (both build it the same way) loads no decoder.* tensor and never calls
    masr_decoder_enable; the engine of ``attention_rescoring`` enables the decoder first and loads both halves"""
    loaded, names, _ = _construct(monkeypatch, sd)
    assert loaded and not any(k.startswith('decoder.') for k in loaded) and 'masr_decoder_enable' not in names
    loaded, names, fake = _construct(monkeypatch, sd, attention_decoder=True, decoder_conf=dict(attention_heads=4, **DEC))
    assert names.index('masr_decoder_enable') < names.index('masr_load_tensor') < names.index('masr_finalize')
    assert [a[1:] for n, a in fake.calls if n == 'masr_decoder_enable'] == [(4, 384, 2, 2)]
    want = {k for k in sd if k.startswith(('decoder.left_decoder.', 'decoder.right_decoder.'))}
    assert want and want <= set(loaded)


def test_tie_rule_and_combination():
    att, r_att, ctc = [-10.0, -8.0, -8.0, -12.0], [-9.0, -7.0, -7.0, -1.0], [-1.0, -2.0, -2.0, -30.0]
    total = ar.combine(att, r_att, ctc, 0.5, 0.3)
    assert np.allclose(total, rr.combine(att, r_att, ctc, 0.5, 0.3)) and np.isclose(total[0], -10 * 0.7 - 9 * 0.3 - 0.5)
    assert total[1] == total[2] == total.max() and ar.pick(total) == 1 == rr.pick(total)
    assert ar.pick(total, 1) == 0                                 # only the first `count` hypotheses of a table are real
    assert ar.pick(ar.combine(att, r_att, ctc, 0.5, 0.0)) == 1 and ar.pick([-3.0, -3.0, -3.0]) == 0
    hyps, lens, count = ar.build_table([[[1, 2, 3], []], [[4]]])
    assert hyps.shape == (2, 2, 3) and lens.tolist() == [[3, 0], [1, 0]] and count.tolist() == [2, 1]


def test_host_search_hands_back_its_n_best_in_rank_order():
    """masr_beam_search_batch_nbest: entry 0 is masr_beam_search_batch's result bit for bit, scores descend"""
    lib = _lib.lib()
    rng = np.random.default_rng(2)
    B, T, K, beam = 3, 24, 6, 8
    p = rng.dirichlet(np.ones(K) * 0.3, (B, T)).astype(np.float32)
    order = np.argsort(-p, axis=-1)
    idx = np.ascontiguousarray(order.astype(np.int32))
    logp = np.ascontiguousarray(np.log(np.take_along_axis(p, order, -1) + np.finfo(np.float32).tiny).astype(np.float32))
    cnt = np.full((B, T), K, np.int32)
    frames = np.array([24, 17, 9], np.int32)
    as_p = lambda a: a.ctypes.data_as(C.c_void_p)
    t1, l1, s1 = np.zeros((B, T), np.int32), np.zeros(B, np.int32), np.zeros(B, np.float32)
    assert lib.masr_beam_search_batch(as_p(idx), as_p(logp), as_p(cnt), as_p(frames), B, T, K, beam, 0, 2, as_p(t1), T, as_p(l1),
                                      as_p(s1)) == 0
    tn, ln, sn, cn = np.zeros((B, beam, T), np.int32), np.zeros((B, beam), np.int32), np.zeros((B, beam), np.float32), np.zeros(B, np.int32)
    assert lib.masr_beam_search_batch_nbest(as_p(idx), as_p(logp), as_p(cnt), as_p(frames), B, T, K, beam, 0, 2, beam, as_p(tn), T,
                                            as_p(ln), as_p(sn), as_p(cn)) == 0
    for b in range(B):
        assert 1 < cn[b] <= beam and ln[b, 0] == l1[b] and sn[b, 0] == s1[b]
        assert tn[b, 0, :l1[b]].tolist() == t1[b, :l1[b]].tolist()
        assert (np.diff(sn[b, :cn[b]]) <= 0).all()
        assert len({tuple(tn[b, n, :ln[b, n]]) for n in range(cn[b])}) == cn[b]


def test_end_to_end_margin_cap_holds_for_the_float32_restatement(sd):
    """the cap of the GPU end-to-end test for ITS seeds (rescoring_ref.E2E), on the CPU: the same utterances through the oracle's
    features, encoder and CTC head, the pruning rule and the library's host-thread n-best search; the float64 top-2 margin of
    the combined score exceeds 2 C max|e_ref| for at least three quarters of the utterances, and there the float32 restatement
    picks what the float64 one picks"""
    import budget
    from oracle import beam_search as obs, conformer as oc, fbank as ofb
    E = rr.E2E
    pcm = synthetic.synthetic_pcm(len(E['lens']), max(E['lens']), seed=E['pcm_seed'])
    feats = [ofb.featurize_pcm16(pcm[i, :n])[0] for i, n in enumerate(E['lens'])]
    T = max(f.shape[0] for f in feats)
    batch = np.zeros((len(feats), T, 80), np.float32)
    for i, f in enumerate(feats):
        batch[i, :f.shape[0]] = f
    frames = [f.shape[0] for f in feats]
    with torch.no_grad():
        enc = oc.encoder_full(sd, torch.from_numpy(batch), torch.tensor(frames), -1)
        probs = oc.ctc_probs(sd, enc).numpy()
    memory, valid = enc.numpy(), [oc.subsampled_len(f) for f in frames]
    B, Ts, K, beam = len(feats), probs.shape[1], E['cutoff_top_n'], E['beam_size']
    idx, logp, cnt = np.zeros((B, Ts, K), np.int32), np.zeros((B, Ts, K), np.float32), np.zeros((B, Ts), np.int32)
    for b in range(B):
        for t in range(valid[b]):
            c = obs.pruned_log_probs(probs[b, t], E['cutoff_prob'], K)
            cnt[b, t] = len(c)
            idx[b, t, :len(c)], logp[b, t, :len(c)] = [k for k, _ in c], [v for _, v in c]
    as_p = lambda a: a.ctypes.data_as(C.c_void_p)
    toks, lens = np.zeros((B, beam, Ts), np.int32), np.zeros((B, beam), np.int32)
    ctc, count = np.zeros((B, beam), np.float32), np.zeros(B, np.int32)
    fr = np.array(valid, np.int32)
    assert _lib.lib().masr_beam_search_batch_nbest(as_p(idx), as_p(logp), as_p(cnt), as_p(fr), B, Ts, K, beam, 0, 2, beam, as_p(toks), Ts,
                                                   as_p(lens), as_p(ctc), as_p(count)) == 0
    kept = 0
    for b in range(B):
        n = int(count[b])
        Lmax = max(1, int(lens[b, :n].max()))
        hyps, hl = toks[b:b + 1, :n, :Lmax], lens[b:b + 1, :n]
        a64 = rr.scores(rr.to64(sd), memory[b:b + 1], fr[b:b + 1], hyps, hl)
        a32 = rr.scores(sd, memory[b:b + 1], fr[b:b + 1], hyps, hl)
        t64 = rr.combine(a64[0][0], a64[1][0], ctc[b, :n], E['ctc_weight'], E['reverse_weight'])
        t32 = rr.combine(a32[0][0], a32[1][0], ctc[b, :n], E['ctc_weight'], E['reverse_weight'])
        top = np.sort(t64)
        margin, bar = (top[-1] - top[-2] if n > 1 else np.inf), 2 * budget.C * np.abs(t32 - t64).max()
        print(f'E2E (CPU) utterance {b}: n-best {n}, lengths {hl[0].tolist()}, margin {margin:.3e}, bar {bar:.3e}, '
              f'att rank {np.argsort(-a64[0][0]).tolist()}, ctc rank {np.argsort(-ctc[b, :n]).tolist()}')
        if margin > bar:
            kept += 1
            assert rr.pick(t32) == rr.pick(t64)
    assert kept >= (3 * B + 3) // 4, kept


def test_stream_pool_and_predict_stream_refuse_the_decoder_by_name():
    """serving.StreamPool reaches its own refusal (not the 'unknown decoder' branch) before it touches an engine, and
    MASRPredictor.predict_stream raises the same text before it opens a pool"""
    from masr_amd.predict import MASRPredictor
    from masr_amd.serving import StreamPool
    from masr_amd.utils.utils import dict_to_object

    class Stub:
        configs = dict_to_object({'streaming': True, 'use_model': 'conformer', 'decoder': 'attention_rescoring'})
    with pytest.raises(Exception) as err:
        StreamPool(Stub())
    assert str(err.value) == ar.STREAM_REFUSAL and 'unknown decoder' not in str(err.value)
    pred = object.__new__(MASRPredictor)
    pred.configs, pred._pool = Stub.configs, None
    with pytest.raises(Exception) as err:
        pred.predict_stream(b'\x00' * 3200)
    assert str(err.value) == ar.STREAM_REFUSAL and pred._pool is None


@pytest.mark.parametrize('decoder', ['ctc_greedy', 'ctc_beam_search', 'attention_rescoring'])
def test_inference_predictor_asks_for_the_decoder_only_when_rescoring(monkeypatch, sd, decoder):
    """the ``configs.decoder`` switch of InferencePredictor: attention_decoder / decoder_conf reach HipEngine for
    attention_rescoring alone; the other two build the engine with the arguments they always passed"""
    from masr_amd.infer_utils import inference_predictor as ip
    from masr_amd.utils.utils import dict_to_object
    seen = {}

    class Engine:
        def __init__(self, state_dict, **kw):
            seen.update(kw)
    monkeypatch.setattr(ip, 'HipEngine', Engine)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    dconf = dict(attention_heads=4, **DEC)
    cfg = dict_to_object({'decoder': decoder, 'encoder_conf': {'num_blocks': 2}, 'decoder_conf': dconf, 'preprocess_conf': {}})
    ip.InferencePredictor(configs=cfg, use_model='conformer', streaming=True, state_dict=sd)
    if decoder == 'attention_rescoring':
        assert seen['attention_decoder'] is True and dict(seen['decoder_conf']) == dconf
    else:
        assert 'attention_decoder' not in seen and 'decoder_conf' not in seen
    assert set(seen) - {'attention_decoder', 'decoder_conf'} == {'encoder_conf', 'streaming', 'n_mels', 'use_model'}
