"""CPU: the attention decoding mode's restatement, fixture, tie rules, configuration checks and refusals (no GPU anywhere here)."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_decode_ref as ar            # noqa: E402
import budget            # noqa: E402
import rescoring_ref as rr            # noqa: E402

from masr_amd import _lib
from masr_amd.decoders import attention_decoder as ad
from masr_amd.utils import synthetic
from oracle import shims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 50
DEC = dict(linear_units=384, num_blocks=2, r_num_blocks=2)
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'attention_decode_v50.npz')


def _tool():
    spec = importlib.util.spec_from_file_location('make_attention_decode_golden',
                                                  os.path.join(ROOT, 'tools', 'make_attention_decode_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def fx():
    z = np.load(FIXTURE)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def sd(fx):
    R = json.loads(str(fx['recipe']))
    return synthetic.conformer_state_dict(R['seed'], R['vocab_size'], d_ff=R['d_ff'], num_blocks=R['num_blocks'], decoder=R['decoder'])


def _rows(sd_, fx):
    B, N, _ = fx['prefixes'].shape
    out = np.zeros((B, N, V), np.float64 if sd_['decoder.left_decoder.embed.0.weight'].dtype == torch.float64 else np.float32)
    for b in range(B):
        for n in range(N):
            out[b, n] = ar.step_logp(sd_, fx['memory'][b, :fx['mem_lens'][b]], fx['prefixes'][b, n, :fx['prefix_lens'][b, n]],
                                       pe=torch.from_numpy(fx['pe']))
    return out


def _ulps(a, b):
    """distance of two float32 arrays in units in the last place (finite values of one sign, as log-probabilities are)"""
    a, b = (np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    return np.abs(a - b)


def test_restatement_equals_the_live_references_forward_one_step(fx, sd):
    """float64: the restatement IS the reference's arithmetic (1e-9); float32: every log-probability within 1 ulp of the record
    (the restatement keeps the reference's operand shapes and uses the record's positional rows)"""
    assert np.abs(_rows(rr.to64(sd), fx) - fx['logp64']).max() < 1e-9
    y32 = _rows(sd, fx)
    assert y32.dtype == np.float32 and fx['logp32'].dtype == np.float32
    u = _ulps(y32, fx['logp32'])
    print(f'float32 restatement against the record: max {u.max()} ulp, {int((u > 0).sum())} of {u.size} entries differ')
    assert u.max() <= 1
    assert np.allclose(np.exp(fx['logp64']).sum(-1), 1.0)


def test_fixture_equals_its_recipe(fx):
    tool = _tool()
    feats, flens, prefixes, plens = tool.recipe_inputs()
    assert json.loads(str(fx['recipe'])) == tool.RECIPE
    assert np.array_equal(fx['feats'], feats) and np.array_equal(fx['feat_lens'], flens)
    assert np.array_equal(fx['prefixes'], prefixes) and np.array_equal(fx['prefix_lens'], plens)
    assert fx['mem_lens'].tolist() == [32, 25, 17] and fx['memory'].shape == (3, 32, 256)
    assert sorted(fx['prefix_lens'][0].tolist()) == [0, 1, 9, 17] and fx['pe'].shape == (34, 256)
    assert fx['trace_cases'].tolist() == [[0, 0], [1, 0], [2, 0], [2, tool.EOS_BIAS]] and fx['trace_parents64'].shape == (4, 32, tool.BEAM)
    assert os.path.getsize(FIXTURE) < (1 << 20)


@pytest.mark.skipif(not shims.reference_available(), reason='the reference checkout is not present')
def test_fixture_against_the_live_reference(fx, tmp_path, monkeypatch):
    """the recorded encoder output and log-probabilities, recomputed by the live reference model"""
    tool = _tool()
    monkeypatch.setattr(tool, 'ROOT', str(tmp_path))
    os.makedirs(os.path.join(tmp_path, 'tests', 'golden'))
    monkeypatch.setattr(sys, 'argv', ['make_attention_decode_golden.py'])
    tool.main()
    z = np.load(os.path.join(tmp_path, 'tests', 'golden', 'attention_decode_v50.npz'))
    np.testing.assert_allclose(z['memory'], fx['memory'], atol=2e-5)
    assert np.array_equal(z['pe'], fx['pe'])
    assert np.abs(z['logp64'] - fx['logp64']).max() < 1e-9 and _ulps(z['logp32'], fx['logp32']).max() <= 1
    for k in ('trace_steps64', 'trace_parents64', 'trace_tokens64', 'trace_steps32'):
        assert np.array_equal(z[k], fx[k]), k
    assert np.abs(z['trace_scores64'] - fx['trace_scores64']).max() < 1e-9


def test_search_equals_the_recorded_beam_loop_where_no_tie_decides(fx, sd):
    """the per-hypothesis search of the restatement against the traces of the batched torch.topk loop over the live reference's
    steps (tools/make_attention_decode_golden.py): the same parents, tokens and scores at every step up to the first whose
    float64 decision margin does not exclude a tie -- float64 to 1e-9 (margin above 1e-6), float32 while the step is safe (margin
    above 2 C max|e_ref| of the recorded traces) with scores within C max|e_ref| of the float64 record"""
    pe = torch.from_numpy(fx['pe'])
    n = fx['trace_parents64'].shape[2]
    compared = 0
    for c, (b, bias) in enumerate(fx['trace_cases']):
        b = int(b)
        sdc = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
        sdc['decoder.left_decoder.output_layer.bias'][V - 1] += float(bias)
        mem = fx['memory'][b, :fx['mem_lens'][b]]
        r64, r32 = ar.search(rr.to64(sdc), mem, n, pe=pe), ar.search(sdc, mem, n, pe=pe)
        steps = int(fx['trace_steps64'][c])
        assert steps == r64['steps'] == len(r64['trace']) and steps == int(fx['trace_steps32'][c])
        s64, s32 = fx['trace_scores64'][c, :steps], fx['trace_scores32'][c, :steps].astype(np.float64)
        fin = np.isfinite(s64) & np.isfinite(s32)
        e_ref = float(np.abs(s32[fin] - s64[fin]).max())
        for name, r, bar, key in (('float64', r64, 1e-6, '64'), ('float32', r32, 2 * budget.C * e_ref, '32')):
            for k in range(steps):
                if not r64['margins'][k] > bar:
                    break
                parents, tokens, scores = r['trace'][k]
                assert parents == fx['trace_parents' + key][c, k].tolist(), (name, c, k)
                assert tokens == fx['trace_tokens' + key][c, k].tolist(), (name, c, k)
                want = fx['trace_scores' + key][c, k]
                if key == '64':
                    assert np.abs(np.asarray(scores) - want)[np.isfinite(want)].max() < 1e-9, (name, c, k)
                else:
                    # the recorded loop runs the beam as one batch, the restatement one hypothesis at a time: two float32
                    # evaluations of the same arithmetic, held to the budget rule against the float64 record
                    ok = np.isfinite(want)
                    err = np.abs(np.asarray(scores, np.float64)[ok] - s64[k][ok]).max()
                    assert err <= budget.C * max(e_ref, budget.ULP32 * np.abs(s64[k][ok]).max()), (name, c, k, err, e_ref)
                compared += 1
            print(f'trace {c} (utterance {b}, eos bias {bias}) {name}: {k + 1 if r64["margins"][k] > bar else k} of {steps} steps '
                  f'compared, bar {bar:.2e}, min margin {min(r64["margins"]):.2e}')
    # finished rows while others run on are part of what was compared
    assert (fx['trace_tokens64'][3, :4] == V - 1).any() and compared > 100


# ---- the rules on hand-made tables ------------------------------------------------------------------------------------------------
def test_top_n_ties_go_to_the_smaller_id():
    ninf = -np.inf
    assert [i for _, i in ar.top_n([-1.0, -0.5, -0.5, ninf, -0.5], 4)] == [1, 2, 4, 0]
    assert [i for _, i in ar.top_n([ninf, ninf, -3.0, ninf], 3)] == [2, 0, 1]
    assert [i for _, i in ar.top_n(np.float32([0.25, 0.25, 0.25]), 2)] == [0, 1]


def test_merge_ties_finished_rows_and_the_first_step():
    ninf, eos = -np.inf, 4
    # step 1: only rank 0 is finite; the -inf candidates tie and go by flat index, so rank 0's top N fill the beam in order
    tops = [[(-0.1, 2), (-0.2, 0), (-0.3, 3)]] * 3
    new = ar.merge([0.0, ninf, ninf], tops, [False] * 3, 3, eos)
    assert [(h, t) for _, h, t in new] == [(0, 2), (0, 0), (0, 3)] and [s for s, _, _ in new] == [-0.1, -0.2, -0.3]
    # a beam wider than the finite candidates: the -inf ones follow by flat index
    new = ar.merge([0.0, ninf], [[(-0.1, 2), (ninf, 0)]] * 2, [False, False], 2, eos)
    assert [(s, h, t) for s, h, t in new] == [(-0.1, 0, 2), (ninf, 0, 0)]
    # equal sums: the smaller parent_rank * N + candidate_rank first
    new = ar.merge([-1.0, -1.5], [[(-1.0, 1), (-1.5, 2)], [(-0.5, 3), (-1.0, 0)]], [False, False], 2, eos)
    assert [(s, h, t) for s, h, t in new] == [(-2.0, 0, 1), (-2.0, 1, 3)]
    # a finished row offers (0, eos) alone and keeps its score; its other candidates are -inf | eos
    new = ar.merge([-1.0, -1.5], [None, [(-0.2, 3), (-0.9, 0)]], [True, False], 2, eos)
    assert [(s, h, t) for s, h, t in new] == [(-1.0, 0, eos), (-1.7, 1, 3)]
    new = ar.merge([-1.0, ninf], [None, None], [True, True], 2, eos)
    assert [(s, h, t) for s, h, t in new] == [(-1.0, 0, eos), (ninf, 0, eos)]


def test_search_stops_limits_and_extra_steps_on_a_table():
    """a hand-made model: the log-probabilities depend on the prefix length alone; eos wins from step 3 on"""
    Vt, eos = 5, 4

    def logp(toks):
        row = np.log(np.array([0.4, 0.3, 0.2, 0.05, 0.05]))
        if len(toks) >= 2:
            row = np.log(np.array([0.01, 0.01, 0.01, 0.01, 0.96]))
        return row
    mem = np.zeros((9, 1))
    r = ar.search(None, mem, 2, logp_fn=logp, vocab=Vt)
    assert r['limit'] == 9 and r['steps'] == 3 and [h for h, _ in r['hyps']] == [[0, 0], [0, 1]]
    assert np.isclose(r['hyps'][0][1], np.log(0.4 * 0.4 * 0.96))
    full = ar.search(None, mem, 2, logp_fn=logp, vocab=Vt, run_to_limit=True)
    assert full['hyps'] == r['hyps'] and len(full['trace']) == 9 and len(r['trace']) == 3
    cut = ar.search(None, mem, 2, logp_fn=logp, vocab=Vt, max_len=2)
    assert cut['limit'] == cut['steps'] == 2 and [h for h, _ in cut['hyps']] == [[0, 0], [0, 1]]
    assert cut['trace'] == r['trace'][:2]
    short = ar.search(None, mem[:1], 2, logp_fn=logp, vocab=Vt)
    assert short['limit'] == 1 and [h for h, _ in short['hyps']] == [[0], [1]]
    assert ar.limit_of(40, 0, 30) == 29 and ar.limit_of(40, 7, 30) == 7 and ar.limit_of(3, 7, 30) == 3


# ---- configuration and refusals ---------------------------------------------------------------------------------------------------
def test_attention_conf_defaults_and_refusals():
    assert ad.validate_attention_conf(None) == {'beam_size': 10, 'max_len': 0}
    assert ad.validate_attention_conf({'beam_size': 64, 'max_len': 7}, 64) == {'beam_size': 64, 'max_len': 7}
    with pytest.raises(_lib.MasrError, match='attention_decoder_conf.ctc_weight is not a known key'):
        ad.validate_attention_conf({'ctc_weight': 0.5})
    for beam in (0, 65, True, 2.0, '4'):
        with pytest.raises(_lib.MasrError, match='attention_decoder_conf.beam_size'):
            ad.validate_attention_conf({'beam_size': beam})
    with pytest.raises(_lib.MasrError, match='exceeds the vocabulary of 50'):
        ad.validate_attention_conf({'beam_size': 51}, V)
    for max_len in (-1, 1.5, False):
        with pytest.raises(_lib.MasrError, match='attention_decoder_conf.max_len'):
            ad.validate_attention_conf({'max_len': max_len})
    assert 'predict_stream' in ad.STREAM_REFUSAL and "decoder='attention' " in ad.STREAM_REFUSAL
    assert 'attention_rescoring' not in ad.STREAM_REFUSAL


def test_c_abi_refuses_by_name_before_it_needs_a_device():
    lib = _lib.lib()
    err = lambda: lib.masr_last_error().decode()
    buf = np.ones(64, np.int32)
    p = buf.ctypes.data_as(C.c_void_p)
    dec = lambda B, Tp, N, max_len, lcap: lib.masr_attention_decode(None, p, p, B, Tp, N, max_len, p, lcap, p, p, None, None)
    assert dec(1, 4, 0, 0, 4) != 0 and 'beam_size = 0 is outside 1 .. 64' in err()
    assert dec(1, 4, 65, 0, 4) != 0 and 'beam_size = 65 is outside 1 .. 64' in err()
    assert dec(1, 4, 4, 0, 0) != 0 and 'Lcap must be at least 1' in err()
    assert dec(1024, 4, 64, 0, 4) != 0 and 'must not exceed 65535' in err()
    assert dec(1, 4, 4, -1, 4) != 0 and 'max_len' in err()
    assert dec(1, 4, 4, 0, 4) != 0 and err() == 'engine not finalized'
    assert lib.masr_attention_decode(None, None, p, 1, 4, 4, 0, p, 4, p, p, None, None) != 0 and 'null argument' in err()
    step = lambda N, top: lib.masr_op_decoder_step(None, p, p, 1, 4, p, p, N, 2, top, p, p, None, None)
    assert step(65, 1) != 0 and 'outside 1 .. 64' in err()
    assert step(1, 1) != 0 and err() == 'engine not finalized'


def _stub(decoder, use_model='conformer'):
    from masr_amd.utils.utils import dict_to_object
    return dict_to_object({'streaming': True, 'use_model': use_model, 'decoder': decoder})


def test_stream_pool_predict_stream_and_decode_refuse_the_decoder_by_name():
    from masr_amd.predict import MASRPredictor
    from masr_amd.serving import StreamPool

    class Stub:
        configs = _stub('attention')
    with pytest.raises(Exception) as err:
        StreamPool(Stub())
    assert str(err.value) == ad.STREAM_REFUSAL and 'unknown decoder' not in str(err.value)
    pred = object.__new__(MASRPredictor)
    pred.configs, pred._pool = Stub.configs, None
    with pytest.raises(Exception) as err:
        pred.predict_stream(b'\x00' * 3200)
    assert str(err.value) == ad.STREAM_REFUSAL and pred._pool is None
    with pytest.raises(Exception) as err:
        pred.decode(np.zeros((4, V), np.float32), False, False)
    assert str(err.value) == ad.DECODE_REFUSAL and "decoder='attention' needs the encoder output" in ad.DECODE_REFUSAL


def test_an_unknown_decoder_string_keeps_its_behaviour(monkeypatch):
    """serving still answers `unknown decoder`; decode() still falls through to the greedy decoder"""
    from masr_amd import predict as predict_mod
    from masr_amd.serving import StreamPool

    class Stub:
        configs = _stub('attention_rescore')
    with pytest.raises(Exception, match='unknown decoder attention_rescore'):
        StreamPool(Stub())
    pred = object.__new__(predict_mod.MASRPredictor)
    pred.configs = Stub.configs

    class TF:
        vocab_list = synthetic.synthetic_vocab(V)
    pred._text_featurizer = TF()
    monkeypatch.setattr(predict_mod, 'greedy_decoder', lambda probs_seq, vocabulary: (1.0, 'greedy'))
    assert pred.decode(np.zeros((3, V), np.float32), False, False) == (1.0, 'greedy')


def test_deepspeech2_is_refused_before_anything_is_loaded(tmp_path):
    from masr_amd.predict import MASRPredictor
    vpath = os.path.join(tmp_path, 'vocabulary.txt')
    with open(vpath, 'w', encoding='utf-8') as f:
        for t in synthetic.synthetic_vocab(V):
            f.write(f'{t}\t1\n')
    cfg = {'preprocess_conf': {'feature_method': 'fbank', 'n_mels': 80, 'n_mfcc': 40, 'sample_rate': 16000,
                               'use_dB_normalization': True, 'target_dB': -20},
           'dataset_conf': {'dataset_vocab': vpath}, 'use_model': 'deepspeech2', 'streaming': True, 'decoder': 'attention',
           'metrics_type': 'cer'}
    with pytest.raises(Exception) as err:
        MASRPredictor(configs=cfg, use_gpu=True, state_dict={})
    assert str(err.value) == ad.DS2_REFUSAL and "decoder='attention'" in ad.DS2_REFUSAL
    cfg.update(use_model='conformer', attention_decoder_conf={'beam_size': V + 1})
    with pytest.raises(_lib.MasrError, match='exceeds the vocabulary'):
        MASRPredictor(configs=cfg, use_gpu=True, state_dict={})


@pytest.mark.parametrize('decoder', ['ctc_greedy', 'attention'])
def test_inference_predictor_asks_for_the_decoder_for_attention(monkeypatch, sd, decoder):
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
    if decoder == 'attention':
        assert seen['attention_decoder'] is True and dict(seen['decoder_conf']) == dconf
    else:
        assert 'attention_decoder' not in seen and 'decoder_conf' not in seen


# ---- the end-to-end inputs --------------------------------------------------------------------------------------------------------
def test_end_to_end_safety_cap_holds_for_the_float32_restatement(sd):
    """the cap of the GPU search-parity test for ITS inputs (attention_decode_ref.E2E), on the CPU: the utterances through the
    oracle's features and encoder; the limits are 18 .. 32 steps, all different; at least 6 of 8 searches are safe (every step's
    float64 decision margin exceeds 2 C max|e_ref| of the trace), and there the float32 search returns the float64 one's
    hypotheses in order"""
    from oracle import conformer as oc, fbank as ofb
    E = ar.E2E
    pcm = synthetic.synthetic_pcm(len(E['lens']), max(E['lens']), seed=E['pcm_seed'])
    feats = [ofb.featurize_pcm16(pcm[i, :n])[0] for i, n in enumerate(E['lens'])]
    T = max(f.shape[0] for f in feats)
    batch = np.zeros((len(feats), T, 80), np.float32)
    for i, f in enumerate(feats):
        batch[i, :f.shape[0]] = f
    frames = [f.shape[0] for f in feats]
    with torch.no_grad():
        enc = oc.encoder_full(sd, torch.from_numpy(batch), torch.tensor(frames), -1).numpy()
    valid = [oc.subsampled_len(f) for f in frames]
    assert min(valid) >= 18 and max(valid) <= 32 and len(set(valid)) == 8
    sd64, safe = rr.to64(sd), 0
    for b in range(len(feats)):
        r64 = ar.search(sd64, enc[b, :valid[b]], E['beam_size'])
        r32 = ar.search(sd, enc[b, :valid[b]], E['beam_size'])
        e_ref, unsafe = ar.safety(r64, r32, budget.C)
        print(f'E2E (CPU) utterance {b}: limit {r64["limit"]}, steps {r64["steps"]}, min margin {min(r64["margins"]):.3e}, '
              f'2 C max|e_ref| {2 * budget.C * e_ref:.3e}, first unsafe step {unsafe}')
        if unsafe is None:
            safe += 1
            assert [h for h, _ in r32['hyps']] == [h for h, _ in r64['hyps']]
    assert safe >= 6, safe
