"""CPU: the float64 evaluation of the oracle and the proof that the budget rule of tests/budget.py bites.

* the float32 path of the dtype-generic restatements is bit-identical to the restatements before they became generic
  (digests recorded by oracle/make_f32_pin.py from that commit);
* deliberately perturbed ORACLES (never kernels) go through ``budget.evaluate`` in the place of the candidate: each must be
  rejected at depth 1 and at depth 12, while the unperturbed float32 oracle with another thread count (a legitimately
  different summation order) must pass;
* the stress checkpoints of tests/test_gpu_f64_budget.py keep the float32 oracle finite and leave at most 2 % of the frames
  undecided by the argmax margin.

Measured here (Conformer, ``conformer_state_dict(0, 512)`` on ``golden_inputs()``, full attention, bar = 8 x reference error):
the reference error on ``enc`` is 2.3e-6 (depth 1) / 2.8e-6 (depth 12), the perturbations land at 3e-5 ... 3e-2 (ratios in
docs/LAB_NOTES.md section 17)."""
import contextlib
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import budget


@pytest.fixture(scope='module')
def mods():
    from oracle import conformer as oc, f64, make_f32_pin, weights
    from oracle.make_golden import golden_inputs
    return oc, f64, make_f32_pin, weights, golden_inputs


@contextlib.contextmanager
def threads(n):
    keep = torch.get_num_threads()
    torch.set_num_threads(n)
    try:
        yield
    finally:
        torch.set_num_threads(keep)


def test_float32_oracle_is_bit_identical_to_the_restatements_before_they_were_dtype_generic(mods):
    make_f32_pin = mods[2]
    rec = json.load(open(make_f32_pin.OUT))
    got = make_f32_pin.compute()
    env = f'recorded with {rec["environment"]}, here {make_f32_pin.environment()}'
    assert set(got) == set(rec['digests'])
    for name in sorted(got):
        assert got[name] == rec['digests'][name], f'{name}: float32 oracle output changed ({env})'


def test_float64_evaluation_runs_every_family_and_streaming_form(mods):
    """every restatement runs in float64 end to end (no float32 tensor sneaks in: a mixed-dtype op raises) and lands within the
    float32 rounding of the float32 result"""
    oc, f64, _, weights, golden_inputs = mods
    feats, lens = golden_inputs()
    sds = {'conformer': weights.conformer_state_dict(0, 64, num_blocks=2),
           'squeezeformer': weights.squeezeformer_state_dict(0, 64, streaming=True),
           'efficient_conformer': weights.efficient_conformer_state_dict(0, 64, num_blocks=6),
           'deepspeech2': weights.deepspeech2_state_dict(0, 64, num_rnn_layers=2, bidirectional=False)}
    kw = {'squeezeformer': {'causal': True, 'decoding_chunk_size': 16}, 'conformer': {'decoding_chunk_size': 4},
          'efficient_conformer': {'decoding_chunk_size': 16}}
    windows = [(0, 67), (64, 67), (128, 23)]
    for fam, sd in sds.items():
        a, b = f64.both(fam, sd, feats, lens, **kw.get(fam, {}))
        assert a['enc'].dtype == torch.float32 and b['enc'].dtype == torch.float64 and b['probs'].dtype == torch.float64
        assert (a['enc'].double() - b['enc']).abs().max() < 1e-4, fam
        p32, *c32 = f64.chunk_run(fam, sd, feats, windows, torch.float32)
        p64, *c64 = f64.chunk_run(fam, sd, feats, windows, torch.float64)
        assert p64.dtype == torch.float64 and all(c.dtype == torch.float64 for c in c64)
        assert (p32.double() - p64).abs().max() < 1e-4, fam
        for x, y in zip(c32, c64):
            assert x.shape == y.shape and (x.double() - y).abs().max() < 1e-4, fam
    for bi in (False, True):                                          # the GRU cell against torch.nn.GRU (float64)
        sd = weights.deepspeech2_state_dict(0, 64, num_rnn_layers=1, bidirectional=bi, use_gru=True)
        r = f64.forward('deepspeech2', sd, feats, lens, torch.float64)
        sd64 = f64.cast_state_dict(sd, torch.float64)
        from oracle import deepspeech2 as ods
        x, xl = ods.conv_frontend(sd64, feats.double(), lens)
        p = 'encoder.rnns.0.rnn.rnn.'
        gru = torch.nn.GRU(x.shape[-1], sd[p + 'weight_hh_l0'].shape[1], batch_first=True, bidirectional=bi).double()
        gru.load_state_dict({k[len(p):]: v for k, v in sd64.items() if k.startswith(p)})
        with torch.no_grad():
            y, hn = gru(torch.nn.utils.rnn.pack_padded_sequence(x, xl, batch_first=True, enforce_sorted=False))
            y, _ = torch.nn.utils.rnn.pad_packed_sequence(y, batch_first=True)
            y = F.layer_norm(y, (y.shape[-1],), sd64['encoder.rnns.0.layer_norm.weight'], sd64['encoder.rnns.0.layer_norm.bias'], 1e-5)
        assert (y - r['enc']).abs().max() < 1e-12 and (hn - r['h'][0]).abs().max() < 1e-12
        assert torch.equal(r['h'], r['c'])


# ---- perturbed oracles ------------------------------------------------------------------------------------------------------
def _attention_mutant(drop_final_fill=False, short_pad_layer=None):
    """oracle.conformer._attention with one defect: the zero fill AFTER the softmax left out, or one key too few in the pad
    mask of one layer"""
    def attention(sd, p, x, pos_emb, key_mask, heads, cache=None):
        B, T, d = x.shape
        dk = d // heads
        q = F.linear(x, sd[p + '.linear_q.weight'], sd[p + '.linear_q.bias']).view(B, T, heads, dk)
        k = F.linear(x, sd[p + '.linear_k.weight'], sd[p + '.linear_k.bias']).view(B, T, heads, dk).transpose(1, 2)
        v = F.linear(x, sd[p + '.linear_v.weight'], sd[p + '.linear_v.bias']).view(B, T, heads, dk).transpose(1, 2)
        pp = F.linear(pos_emb, sd[p + '.linear_pos.weight']).view(1, -1, heads, dk).transpose(1, 2)
        qu = (q + sd[p + '.pos_bias_u']).transpose(1, 2)
        qv = (q + sd[p + '.pos_bias_v']).transpose(1, 2)
        scores = (qu @ k.transpose(-2, -1) + qv @ pp.transpose(-2, -1)) / math.sqrt(dk)
        if short_pad_layer is not None and p == f'encoder.encoders.{short_pad_layer}.self_attn':
            key_mask = key_mask.clone()
            last = key_mask.any(dim=1).long().sum(dim=-1) - 1                 # last kept key of every utterance
            key_mask[torch.arange(B), :, last] = False
        m = ~key_mask.unsqueeze(1)
        attn = torch.softmax(scores.masked_fill(m, -float('inf')), dim=-1)
        if not drop_final_fill:
            attn = attn.masked_fill(m, 0.0)
        o = (attn @ v).transpose(1, 2).reshape(B, T, d)
        return F.linear(o, sd[p + '.linear_out.weight'], sd[p + '.linear_out.bias']), None
    return attention


def _mutants(oc):
    """name -> {attribute of oracle.conformer: replacement}"""
    table = oc.positional_table

    def ln_eps(eps):
        return lambda sd, p, x: F.layer_norm(x, (x.shape[-1],), sd[p + '.weight'], sd[p + '.bias'], eps)

    def ffn_swish(sd, p, x):
        h = F.silu(F.linear(x, sd[p + '.w_1.weight'], sd[p + '.w_1.bias'])) * (1 + 1e-4)
        return F.linear(h, sd[p + '.w_2.weight'], sd[p + '.w_2.bias'])

    def table_shifted(max_len, d, dtype=torch.float32):
        pe = table(max_len, d, dtype).clone()
        pe[7] = pe[8]                                                        # one positional row shifted
        return pe
    return {'layernorm_eps_1e-6': {'_ln': ln_eps(1e-6)}, 'layernorm_eps_0': {'_ln': ln_eps(0.0)},
            'swish_rel_1e-4': {'_ffn': ffn_swish}, 'positional_row_shifted': {'positional_table': table_shifted},
            'pad_mask_one_key_short': {'_attention': _attention_mutant(short_pad_layer=0)}}


@contextlib.contextmanager
def patched(mod, repl):
    keep = {k: getattr(mod, k) for k in repl}
    for k, v in repl.items():
        setattr(mod, k, v)
    try:
        yield
    finally:
        for k, v in keep.items():
            setattr(mod, k, v)


@pytest.fixture(scope='module')
def truth(mods):
    """depth -> (sd, float32 result at 1 thread, float64 result, valid mask)"""
    oc, f64, _, weights, golden_inputs = mods
    feats, lens = golden_inputs()
    out = {}
    for depth in (1, 12):
        sd = weights.conformer_state_dict(0, 512, num_blocks=depth)
        with threads(1):
            r32 = f64.forward('conformer', sd, feats, lens, torch.float32)
        with threads(16):
            r64 = f64.forward('conformer', sd, feats, lens, torch.float64)
        out[depth] = (sd, r32, r64, budget.valid_mask(r64['enc'].shape, lens))
    return out


@pytest.mark.parametrize('depth', [1, 12])
@pytest.mark.parametrize('name', ['layernorm_eps_1e-6', 'layernorm_eps_0', 'swish_rel_1e-4', 'positional_row_shifted',
                                  'pad_mask_one_key_short'])
def test_perturbed_oracle_is_rejected(mods, truth, name, depth):
    oc, f64, _, _, golden_inputs = mods
    feats, lens = golden_inputs()
    sd, r32, r64, mask = truth[depth]
    with patched(oc, _mutants(oc)[name]), threads(1):
        bad = f64.forward('conformer', sd, feats, lens, torch.float32)
    fe = budget.evaluate(r64['enc'], r32['enc'], bad['enc'], mask)
    fp = budget.evaluate(r64['probs'], r32['probs'], bad['probs'], mask)
    print(budget.line(f'{name} depth {depth} enc', fe))
    print(budget.line(f'{name} depth {depth} probs', fp))
    assert not fe['ok'], f'{name} at depth {depth} passes the budget on enc: ' + budget.line('enc', fe)


@pytest.mark.parametrize('depth', [1, 12])
def test_softmax_without_the_final_zero_fill_is_the_same_function_here(mods, truth, depth):
    """``softmax(scores.masked_fill(m, -inf)).masked_fill(m, 0)`` without its last fill: a masked key already has weight
    exp(-inf) = 0 exactly, and no query row of these inputs has every key masked (a padded query still sees the valid keys of
    its utterance), so this 'defect' changes no bit and no rule can reject it -- shown here rather than assumed; the mask
    defect that must be rejected is ``pad_mask_one_key_short`` above."""
    oc, f64, _, _, golden_inputs = mods
    feats, lens = golden_inputs()
    sd, r32, _, _ = truth[depth]
    with patched(oc, {'_attention': _attention_mutant(drop_final_fill=True)}), threads(1):
        same = f64.forward('conformer', sd, feats, lens, torch.float32)
    assert torch.equal(same['enc'], r32['enc'])


@pytest.mark.parametrize('depth', [1, 12])
def test_other_thread_count_passes(mods, truth, depth):
    """the unperturbed float32 oracle with 16 threads instead of 1: another legitimate summation order"""
    oc, f64, _, _, golden_inputs = mods
    feats, lens = golden_inputs()
    sd, r32, r64, mask = truth[depth]
    with threads(16):
        other = f64.forward('conformer', sd, feats, lens, torch.float32)
    for key in ('enc', 'probs'):
        budget.check(f'threads 16 vs 1 depth {depth} {key}', r64[key], r32[key], other[key], mask)


def test_rule_arithmetic():
    t = np.zeros((1, 4, 2))
    t[0, 0, 0] = 4.0
    ref = t + 1e-6
    m = budget.valid_mask(t.shape, [9])                          # 4 * t < 9: frames 0, 1, 2
    assert m.tolist() == [[True, True, True, False]]
    bad = t.copy()
    bad[0, 3] = 1.0                                              # a padded frame is not looked at
    assert budget.evaluate(t, ref, bad, m)['ok']
    bad[0, 2, 1] = 8.1e-6
    f = budget.evaluate(t, ref, bad, m)
    assert not f['ok'] and abs(f['bar_max'] - 8e-6) < 1e-12
    one = np.zeros_like(t)
    one[0, 1, 1] = 1.0
    f = budget.evaluate(t, t, t + 2e-6 * one, m)                 # exact reference: the ulp floor carries both bars
    assert f['ulp_floor'] == 4.0 * 2.0 ** -23 and f['ok'] and abs(f['bar_rms'] - 2 * f['ulp_floor']) < 1e-15
    assert not budget.evaluate(t, t, t + 4e-6 * one, m)['ok']    # 8 ulp = 3.8e-6
    assert not budget.evaluate(t, t, t + 1e-6, m)['ok']          # under the max bar everywhere, over the rms bar (2 ulp = 9.5e-7)
    bad = t.copy()
    bad[0, 0, 0] = np.nan
    assert not budget.evaluate(t, ref, bad, m)['ok']


# ---- stress checkpoints: conditions on the oracle alone ---------------------------------------------------------------------
STRESS_LEVELS = [(3, 4, 4), (6, 8, 8)]


@pytest.mark.parametrize('depth', [1, 2])
@pytest.mark.parametrize('level', STRESS_LEVELS)
def test_stress_checkpoints_keep_the_oracle_finite_and_decided(mods, level, depth):
    oc, f64, _, weights, golden_inputs = mods
    feats, lens = golden_inputs()
    sd = budget.stress_state_dict(weights.conformer_state_dict(0, 512, num_blocks=depth), *level)
    r32, r64 = f64.both('conformer', sd, feats, lens)
    for key in ('enc', 'logits', 'probs'):
        assert torch.isfinite(r32[key]).all() and torch.isfinite(r64[key]).all(), key
    mask = budget.valid_mask(r64['enc'].shape, lens)
    e_ref = np.abs(budget.as64(r32['probs']) - budget.as64(r64['probs']))[mask].max()
    assert e_ref < 2e-3, e_ref
    decided = budget.argmax_margin(r64['probs'], e_ref)[mask]
    print(f'stress {level} depth {depth}: |logit| <= {r64["logits"].abs().max():.1f}, probs e_ref {e_ref:.2e}, '
          f'undecided {100 * (1 - decided.mean()):.2f} %')
    assert 1 - decided.mean() <= 0.02
    assert (budget.as64(r32['probs']).argmax(-1)[mask][decided] == budget.as64(r64['probs']).argmax(-1)[mask][decided]).all()
