"""The error budget of the float64 parity tests, written once (a plain helper module: tests import it).

For an output with float64 truth ``y64`` (the oracle evaluated in float64, oracle/f64.py), float32 CPU reference ``y32`` (the
same oracle in float32) and candidate ``y`` (the HIP path), over the valid frames only:

    e_ref = y32 - y64        e = y - y64
    max|e| <= C * max(max|e_ref|, ulp_floor)      and      rms(e) <= C * max(rms(e_ref), ulp_floor / 4)

``ulp_floor`` = 2^-23 * max|y64|: one float32 ulp of the largest output, so that a reference that happens to land on the
truth does not ask the impossible.  C = 8 is an allowance for a different, equally legitimate float32 evaluation: the CPU
GEMMs accumulate in 8 / 16-lane partial sums while an MFMA chain is sequential over K / 2 steps (random-walk ratio about
sqrt(8) = 2.8), and the device's fast exp + rcp in the gated epilogues are 1-2 ulp against libm (about a factor 2).  It is
derived from the reference side only and is NOT tuned to what the kernels reach; a case that needs more carries its own
allowance next to the case, with the cause written beside it."""
import numpy as np
import torch

C = 8.0
ULP32 = 2.0 ** -23


def as64(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def valid_mask(shape, lens, rate=4, counts=None):
    """bool [B, T'] : frame t of utterance b is valid iff rate * t < lens[b] (the ``valid_frames`` convention of
    tests/test_gpu_parity.py), or t < counts[b] when the valid frame counts are given directly"""
    B, T = shape[0], shape[1]
    if counts is None:
        counts = [-(-int(l) // rate) for l in lens]
    m = np.zeros((B, T), bool)
    for b in range(B):
        m[b, :min(T, int(counts[b]))] = True
    return m


def _sel(a, mask):
    a = as64(a)
    return a if mask is None else a[np.asarray(mask, bool)]


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0


def evaluate(y64, y32, y, mask=None, c=C, c_max=None):
    """the figures of the rule and whether ``y`` holds it; shapes must agree (a mask selects leading [B, T'] positions).
    ``c_max``: a case's own allowance on the max criterion (the rms criterion keeps ``c``)"""
    c_max = c if c_max is None else c_max
    t, r, g = _sel(y64, mask), _sel(y32, mask), _sel(y, mask)
    assert t.shape == r.shape == g.shape, (t.shape, r.shape, g.shape)
    finite = bool(np.isfinite(g).all())
    e_ref, e = r - t, g - t
    floor = ULP32 * float(np.abs(t).max()) if t.size else 0.0
    f = {'max_ref': float(np.abs(e_ref).max()), 'rms_ref': rms(e_ref), 'max': float(np.abs(e).max()) if finite else float('inf'),
         'rms': rms(e) if finite else float('inf'), 'ulp_floor': floor, 'c': float(c_max)}
    f['bar_max'] = c_max * max(f['max_ref'], floor)
    f['bar_rms'] = c * max(f['rms_ref'], floor / 4)
    f['ratio_max'] = f['max'] / max(f['max_ref'], floor)
    f['ratio_rms'] = f['rms'] / max(f['rms_ref'], floor / 4)
    f['ok'] = finite and f['max'] <= f['bar_max'] and f['rms'] <= f['bar_rms']
    return f


def line(name, f):
    return (f'BUDGET {name}: max {f["max"]:.3e} (ref {f["max_ref"]:.3e}, x{f["ratio_max"]:.2f})  rms {f["rms"]:.3e} '
            f'(ref {f["rms_ref"]:.3e}, x{f["ratio_rms"]:.2f})  floor {f["ulp_floor"]:.2e}  C {f["c"]:g}')


def check(name, y64, y32, y, mask=None, c=C, c_max=None):
    """print the figures of one case, then assert the rule (``c_max``: the case's own allowance on the max criterion)"""
    f = evaluate(y64, y32, y, mask, c, c_max)
    print(line(name, f), flush=True)
    assert f['ok'], 'over budget -- ' + line(name, f)
    return f


# ---- stress checkpoints -----------------------------------------------------------------------------------------------------
def stress_state_dict(sd, g_att, g_act, g_ctc, ln_shift=2.0):
    """a copy of a synthetic Conformer-family checkpoint with raised gains: q / k projections x g_att (score spread grows with
    g_att^2), ``w_1`` and ``pointwise_conv1`` x g_act (Swish / GLU gates at |v| of tens), the CTC head x g_ctc (logits towards
    the float32 exp range), and the LayerNorm biases in front of those projections shifted by ``ln_shift`` so that the
    normalised rows they read have a large mean.  Everything stays finite by construction (finite gains on finite weights)."""
    out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
    for k, v in out.items():
        if not torch.is_tensor(v) or not v.is_floating_point():
            continue
        if k.endswith(('linear_q.weight', 'linear_q.bias', 'linear_k.weight', 'linear_k.bias')):
            v.mul_(g_att)
        elif '.w_1.' in k or '.pointwise_conv1.' in k:
            v.mul_(g_act)
        elif k.startswith('ctc.ctc_lo.'):
            v.mul_(g_ctc)
        elif k.endswith(('norm_ff.bias', 'norm_ff_macaron.bias', 'norm_mha.bias', 'norm_conv.bias')):
            v.add_(ln_shift)
    return out


def argmax_margin(p64, e_ref_max, c=C):
    """frames whose float64 top-2 margin exceeds 2 * c * max|e_ref| (bool, shape of p64 without the last axis)"""
    p = np.sort(as64(p64), axis=-1)
    return (p[..., -1] - p[..., -2]) > 2 * c * e_ref_max
