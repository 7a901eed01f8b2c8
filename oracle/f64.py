"""TEST INFRASTRUCTURE ONLY -- the oracle restatements evaluated in a chosen dtype.

The restatements under ``oracle/`` take their dtype from the ``state_dict`` and the inputs, so the same functions give the
float32 reference (what the parity tests compare with) and, on a float64 copy of the checkpoint, the truth both the
reference and the kernels are measured against (``tests/budget.py``)."""
import torch
import torch.nn.functional as F

FAMILIES = ('conformer', 'squeezeformer', 'efficient_conformer', 'deepspeech2')


def cast_state_dict(sd, dtype):
    """floating-point entries of a checkpoint in ``dtype`` (a float32 -> float64 cast is exact)"""
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}


def module_of(family):
    from oracle import conformer, deepspeech2, efficient_conformer, squeezeformer
    return {'conformer': conformer, 'squeezeformer': squeezeformer, 'efficient_conformer': efficient_conformer,
            'deepspeech2': deepspeech2}[family]


@torch.no_grad()
def forward(family, sd, feats, lens, dtype=torch.float32, encoder_fn=None, **kw):
    """full-context forward of one family in ``dtype`` -> {'enc', 'logits', 'probs'} (DeepSpeech2: + 'h', 'c', 'lens');
    ``encoder_fn(sd, feats, lens, **kw)`` replaces the family's ``encoder_full`` (a restatement kept elsewhere, or a
    deliberately perturbed one)"""
    sd = cast_state_dict(sd, dtype)
    feats = torch.as_tensor(feats).to(dtype)
    lens = torch.as_tensor(lens).long()
    m = module_of(family)
    out = {}
    if family == 'deepspeech2':
        enc, xl, h, c = m.encoder(sd, feats, lens, **kw)
        out.update(h=h, c=c, lens=xl)
        head = 'decoder.ctc_lo'
    else:
        enc = (encoder_fn or m.encoder_full)(sd, feats, lens, **kw)
        head = 'ctc.ctc_lo'
    out['enc'] = enc
    out['logits'] = F.linear(enc, sd[head + '.weight'], sd[head + '.bias'])
    out['probs'] = torch.softmax(out['logits'], dim=2)
    return out


def both(family, sd, feats, lens, **kw):
    """(float32 result, float64 result) of ``forward``"""
    return forward(family, sd, feats, lens, torch.float32, **kw), forward(family, sd, feats, lens, torch.float64, **kw)


def both_chunks(family, sd, feats, windows, **kw):
    """(float32 result, float64 result) of ``chunk_run``"""
    return chunk_run(family, sd, feats, windows, torch.float32, **kw), chunk_run(family, sd, feats, windows, torch.float64, **kw)


@torch.no_grad()
def chunk_run(family, sd, feats, windows, dtype=torch.float32, required_cache_size=-16, **kw):
    """chunked streaming of one utterance (feats [1, T, n_mels]) over ``windows`` = [(first frame, frames), ...] in ``dtype``
    -> (probabilities of all chunks concatenated [T', V], att_cache, cnn_cache); DeepSpeech2: (probs, h, c).  ``kw`` goes to the
    family's ``get_encoder_out_chunk`` (the layer layout, the kernel size)"""
    sd = cast_state_dict(sd, dtype)
    feats = torch.as_tensor(feats).to(dtype)
    m = module_of(family)
    a = torch.zeros(0, 0, 0, 0, dtype=dtype)
    b = torch.zeros(0, 0, 0, 0, dtype=dtype)
    off, outs = 0, []
    for cur, n in windows:
        x = feats[:1, cur:cur + n]
        if family == 'deepspeech2':
            p, _, a, b = m.get_encoder_out_chunk(sd, x, torch.tensor([x.shape[1]]), a, b, **kw)
        else:
            p, a, b = m.get_encoder_out_chunk(sd, x, off, required_cache_size, a, b, **kw)
        off += p.shape[1]
        outs.append(p[0])
    return torch.cat(outs), a, b
