"""TEST INFRASTRUCTURE ONLY -- record the float32 outputs of the four oracle families on ``golden_inputs()`` as SHA-256
digests (``tests/golden/oracle_f32_pin.json``):  ``python -m oracle.make_f32_pin``.

The file was written once, from the commit BEFORE the restatements became dtype-generic; ``tests/test_f64_budget_cpu.py``
recomputes the digests and so shows that the float32 path still runs the same operations in the same order.  One CPU thread:
the summation order of the CPU GEMMs depends on the thread count."""
import hashlib
import json
import os

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'oracle_f32_pin.json')


def digest(t):
    a = np.ascontiguousarray(t.detach().numpy())
    return hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def cases():
    """name -> (family, state dict, forward keywords)"""
    from oracle import weights
    return {
        'conformer': ('conformer', weights.conformer_state_dict(0, 512), {}),
        'conformer_chunk16': ('conformer', weights.conformer_state_dict(0, 512), {'decoding_chunk_size': 16}),
        'squeezeformer': ('squeezeformer', weights.squeezeformer_state_dict(0, 512), {}),
        'efficient_conformer': ('efficient_conformer', weights.efficient_conformer_state_dict(0, 512), {}),
        'deepspeech2_uni': ('deepspeech2', weights.deepspeech2_state_dict(0, 300, bidirectional=False), {}),
        'deepspeech2_bi': ('deepspeech2', weights.deepspeech2_state_dict(0, 300, bidirectional=True), {}),
    }


def compute():
    from oracle import f64
    from oracle.make_golden import golden_inputs
    feats, lens = golden_inputs()
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = {}
        for name, (family, sd, kw) in cases().items():
            r = f64.forward(family, sd, feats, lens, torch.float32, **kw)
            out[name] = {k: digest(r[k]) for k in ('enc', 'probs')}
    finally:
        torch.set_num_threads(n)
    return out


def environment():
    return {'torch': torch.__version__, 'cpu_capability': torch.backends.cpu.get_cpu_capability()}


if __name__ == '__main__':
    rec = {'environment': environment(), 'digests': compute()}
    with open(OUT, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(rec, indent=1, sort_keys=True))
