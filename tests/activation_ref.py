"""The Conformer forward with ``encoder_conf.activation_type`` as an argument (a helper module: tests and
tools/make_activation_golden.py import it; it never calls the code under test).

oracle/conformer.py states the shipped variant, Swish, and stays as it is.  This module restates the full-context forward and the
chunk step around the two places where the reference uses the activation (conformer/encoder.py ``positionwise_layer_args`` and
``convolution_layer_args``): the hidden activation of both PositionwiseFeedForward modules and the activation behind the conv
module's norm.  The GLU keeps its sigmoid.  Everything the activation does not touch -- the front end, LayerNorm, the
relative-position attention, the positional table -- is oracle.conformer's own function, so ``act='swish'`` gives its bits.

    ACTS[name](x)      torch's defaults, like the reference's ``get_activation`` (utils/common.py:143-154): nn.Hardtanh() on
                       [-1, 1], nn.Tanh, nn.ReLU, nn.SELU, Swish = x * sigmoid(x), erf-exact nn.GELU

Generic in dtype (float64 on a float64 checkpoint: the truth of tests/budget.py).  ``encoder_full`` is usable as the
``encoder_fn`` of ``oracle.f64.forward`` / ``both``; ``chunk_run`` / ``both_chunks`` have the shape of ``oracle.f64.chunk_run``.
``pos_enc`` 'abs_pos' (plain MultiHeadedAttention, ``x * sqrt(d) + pe[offset + t]``, conformer/embedding.py:52-54) and
``input_layer`` 'conv2d6' (subsampling.py:115-156) serve the cases that combine an activation with those keys."""
import math

import torch
import torch.nn.functional as F

from oracle import conformer as oc
from oracle.f64 import cast_state_dict

ACTS = {
    'swish': F.silu,
    'relu': F.relu,
    'gelu': F.gelu,                   # approximate='none'
    'tanh': torch.tanh,
    'hardtanh': F.hardtanh,           # min_val = -1, max_val = 1
    'selu': F.selu,                   # scale 1.0507009873554805, alpha 1.6732632423543772
}
NEW = ('relu', 'gelu', 'tanh', 'hardtanh', 'selu')


def _ffn(sd, p, x, act):
    """conformer/positionwise.py:30-37: w_2(activation(w_1(x)))"""
    h = ACTS[act](F.linear(x, sd[p + '.w_1.weight'], sd[p + '.w_1.bias']))
    return F.linear(h, sd[p + '.w_2.weight'], sd[p + '.w_2.bias'])


def _plain_attention(sd, p, x, key_mask, heads, cache=None):
    """MultiHeadedAttention.forward (conformer/attention.py:133-167): oracle.conformer._attention without the positional term"""
    B, T, d = x.shape
    dk = d // heads
    q = F.linear(x, sd[p + '.linear_q.weight'], sd[p + '.linear_q.bias']).view(B, T, heads, dk).transpose(1, 2)
    k = F.linear(x, sd[p + '.linear_k.weight'], sd[p + '.linear_k.bias']).view(B, T, heads, dk).transpose(1, 2)
    v = F.linear(x, sd[p + '.linear_v.weight'], sd[p + '.linear_v.bias']).view(B, T, heads, dk).transpose(1, 2)
    if cache is not None and cache.shape[2] > 0:
        k = torch.cat([cache[..., :dk], k], dim=2)
        v = torch.cat([cache[..., dk:], v], dim=2)
    new_cache = torch.cat([k, v], dim=-1)
    scores = q @ k.transpose(-2, -1) / math.sqrt(dk)
    if key_mask is not None:
        m = ~key_mask.unsqueeze(1)
        scores = scores.masked_fill(m, -float('inf'))
        attn = torch.softmax(scores, dim=-1).masked_fill(m, 0.0)
    else:
        attn = torch.softmax(scores, dim=-1)
    o = (attn @ v).transpose(1, 2).reshape(B, T, d)
    return F.linear(o, sd[p + '.linear_out.weight'], sd[p + '.linear_out.bias']), new_cache


def _conv_module(sd, p, x, pad_mask, kernel, act, cache=None, causal=True):
    """ConvolutionModule.forward with layer_norm (conformer/convolution.py:76-132): oracle.conformer._conv_module with the
    activation behind the norm as an argument"""
    x = x.transpose(1, 2)
    if pad_mask is not None:
        x = x.masked_fill(~pad_mask.unsqueeze(1), 0.0)
    lorder = kernel - 1
    new_cache = None
    if causal:
        if cache is None or cache.shape[2] == 0:
            x = F.pad(x, (lorder, 0))
        else:
            x = torch.cat([cache, x], dim=2)
        new_cache = x[:, :, -lorder:]
    x = F.conv1d(x, sd[p + '.pointwise_conv1.weight'], sd[p + '.pointwise_conv1.bias'])
    x = F.glu(x, dim=1)
    x = F.conv1d(x, sd[p + '.depthwise_conv.weight'], sd[p + '.depthwise_conv.bias'], groups=x.shape[1],
                 padding=0 if causal else lorder // 2)
    x = ACTS[act](oc._ln(sd, p + '.norm', x.transpose(1, 2))).transpose(1, 2)
    x = F.conv1d(x, sd[p + '.pointwise_conv2.weight'], sd[p + '.pointwise_conv2.bias'])
    if pad_mask is not None:
        x = x.masked_fill(~pad_mask.unsqueeze(1), 0.0)
    return x.transpose(1, 2), new_cache


def _layer(sd, i, x, pos_emb, att_mask, pad_mask, heads, kernel, act, att_cache=None, cnn_cache=None, causal=True):
    """ConformerEncoderLayer.forward (conformer/encoder.py:82-163); pos_emb None: plain attention"""
    p = f'encoder.encoders.{i}'
    x = x + 0.5 * _ffn(sd, p + '.feed_forward_macaron', oc._ln(sd, p + '.norm_ff_macaron', x), act)
    h = oc._ln(sd, p + '.norm_mha', x)
    if pos_emb is None:
        a, new_att = _plain_attention(sd, p + '.self_attn', h, att_mask, heads, att_cache)
    else:
        a, new_att = oc._attention(sd, p + '.self_attn', h, pos_emb, att_mask, heads, att_cache)
    x = x + a
    c, new_cnn = _conv_module(sd, p + '.conv_module', oc._ln(sd, p + '.norm_conv', x), pad_mask, kernel, act, cnn_cache, causal)
    x = x + c
    x = x + 0.5 * _ffn(sd, p + '.feed_forward', oc._ln(sd, p + '.norm_ff', x), act)
    return oc._ln(sd, p + '.norm_final', x), new_att, new_cnn


def _embed(sd, feats, input_layer):
    if input_layer == 'conv2d':
        return oc.embed(sd, feats)
    assert input_layer == 'conv2d6', input_layer
    x = ((feats - sd['encoder.global_cmvn.mean']) * sd['encoder.global_cmvn.istd']).unsqueeze(1)
    x = F.relu(F.conv2d(x, sd['encoder.embed.conv.0.weight'], sd['encoder.embed.conv.0.bias'], stride=2))
    x = F.relu(F.conv2d(x, sd['encoder.embed.conv.2.weight'], sd['encoder.embed.conv.2.bias'], stride=3))
    b, c, t, f = x.shape
    x = F.linear(x.transpose(1, 2).reshape(b, t, c * f), sd['encoder.embed.linear.weight'], sd['encoder.embed.linear.bias'])
    return x * math.sqrt(x.shape[-1])


def encoder_full(sd, feats, lens, act='swish', decoding_chunk_size=-1, heads=4, kernel=15, streaming=True, pos_enc='rel_pos',
                 input_layer='conv2d'):
    """ConformerEncoder.forward (conformer/encoder.py:305-346): oracle.conformer.encoder_full with the activation"""
    if not streaming:
        decoding_chunk_size = -1
    B, T, _ = feats.shape
    pad = torch.arange(T)[None, :] < lens[:, None]
    x = _embed(sd, feats, input_layer)
    Tp = x.shape[1]
    pad_s = pad[:, :-2:2][:, :-2:2] if input_layer == 'conv2d' else pad[:, :-2:2][:, :-4:3]
    pe = oc.positional_table(5000, x.shape[-1], x.dtype)[:Tp].unsqueeze(0)
    if pos_enc == 'abs_pos':
        x, pe = x + pe, None
    else:
        assert pos_enc == 'rel_pos', pos_enc
    idx = torch.arange(Tp)
    if decoding_chunk_size < 0:
        chunk = torch.ones(Tp, Tp, dtype=torch.bool)
    else:
        chunk = idx[None, :] < ((idx[:, None] // decoding_chunk_size + 1) * decoding_chunk_size)
    att_mask = pad_s[:, None, :] & chunk[None]
    for i in range(oc.num_blocks_of(sd)):
        x, _, _ = _layer(sd, i, x, pe, att_mask, pad_s, heads, kernel, act, causal=streaming)
    return oc._ln(sd, 'encoder.after_norm', x)


def get_encoder_out(sd, feats, lens, act='swish', **kw):
    return oc.ctc_probs(sd, encoder_full(sd, feats, lens, act=act, decoding_chunk_size=-1, **kw))


def get_encoder_out_chunk(sd, feats, offset, required_cache_size, att_cache, cnn_cache, act='swish', heads=4, kernel=15):
    """ConformerModel.get_encoder_out_chunk (conformer/model.py:169-190, rel_pos): oracle.conformer's with the activation"""
    assert feats.shape[0] == 1
    x = oc.embed(sd, feats)
    have = att_cache.numel() > 0
    cache_t1 = att_cache.shape[2] if have else 0
    key_size = cache_t1 + x.shape[1]
    pos_emb = oc.positional_table(5000, x.shape[-1], x.dtype)[offset - cache_t1: offset - cache_t1 + key_size].unsqueeze(0)
    if required_cache_size < 0:
        start = 0
    elif required_cache_size == 0:
        start = key_size
    else:
        start = max(key_size - required_cache_size, 0)
    r_att, r_cnn = [], []
    for i in range(oc.num_blocks_of(sd)):
        x, na, nc = _layer(sd, i, x, pos_emb, None, None, heads, kernel, act, att_cache[i:i + 1] if have else None,
                           cnn_cache[i] if cnn_cache.numel() > 0 else None)
        r_att.append(na[:, :, start:, :])
        r_cnn.append(nc)
    x = oc._ln(sd, 'encoder.after_norm', x)
    return oc.ctc_probs(sd, x), torch.cat(r_att, dim=0), torch.stack(r_cnn, dim=0)


@torch.no_grad()
def chunk_run(sd, feats, windows, act, dtype=torch.float32, required_cache_size=-16, **kw):
    """oracle.f64.chunk_run for this module: one utterance (feats [1, T, n_mels]) over ``windows`` = [(first frame, frames), ...]
    in ``dtype`` -> (probabilities of all chunks concatenated [T', V], att_cache, cnn_cache)"""
    sd = cast_state_dict(sd, dtype)
    feats = torch.as_tensor(feats).to(dtype)
    a = torch.zeros(0, 0, 0, 0, dtype=dtype)
    b = torch.zeros(0, 0, 0, 0, dtype=dtype)
    off, outs = 0, []
    for cur, n in windows:
        p, a, b = get_encoder_out_chunk(sd, feats[:1, cur:cur + n], off, required_cache_size, a, b, act=act, **kw)
        off += p.shape[1]
        outs.append(p[0])
    return torch.cat(outs), a, b


def both_chunks(sd, feats, windows, act, **kw):
    """(float32 result, float64 result) of ``chunk_run``"""
    return chunk_run(sd, feats, windows, act, torch.float32, **kw), chunk_run(sd, feats, windows, act, torch.float64, **kw)
