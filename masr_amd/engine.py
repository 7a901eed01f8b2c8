"""Python handle on the HIP engine (libmasr_hip.so).  torch is used only for device memory,
streams and host<->device copies; all arithmetic of the hot path runs in the HIP kernels."""
import contextlib
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import MasrConfig, check
from .pinned import PinnedRing


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def positional_table(max_len, d):
    """Same torch ops as the reference (conformer/embedding.py:31-37) -> bit-identical table."""
    pe = torch.zeros(max_len, d)
    pos = torch.arange(0, max_len, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe


# encoder_conf.input_layer -> masr_config.reserved[3] (include/masr_hip.h): Conv2dSubsampling4 / 6 / 8 (conformer/subsampling.py)
INPUT_LAYERS = {'conv2d': 0, 'conv2d6': 1, 'conv2d8': 2}
# the fewest feature frames that give one encoder frame
MIN_FRAMES = {'conv2d': 7, 'conv2d6': 11, 'conv2d8': 15}


def subsampled_len(t, input_layer='conv2d'):
    """encoder frames for t feature frames (int, array or tensor): conv1 3x3 stride 2, then 3x3 stride 2 (conv2d), 5x5 stride 3
    (conv2d6) or 3x3 stride 2 twice (conv2d8), none padded.  Below the minimum the result is <= 0."""
    t1 = (t - 1) // 2
    if input_layer == 'conv2d6':
        return (t1 - 2) // 3
    if input_layer == 'conv2d8':
        return ((t1 - 1) // 2 - 1) // 2
    return (t1 - 1) // 2


def reference_gains_scalar(mean_square, target_db, max_gain_db=300.0):
    """float32 mean squares [B] -> linear gains [B] with the reference's own scalar expressions, verbatim in numpy on this host:
    ``rms_db = 10 * np.log10(mean_square)`` (audio.py:524-529), ``gain = target_db - rms_db`` and the max_gain_db check
    (:300-304), ``samples *= 10. ** (gain / 20.)`` (:256-264).  A zero mean square (digital silence) counts as 1, like the
    reference's ``rms_db`` -- the gain is then just target_dB and nothing raises; a NaN mean square (NaN samples in the input) is
    NOT special-cased there either: it propagates into the gain, and the transcript of that utterance is whatever NaN features
    decode to, as in the reference."""
    out = np.empty(len(mean_square), np.float32)
    for i, ms in enumerate(np.asarray(mean_square, np.float32)):
        if ms == 0:
            ms = 1
        rms_db = 10 * np.log10(ms)
        gain = target_db - rms_db
        if gain > max_gain_db:
            raise ValueError(f"无法将段规范化到{target_db}dB，音频增益{gain}增益已经超过max_gain_db ({max_gain_db}dB)")
        out[i] = 10. ** (min(max_gain_db, gain) / 20.)
    return out


def reference_gains(mean_square, target_db, max_gain_db=300.0):
    """``reference_gains_scalar`` for a whole batch.  The two transcendental steps -- ``np.log10(mean_square)`` and
    ``10. ** (gain / 20.)`` -- are evaluated element by element on numpy float32 SCALARS, exactly as the reference evaluates them:
    numpy's float32 ARRAY loops of log10 / power are SIMD routines (SVML on AVX-512 hosts) whose last bit differs from the scalar
    libm path on some arguments -- measured on the GPU box's EPYC 9575F: 1 of 32 gains, 273 int16 samples of that utterance off by
    one LSB.  The products, differences and quotients in between are IEEE-exact float32 operations (identical in any loop) and
    run as array operations.  128 streams: ~0.15 ms per pool step."""
    ms = np.asarray(mean_square, np.float32)
    if len(ms) <= 2 or not isinstance(target_db, (int, float)) or np.float32(target_db) != target_db:
        return reference_gains_scalar(ms, target_db, max_gain_db)     # one utterance (predict): 3 us; or a target that float32
                                                                      # does not hold: the long way
    silent = ms == 0
    lg = np.array([np.log10(x) for x in np.where(silent, np.float32(1), ms).astype(np.float32)], np.float32)
    gain = np.float32(target_db) - np.float32(10) * lg
    if (gain > max_gain_db).any():
        g = gain[gain > max_gain_db][0]
        raise ValueError(f"无法将段规范化到{target_db}dB，音频增益{g}增益已经超过max_gain_db ({max_gain_db}dB)")
    out = np.array([10. ** (x / 20.) for x in gain], np.float32)
    if silent.any():
        # digital silence: the scalar code sets ``ms = 1`` -- a Python int, so its logarithm, the gain and the power are evaluated in
        # float64 and rounded once
        out[silent] = np.float32(10. ** (min(max_gain_db, target_db - 10 * np.log10(1)) / 20.))
    return out


# encoder_conf.pos_enc_layer_type -> masr_config.reserved[2] of the Conformer (include/masr_hip.h; conformer/encoder.py:239-281)
POS_ENC_LAYER_TYPES = {'rel_pos': 0, 'abs_pos': 1, 'no_pos': 2}
# what only RelPositionMultiHeadedAttention owns: a checkpoint has all three per layer (rel_pos) or none (abs_pos / no_pos)
REL_POS_KEYS = ('self_attn.linear_pos.weight', 'self_attn.pos_bias_u', 'self_attn.pos_bias_v')


def _validate_pos_enc(use_model, enc, state_dict):
    """``encoder_conf.pos_enc_layer_type``: rel_pos for every family; the Conformer also abs_pos (sinusoid rows added to the scaled
    embedding, plain attention) and no_pos (plain attention, nothing added).  Config and checkpoint have to agree in both
    directions: only a rel_pos checkpoint holds ``linear_pos`` / ``pos_bias_u`` / ``pos_bias_v``."""
    v = enc.get('pos_enc_layer_type', 'rel_pos')
    if use_model != 'conformer':
        if v != 'rel_pos':
            raise _lib.MasrError(f'{use_model}: encoder_conf.pos_enc_layer_type={v!r} is not implemented for the {use_model} '
                                 f"(supported: ('rel_pos',); abs_pos / no_pos run for the conformer only)")
        return
    if not isinstance(v, str) or v not in POS_ENC_LAYER_TYPES:
        raise _lib.MasrError(f'{use_model}: encoder_conf.pos_enc_layer_type={v!r} is not implemented '
                             f'(supported: {tuple(POS_ENC_LAYER_TYPES)})')
    if state_dict is None:
        return
    for key in (f'encoder.encoders.0.{k}' for k in REL_POS_KEYS):
        if v == 'rel_pos' and key not in state_dict:
            raise _lib.MasrError(f'{use_model}: encoder_conf.pos_enc_layer_type={v!r} but the checkpoint has no {key} '
                                 f'(it was trained with abs_pos or no_pos)')
        if v != 'rel_pos' and key in state_dict:
            raise _lib.MasrError(f'{use_model}: encoder_conf.pos_enc_layer_type={v!r} but the checkpoint holds {key} '
                                 f'(it was trained with rel_pos)')


# encoder_conf.activation_type -> masr_config.reserved[4] of the Conformer (include/masr_hip.h; get_activation of the reference's
# model_utils/utils/common.py): torch's defaults, i.e. erf-exact GELU, Hardtanh on [-1, 1], SELU with its own scale and alpha
ACTIVATION_TYPES = {'swish': 0, 'relu': 1, 'gelu': 2, 'tanh': 3, 'hardtanh': 4, 'selu': 5}


def _validate_activation(use_model, enc):
    """``encoder_conf.activation_type``: the hidden activation of both feed-forward modules and the one behind the conv module's
    norm (the GLU keeps its sigmoid).  ``swish`` for every family; the Conformer also the other five of the reference's
    ``get_activation``, on the width-generic layer (csrc/wide.hip), which carries layer_norm only.  An activation has no weights:
    nothing in a checkpoint can confirm the value, so a wrong one loads cleanly into the wrong arithmetic."""
    v = enc.get('activation_type', 'swish')
    if not isinstance(v, str) or v not in ACTIVATION_TYPES:
        raise _lib.MasrError(f'{use_model}: encoder_conf.activation_type={v!r} is not implemented '
                             f'(supported: {tuple(ACTIVATION_TYPES)} for the conformer, swish for the other families)')
    if v == 'swish':
        return
    if use_model != 'conformer':
        raise _lib.MasrError(f'{use_model}: encoder_conf.activation_type={v!r} is not implemented for the {use_model} '
                             f"(supported: ('swish',); the other activations run for the conformer only)")
    if enc.get('cnn_module_norm', 'layer_norm') == 'batch_norm':
        raise _lib.MasrError(f"conformer: encoder_conf.activation_type={v!r} with encoder_conf.cnn_module_norm='batch_norm' is not "
                             f'implemented (batch_norm runs with swish only: the width-generic layer carries layer_norm)')


CNN_KERNEL_DEFAULT = {'conformer': 15, 'efficient_conformer': 15, 'squeezeformer': 31}
CNN_KERNEL_MIN, CNN_KERNEL_MAX = 3, 31


def _validate_cnn_kernel(use_model, enc, state_dict, streaming):
    """``encoder_conf.cnn_module_kernel`` (masr_create repeats the range and parity checks): every integer from 3 to 31 on a
    ``streaming: True`` build, the odd ones on a ``streaming: False`` build (the symmetric padding is ``(K - 1) / 2`` frames on each
    side; the reference asserts it), 15 only for the Efficient Conformer (its stride layer halves the kernel).  ``streaming=None``:
    not known, the parity check is skipped.  The value has to be the checkpoint's own."""
    k = enc.get('cnn_module_kernel', CNN_KERNEL_DEFAULT.get(use_model, 15))
    head = f'{use_model}: encoder_conf.cnn_module_kernel={k!r} is not supported: '
    if use_model == 'efficient_conformer':
        if isinstance(k, bool) or not isinstance(k, int) or k != 15:
            raise _lib.MasrError(head + '15 only (the stride layer halves the kernel: the kernels are built around 15 / 7)')
    else:
        accepted = (f'an integer from {CNN_KERNEL_MIN} to {CNN_KERNEL_MAX} with streaming: True, an odd one with streaming: False')
        if isinstance(k, bool) or not isinstance(k, int) or not CNN_KERNEL_MIN <= k <= CNN_KERNEL_MAX:
            raise _lib.MasrError(head + accepted)
        if streaming is not None and not streaming and k % 2 == 0:
            raise _lib.MasrError(head + f'streaming: False pads (K - 1) / 2 frames on each side ({accepted})')
    key = 'encoder.encoders.0.conv_module.depthwise_conv.weight'
    if state_dict is not None and key in state_dict:
        have = int(state_dict[key].shape[-1])
        if have != k:
            raise _lib.MasrError(f'{use_model}: encoder_conf.cnn_module_kernel={k} but the checkpoint was trained with '
                                 f'cnn_module_kernel={have} ({key} is {list(state_dict[key].shape)})')


def _layer_layout(use_model, enc):
    """The layer positions a checkpoint's YAML sets, checked as masr_create checks them (include/masr_hip.h, ``reserved[5]``) and
    returned as that call takes them: Squeezeformer ``(reduce_idx, recover_idx)`` with -1 for null, Efficient Conformer
    ``(stride_layer_idx, len(group_layer_idx))``.  L = ``num_blocks``.

    Squeezeformer: ``reduce_idx`` null or a layer in [0, L); with it set, ``recover_idx`` a layer in [reduce_idx, L).  The reference
    fails on ``recover_idx < reduce_idx`` (an empty stack) and keeps HALF the frame rate to the end with ``recover_idx`` null or
    >= L: the engine's output is at the input frame rate everywhere, so those are refused by name rather than run.  With
    ``reduce_idx`` null the reference ignores ``recover_idx``, and so does this.
    Efficient Conformer: one stride-2 layer in [0, L) and 0 .. stride_layer_idx + 1 leading grouped layers."""
    def index(key, v):
        if isinstance(v, bool) or not isinstance(v, int):
            raise _lib.MasrError(f'{use_model}: encoder_conf.{key}={v!r} is not supported: a layer index (an integer)')
        return v
    L = index('num_blocks', enc.get('num_blocks', 12))
    if use_model == 'squeezeformer':
        red, rec = enc.get('reduce_idx', 5), enc.get('recover_idx', 11)
        r = -1 if red is None else index('reduce_idx', red)
        c = -1 if rec is None else index('recover_idx', rec)
        if red is not None and not 0 <= r < L:
            raise _lib.MasrError(f'squeezeformer: encoder_conf.reduce_idx={red!r} is not supported: null or a layer in '
                                 f'[0, num_blocks = {L})')
        if red is not None and (rec is None or not r <= c < L):
            raise _lib.MasrError(f'squeezeformer: encoder_conf.recover_idx={rec!r} with reduce_idx={r} is not supported: a layer in '
                                 f'[reduce_idx, num_blocks = {L}) (the reference fails on a recovery in front of the reduction; with '
                                 f'recover_idx null or >= num_blocks its output stays at half the frame rate, which is not implemented)')
        return r, c
    eff = dict(enc.get('efficient_conf', {}) or {})
    stride_idx = eff.get('stride_layer_idx', [3])
    stride_idx = list(stride_idx) if isinstance(stride_idx, (list, tuple)) else [stride_idx]
    groups = eff.get('group_layer_idx', [0, 1, 2, 3])
    groups = list(groups) if isinstance(groups, (list, tuple)) else [groups]
    stride = eff.get('stride', [2])
    stride = list(stride) if isinstance(stride, (list, tuple)) else [stride]
    if len(stride_idx) != 1 or stride != [2]:
        raise _lib.MasrError(f'efficient_conformer: efficient_conf.stride_layer_idx={stride_idx!r} with stride={stride!r} is not '
                             f'supported: only one stride-2 layer and leading grouped layers are supported')
    s = index('stride_layer_idx', stride_idx[0])
    if not 0 <= s < L:
        raise _lib.MasrError(f'efficient_conformer: efficient_conf.stride_layer_idx={s} is not supported: one stride layer in '
                             f'[0, num_blocks = {L})')
    if groups != list(range(len(groups))):
        raise _lib.MasrError(f'efficient_conformer: efficient_conf.group_layer_idx={groups!r} is not supported: only one stride-2 '
                             f'layer and leading grouped layers (0, 1, ..., g - 1) are supported')
    if len(groups) > s + 1:
        raise _lib.MasrError(f'efficient_conformer: efficient_conf.group_layer_idx={groups!r} with stride_layer_idx={s} is not '
                             f'supported: grouped attention after the stride layer is not implemented (at most layers 0 .. {s})')
    return s, len(groups)


def _validate_encoder_conf(use_model, enc, state_dict, streaming=None):
    """The kernels implement exactly the module variants the shipped YAMLs select; anything else must fail here instead of
    loading cleanly into the wrong arithmetic (e.g. ``cnn_module_norm: batch_norm`` has LayerNorm-shaped ``norm.weight``).
    ``streaming``: the build, where the caller knows it (``cnn_module_kernel`` has to be odd on a ``streaming: False`` one)."""
    def want(key, allowed, default):
        v = enc.get(key, default)
        if v not in allowed:
            raise _lib.MasrError(f'{use_model}: encoder_conf.{key}={v!r} is not implemented (supported: {allowed})')
    if use_model != 'deepspeech2':
        # model width (masr_create repeats these checks): 256 / 4 for every family; the Conformer also 512 / 8, on the width-generic
        # path (csrc/wide.hip), which carries layer_norm and the conv2d input layer only
        width_key = 'encoder_dim' if use_model == 'squeezeformer' else 'output_size'
        pair = (enc.get(width_key, 256), enc.get('attention_heads', 4))
        if pair != (256, 4) and not (use_model == 'conformer' and pair == (512, 8)):
            raise _lib.MasrError(f'{use_model}: encoder_conf.{width_key} / attention_heads = {pair[0]!r} / {pair[1]!r} is not '
                                 f'supported: 256 / 4 for every family, 512 / 8 for the conformer only')
        if pair[0] == 512:
            if enc.get('cnn_module_norm', 'layer_norm') == 'batch_norm':
                raise _lib.MasrError('conformer: encoder_conf.cnn_module_norm=\'batch_norm\' is implemented at output_size 256 only')
            if enc.get('input_layer', 'conv2d') != 'conv2d':
                raise _lib.MasrError(f'conformer: encoder_conf.input_layer={enc.get("input_layer")!r} is implemented at output_size '
                                     f'256 only (output_size 512 takes conv2d)')
        _validate_cnn_kernel(use_model, enc, state_dict, streaming)
    if use_model in ('squeezeformer', 'efficient_conformer'):
        _layer_layout(use_model, enc)
    if use_model in ('conformer', 'efficient_conformer'):
        # batch_norm (conformer/convolution.py:60-67, eval-mode statistics folded into scale / shift): Conformer in the full-context
        # forward only, Efficient Conformer full-context and chunked.  An absent key means layer_norm here for both families (the
        # reference's EfficientConformerEncoder defaults to batch_norm; the shipped YAML sets layer_norm)
        want('cnn_module_norm', ('layer_norm', 'batch_norm'), 'layer_norm')
        _validate_activation(use_model, enc)
        want('normalize_before', (True,), True)
        want('use_cnn_module', (True,), True)
        want('macaron_style', (True,), True)
        want('input_layer', tuple(INPUT_LAYERS), 'conv2d')
        _validate_pos_enc(use_model, enc, state_dict)
        has_bn = state_dict is not None and any(k.endswith('conv_module.norm.running_mean') for k in state_dict)
        is_bn = enc.get('cnn_module_norm', 'layer_norm') == 'batch_norm'
        if has_bn != is_bn and state_dict is not None:
            raise _lib.MasrError(f'{use_model}: encoder_conf.cnn_module_norm={enc.get("cnn_module_norm", "layer_norm")!r} but the checkpoint '
                                 f'{"holds" if has_bn else "has no"} BatchNorm statistics (conv_module.norm.running_mean)')
    elif use_model == 'squeezeformer':
        want('cnn_norm_type', ('batch_norm',), 'batch_norm')
        _validate_activation(use_model, enc)
        want('normalize_before', (False,), False)
        _validate_pos_enc(use_model, enc, state_dict)
        want('adaptive_scale', (True,), True)
        want('dw_stride', (False,), False)
    elif use_model == 'deepspeech2':
        # use_gru (deepspeech2/encoder.py:21-33): nn.GRU inside the reference's own GRU module, so its keys carry one more '.rnn'
        want('use_gru', (False, True), False)
        has_gru = state_dict is not None and 'encoder.rnns.0.rnn.rnn.weight_ih_l0' in state_dict
        is_gru = bool(enc.get('use_gru', False))
        if has_gru != is_gru and state_dict is not None:
            raise _lib.MasrError(f'{use_model}: encoder_conf.use_gru={is_gru!r} but the checkpoint holds '
                                 f'{"GRU" if has_gru else "LSTM"} layers ({"encoder.rnns.0.rnn.rnn" if has_gru else "encoder.rnns.0.rnn"}'
                                 f'.weight_ih_l0)')


DECODER_PREFIXES = ('decoder.left_decoder.', 'decoder.right_decoder.')


def _decoder_blocks(state_dict, side):
    """number of DecoderLayers a checkpoint holds under ``decoder.<side>_decoder.decoders``"""
    head = f'decoder.{side}_decoder.decoders.'
    return len({k[len(head):].split('.', 1)[0] for k in state_dict if k.startswith(head)})


def _validate_decoder_conf(use_model, dec, state_dict, d_model=256):
    """``decoder_conf`` of an engine that is to rescore with the checkpoint's attention decoder (``decoder: attention_rescoring``):
    the BiTransformerDecoder the reference trains beside the CTC head (transformer/decoder.py; configs: 3 + 3 blocks, 4 heads,
    linear_units 1024).  The kernels run the shipped variant -- pre-norm blocks, no concat, an output layer, heads of 64 -- and
    ``attention_heads`` / ``linear_units`` / ``num_blocks`` / ``r_num_blocks`` have to be the checkpoint's own, in both directions.
    -> (attention_heads, linear_units, num_blocks, r_num_blocks); masr_decoder_enable / masr_finalize repeat the checks."""
    dec = dict(dec or {})
    if use_model == 'deepspeech2':
        raise _lib.MasrError("deepspeech2: decoder='attention_rescoring' is not available: use_model deepspeech2 has no attention "
                             "decoder (its decoder.* tensors are the CTC head)")
    if state_dict is None or not any(k.startswith('decoder.left_decoder.') for k in state_dict):
        raise _lib.MasrError(f"{use_model}: decoder='attention_rescoring' but the checkpoint holds no decoder.left_decoder.* tensors "
                             f"(it has no attention decoder)")
    for key, allowed, default in (('normalize_before', (True,), True), ('concat_after', (False,), False),
                                  ('use_output_layer', (True,), True), ('input_layer', ('embed',), 'embed')):
        v = dec.get(key, default)
        if v not in allowed or isinstance(v, bool) != isinstance(allowed[0], bool):
            raise _lib.MasrError(f'{use_model}: decoder_conf.{key}={v!r} is not implemented (supported: {allowed})')

    def integer(key, default):
        v = dec.get(key, default)
        if isinstance(v, bool) or not isinstance(v, int):
            raise _lib.MasrError(f'{use_model}: decoder_conf.{key}={v!r} is not an integer')
        return v
    heads, units = integer('attention_heads', 4), integer('linear_units', 2048)
    nl, nr = integer('num_blocks', 6), integer('r_num_blocks', 0)
    if heads * 64 != d_model:
        raise _lib.MasrError(f'{use_model}: decoder_conf.attention_heads={heads} is not supported at an encoder output of {d_model}: '
                             f'{d_model // 64} (the decoder\'s attention kernel runs heads of 64)')
    if units <= 0 or units % 32:
        raise _lib.MasrError(f'{use_model}: decoder_conf.linear_units={units} is not supported: a positive multiple of 32')
    key = 'decoder.left_decoder.decoders.0.feed_forward.w_1.weight'
    if key in state_dict and int(state_dict[key].shape[0]) != units:
        raise _lib.MasrError(f'{use_model}: decoder_conf.linear_units={units} but the checkpoint was trained with '
                             f'linear_units={int(state_dict[key].shape[0])} ({key} is {list(state_dict[key].shape)})')
    key = 'decoder.left_decoder.embed.0.weight'
    if key in state_dict and int(state_dict[key].shape[1]) != d_model:
        raise _lib.MasrError(f'{use_model}: the attention decoder is {int(state_dict[key].shape[1])} wide ({key}) but the encoder '
                             f'output is {d_model}')
    for conf_key, side, want in (('num_blocks', 'left', nl), ('r_num_blocks', 'right', nr)):
        have = _decoder_blocks(state_dict, side)
        if have != want:
            raise _lib.MasrError(f'{use_model}: decoder_conf.{conf_key}={want} but the checkpoint holds {have} blocks under '
                                 f'decoder.{side}_decoder.decoders')
    if nl < 1:
        raise _lib.MasrError(f'{use_model}: decoder_conf.num_blocks={nl} is not supported: at least 1')
    return heads, units, nl, nr


RNN_SIZES = tuple(range(256, 2049, 256))


def _validate_rnn_size(enc, state_dict):
    """DeepSpeech2 ``encoder_conf.rnn_size`` (configs/deepspeech2.yml): the recurrent step kernels (lstm.hip, gru.hip) are
    instantiated for every multiple of 256 from 256 to 2048, and the value has to be the checkpoint's own hidden size."""
    size = enc.get('rnn_size', 1024)
    if isinstance(size, bool) or not isinstance(size, int) or size not in RNN_SIZES:
        raise _lib.MasrError(f'deepspeech2: encoder_conf.rnn_size={size!r} is not supported: multiples of 256 from 256 to 2048 '
                             f'are ({", ".join(map(str, RNN_SIZES))})')
    if state_dict is None:
        return
    for key in ('encoder.rnns.0.rnn.weight_hh_l0', 'encoder.rnns.0.rnn.rnn.weight_hh_l0'):
        if key in state_dict:
            have = int(state_dict[key].shape[1])
            if have != size:
                raise _lib.MasrError(f'deepspeech2: encoder_conf.rnn_size={size} but the checkpoint was trained with rnn_size={have} '
                                     f'({key} is {list(state_dict[key].shape)})')


class HipEngine:
    """One engine per GPU rank.  ``state_dict`` uses the reference key names
    (``encoder.*`` / ``ctc.*``; extra keys are ignored); ``state_dict=None`` gives a weight-less
    engine that can run the model-independent kernels (fbank, argmax, CTC collapse)."""

    def __init__(self, state_dict, encoder_conf=None, vocab_size=None, streaming=True, n_mels=80, device=None,
                 max_pos=5000, use_model='conformer', decoder_conf=None, attention_decoder=False):
        """``attention_decoder=True`` (``decoder: attention_rescoring``): the engine also loads the checkpoint's
        ``decoder.left_decoder.*`` / ``decoder.right_decoder.*`` tensors, described by ``decoder_conf`` (the YAML block), and
        ``rescore`` works; otherwise those tensors are never touched and the engine is what it always was."""
        if not torch.cuda.is_available():
            raise _lib.MasrError('no HIP device visible to torch: the MI355X engine has no CPU fallback')
        if device is None:          # the calling rank's GPU (one process per GPU: torch.cuda.set_device(LOCAL_RANK) comes first)
            device = torch.cuda.current_device()
        device = int(device)
        self.lib = _lib.lib()
        enc = dict(encoder_conf or {})
        if vocab_size is None:
            ctc_key = 'decoder.ctc_lo.weight' if use_model == 'deepspeech2' else 'ctc.ctc_lo.weight'
            vocab_size = int(state_dict[ctc_key].shape[0]) if state_dict is not None else 1
        self.device = torch.device('cuda', device)
        torch.cuda.set_device(self.device)
        _validate_encoder_conf(use_model, enc, state_dict, bool(streaming))
        if use_model == 'deepspeech2':
            _validate_rnn_size(enc, state_dict)
        # subsampling front-end (Conformer / Efficient Conformer; the other models have their own)
        self.input_layer = enc.get('input_layer', 'conv2d') if use_model in ('conformer', 'efficient_conformer') else 'conv2d'
        if use_model == 'conformer':
            cfg = MasrConfig(model_kind=0, d_model=int(enc.get('output_size', 256)),
                             heads=int(enc.get('attention_heads', 4)), d_ff=int(enc.get('linear_units', 2048)),
                             num_blocks=int(enc.get('num_blocks', 12)),
                             cnn_kernel=int(enc.get('cnn_module_kernel', 15)), n_mels=n_mels,
                             vocab_size=int(vocab_size), causal=1 if streaming else 0, max_pos=max_pos,
                             device_id=device)
            cfg.reserved[0] = 1 if enc.get('cnn_module_norm', 'layer_norm') == 'batch_norm' else 0
            cfg.reserved[3] = INPUT_LAYERS[self.input_layer]
            cfg.reserved[2] = POS_ENC_LAYER_TYPES[enc.get('pos_enc_layer_type', 'rel_pos')]
            cfg.reserved[4] = ACTIVATION_TYPES[enc.get('activation_type', 'swish')]
        elif use_model == 'squeezeformer':
            # configs/squeezeformer.yml: encoder_dim, feed_forward_expansion_factor, reduce_idx / recover_idx
            dim = int(enc.get('encoder_dim', 256))
            cfg = MasrConfig(model_kind=1, d_model=dim, heads=int(enc.get('attention_heads', 4)),
                             d_ff=dim * int(enc.get('feed_forward_expansion_factor', 8)),
                             num_blocks=int(enc.get('num_blocks', 12)),
                             cnn_kernel=int(enc.get('cnn_module_kernel', 31)), n_mels=n_mels,
                             vocab_size=int(vocab_size), causal=1 if streaming else 0, max_pos=max_pos,
                             device_id=device)
            cfg.reserved[0], cfg.reserved[1] = _layer_layout(use_model, enc)
        elif use_model == 'efficient_conformer':
            # configs/efficient_conformer.yml: the nested efficient_conf is swallowed by **kwargs in the reference
            # (efficient_conformer/encoder.py:54); its constructor defaults equal the shipped YAML values
            eff = dict(enc.get('efficient_conf', {}) or {})
            cfg = MasrConfig(model_kind=2, d_model=int(enc.get('output_size', 256)),
                             heads=int(enc.get('attention_heads', 4)), d_ff=int(enc.get('linear_units', 2048)),
                             num_blocks=int(enc.get('num_blocks', 12)),
                             cnn_kernel=int(enc.get('cnn_module_kernel', 15)), n_mels=n_mels,
                             vocab_size=int(vocab_size), causal=1 if streaming else 0, max_pos=max_pos,
                             device_id=device)
            cfg.reserved[0], cfg.reserved[1] = _layer_layout(use_model, enc)
            cfg.reserved[2] = int(eff.get('group_size', 3))
            cfg.reserved[4] = 1 if enc.get('cnn_module_norm', 'layer_norm') == 'batch_norm' else 0
            cfg.reserved[3] = INPUT_LAYERS[self.input_layer]
        elif use_model == 'deepspeech2':
            # configs/deepspeech2.yml encoder_conf: rnn_size, num_rnn_layers, use_gru; streaming <=> uni-directional recurrent
            # layers (deepspeech2/encoder.py:14-19: rnn_direction = 'forward' if streaming else 'bidirect')
            cfg = MasrConfig(model_kind=3, d_model=int(enc.get('rnn_size', 1024)), heads=0, d_ff=0,
                             num_blocks=int(enc.get('num_rnn_layers', 5)), cnn_kernel=0, n_mels=n_mels,
                             vocab_size=int(vocab_size), causal=1 if streaming else 0, max_pos=max_pos,
                             device_id=device)
            cfg.reserved[0] = int(enc.get('use_gru', False))          # 0 = LSTM, 1 = GRU (checked above)
        else:
            raise _lib.MasrError(f'use_model={use_model}: conformer, squeezeformer, efficient_conformer, deepspeech2 '
                                 f'are implemented')
        self.use_model = use_model
        self.pos_enc_layer_type = enc.get('pos_enc_layer_type', 'rel_pos') if use_model == 'conformer' else 'rel_pos'
        self.activation_type = enc.get('activation_type', 'swish') if use_model == 'conformer' else 'swish'
        self.cfg = cfg
        self.d_model, self.vocab_size, self.n_mels = cfg.d_model, cfg.vocab_size, n_mels
        # width of the encoder output rows (DeepSpeech2: rnn_size x directions)
        self.enc_dim = cfg.d_model * (1 if streaming else 2) if use_model == 'deepspeech2' else cfg.d_model
        self.num_blocks, self.heads, self.cnn_kernel = cfg.num_blocks, cfg.heads, cfg.cnn_kernel
        # (refused before an engine exists: nothing to release on the way out)
        dconf = _validate_decoder_conf(use_model, decoder_conf, state_dict, self.enc_dim) if attention_decoder else None
        h = C.c_void_p()
        check(self.lib.masr_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.lane = 0
        self._up_ring = PinnedRing(8, min_numel=64, events=True)          # ``to_device``
        self.has_weights = state_dict is not None
        self.has_decoder = False
        self.max_pos = int(max_pos)
        if attention_decoder:
            check(self.lib.masr_decoder_enable(self.h, *dconf))
            self.has_decoder, self.decoder_blocks = True, dconf[2:]
        if state_dict is None:      # weight-less engine: fbank / argmax / collapse kernels only
            return
        for name, t in state_dict.items():
            if not (name.startswith('encoder.') or name.startswith('ctc.') or name.startswith('decoder.ctc_lo.')):
                if not (self.has_decoder and name.startswith(DECODER_PREFIXES) and torch.is_tensor(t) and t.is_floating_point()):
                    continue
            self._load(name, t)
        if use_model != 'deepspeech2':
            self._load('__pos_table__', positional_table(max_pos, cfg.d_model))
        check(self.lib.masr_finalize(self.h, _stream()))

    def _load(self, name, t):
        a = np.ascontiguousarray(t.detach().cpu().float().numpy())
        shape = (C.c_int64 * a.ndim)(*a.shape)
        check(self.lib.masr_load_tensor(self.h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))

    def close(self):
        if getattr(self, 'h', None):
            for pool in list(self.__dict__.get('_pools', ())):        # serving pools hold streams of this engine
                pool.shutdown()
            torch.cuda.synchronize()
            self.lib.masr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- features -------------------------------------------------------------------------------
    def mean_square(self, samples, n_samples, out=None):
        """float32 ``np.mean(samples ** 2)`` per utterance in numpy's summation order (audio.py:524) -> [B] f32 (device).  The
        kernels use a scratch of the calling stream's own (not the feature launch's): preparing the next pass on a side
        stream never touches what the current pass reads."""
        B, n_max = samples.shape
        fmt = {torch.int16: 0, torch.float32: 1}[samples.dtype]
        ms = out if out is not None else torch.empty(B, dtype=torch.float32, device=self.device)
        check(self.lib.masr_mean_square(self.h, _ptr(samples), fmt, _ptr(n_samples), B, n_max, _ptr(ms), _stream()))
        return ms

    def resample_table(self, sr_orig, sr_new, filter='kaiser_best'):
        """(win, dwin) pairs of ``filter`` for ``sr_orig -> sr_new`` on the device (``data_utils.resample.device_table``),
        uploaded once per (ratio, filter) and kept on the engine -> (tensor [nwin, 2] float64, num_table)"""
        from .data_utils.resample import device_table
        cache = self.__dict__.setdefault('_resample_tables', {})
        key = (float(sr_new) / sr_orig, filter)
        if key not in cache:
            pairs, num_table = device_table(sr_orig, sr_new, filter)
            cache[key] = (torch.from_numpy(pairs).to(self.device), num_table)
        return cache[key]

    def resample_rows(self, src, n_in, sr_orig, sr_new, filter='kaiser_best', out=None, dst_rows=None):
        """masr_resample_rows: the rows of ONE source rate -- ``src`` [R, m] int16 PCM or float32 (device), ``n_in`` [R] their
        lengths (host) -- resampled to ``sr_new`` on the current stream, bit for bit the samples of ``AudioSegment.resample``
        (audio.py:306-317).  Row i goes to row ``dst_rows[i]`` (default i) of ``out`` [B, n_max] float32 (default: a new
        [R, longest output] buffer), zeros behind its own ``int(n_in[i] * ratio)`` samples.  ``sr_orig == sr_new``: the rows
        are converted and copied.  -> (out, output lengths [R] int32 numpy); raises like the host resampler for a row too
        short to give one sample."""
        from .data_utils.resample import resampled_length
        R = src.shape[0]
        fmt = {torch.int16: 0, torch.float32: 1}[src.dtype]
        n_in = np.asarray(n_in, np.int64).reshape(-1)
        if n_in.shape[0] != R or not src.is_contiguous():
            raise ValueError('resample_rows: src [R, m] contiguous and one length per row expected')
        same = sr_orig == sr_new
        n_out = n_in if same else np.array([resampled_length(n, sr_orig, sr_new) for n in n_in], np.int64)
        if out is None:
            out = torch.empty(R, int(n_out.max(initial=1)), dtype=torch.float32, device=self.device)
        rows = np.stack([n_in, n_out, np.arange(R) if dst_rows is None else np.asarray(dst_rows, np.int64)], axis=1).astype(np.int32)
        table, num_table = (None, 0) if same else self.resample_table(sr_orig, sr_new, filter)
        rows_dev = self.to_device(rows)
        check(self.lib.masr_resample_rows(self.h, _ptr(src), fmt, src.shape[1], rows.ctypes.data_as(C.c_void_p), _ptr(rows_dev), R,
                                          float(sr_new) / sr_orig, _ptr(table), 0 if same else table.shape[0], num_table,
                                          _ptr(out), out.shape[0], out.shape[1], _stream()))
        return out, n_out.astype(np.int32)

    def resample_rate(self, sr_orig, sr_new, filter='kaiser_best'):
        """one ``masr_resample_rate`` record (``_lib.RESAMPLE_RATE``) for ``sr_orig -> sr_new``: the table of
        :meth:`resample_table` and what ``masr_resample_rate_fill`` derives from the ratio"""
        from ._lib import RESAMPLE_RATE
        table, num_table = self.resample_table(sr_orig, sr_new, filter)
        rec = np.zeros(1, RESAMPLE_RATE)
        if self.lib.masr_resample_rate_fill(float(sr_new) / sr_orig, _ptr(table), table.shape[0], num_table,
                                            rec.ctypes.data_as(C.c_void_p)) != 0:
            raise ValueError(f'cannot resample from {sr_orig}->{sr_new}: ratio too small for the filter table')
        return rec[0]

    def resample_plan(self, feeds, rates, src_bytes, dst_rows, dst_stride):
        """masr_resample_plan (host only): validates ``feeds`` (``_lib.RESAMPLE_FEED`` records) against ``rates``
        (``_lib.RESAMPLE_RATE`` records) and the buffers -> the tile list [n_tiles, 2] int32 = (feed, first output); raises
        ValueError with the reason for a refused feed"""
        feeds, rates = np.ascontiguousarray(feeds), np.ascontiguousarray(rates)
        n, bad, why = C.c_int64(), C.c_int32(), C.c_char_p()
        args = (feeds.ctypes.data_as(C.c_void_p), feeds.shape[0], rates.ctypes.data_as(C.c_void_p), rates.shape[0], int(src_bytes),
                int(dst_rows), int(dst_stride))
        if self.lib.masr_resample_plan(*args, None, 0, C.byref(n), C.byref(bad), C.byref(why)) != 0:
            raise ValueError(f'resample_plan: feed {bad.value}: {(why.value or b"refused").decode()}')
        tiles = np.zeros((n.value, 2), np.int32)
        self.lib.masr_resample_plan(*args, tiles.ctypes.data_as(C.c_void_p), n.value, C.byref(n), C.byref(bad), C.byref(why))
        return tiles

    def resample_feeds(self, src, feeds, rates, tiles, out):
        """masr_resample_feeds: many short feeds of mixed rates and formats in ONE launch on the current stream.  ``src``: the
        feeds' raw bytes, one ragged uint8 device buffer; ``feeds`` / ``rates`` / ``tiles``: the host tables (uploaded here);
        feed k writes ``out[dst_row, dst_offset : dst_offset + n_out]`` (float32 device, contiguous) and nothing else, bit for
        bit the samples ``AudioSegment.resample`` makes of it on its own (predict.py:260-281 -> audio.py:306-317).  Raises
        MasrError, with nothing launched, for what ``masr_resample_plan`` refuses."""
        feeds, rates, tiles = np.ascontiguousarray(feeds), np.ascontiguousarray(rates), np.ascontiguousarray(tiles, np.int32)
        if src.dtype != torch.uint8 or out.dtype != torch.float32 or out.dim() != 2 or not out.is_contiguous() or not src.is_contiguous():
            raise ValueError('resample_feeds: src uint8 and out [rows, stride] float32, both contiguous, expected')
        up = [self.to_device(a.view(np.uint8)) for a in (feeds, rates, tiles)]
        check(self.lib.masr_resample_feeds(self.h, _ptr(src), src.numel(), feeds.ctypes.data_as(C.c_void_p), _ptr(up[0]), feeds.shape[0],
                                           rates.ctypes.data_as(C.c_void_p), _ptr(up[1]), rates.shape[0],
                                           tiles.ctypes.data_as(C.c_void_p), _ptr(up[2]), tiles.shape[0], _ptr(out), out.shape[0],
                                           out.shape[1], _stream()))
        return out

    def side_stream(self, kind):
        """a side stream of THIS DEVICE owned by libmasr_hip.so (masr_side_stream; kind 0 / 1: prefix searches of consecutive
        passes, 2: per-pass preparation, 3: copies, 4: encoder passes of lane 1), as a torch stream.  One set per device, created
        with the device's first engine at default priority -- hardware queues of their own, whatever streams the process creates
        before or after (include/masr_hip.h); borrowed, never destroyed."""
        cache = self.__dict__.setdefault('_side', {})
        st = cache.get(kind)
        if st is None:
            ptr = C.c_void_p()
            check(self.lib.masr_side_stream(self.h, int(kind), C.byref(ptr)))
            st = cache[kind] = torch.cuda.ExternalStream(ptr.value, device=self.device)
        return st

    def select_lane(self, lane):
        """masr_select_lane: the calls that follow use workspace set ``lane`` (0 / 1) of this engine, so two offline passes can be
        in flight on two streams; launches sharing a lane must be ordered by their stream (include/masr_hip.h)."""
        check(self.lib.masr_select_lane(self.h, int(lane)))
        self.lane = int(lane)

    @contextlib.contextmanager
    def on_lane(self, lane, stream):
        """the calls inside run on workspace set ``lane`` and on ``stream``; afterwards the lane that was active is selected again
        (every caller outside such a block works on lane 0)"""
        active = self.lane
        if lane != active:
            self.select_lane(lane)
        try:
            with torch.cuda.stream(stream):
                yield
        finally:
            if lane != active:
                self.select_lane(active)

    def to_host(self, t):
        """small device tensor -> numpy through a pinned buffer, waiting for THIS stream only.  (``tensor.cpu()`` copies to
        pageable memory, which the HIP runtime serialises against every stream of the device: a prefix search running on a side
        stream then stalls the next pass's features and encoder for its whole duration -- 32 ms per predict_batch call of
        BASELINE configs[2], tools/beam_batch_profile.py.)"""
        pin = self.__dict__.setdefault('_pins', {})
        buf = pin.get(t.dtype)
        if buf is None or buf.numel() < t.numel():
            buf = torch.empty(max(int(t.numel()), 256), dtype=t.dtype, pin_memory=True)
            pin[t.dtype] = buf
        view = buf[:t.numel()].view(t.shape)
        view.copy_(t, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return view.numpy().copy()

    def to_device(self, a):
        """small host array -> device through pinned memory (asynchronous, no device-wide serialisation).  A ring of eight pinned
        slots per dtype; every slot carries the event of its last copy (recorded on the stream the copy was issued on), which is
        waited for before the slot is rewritten -- a copy queued on a side stream behind a long prefix search keeps its source
        however many uploads follow."""
        t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
        slot = self._up_ring.take(t.numel(), t.dtype)
        slot.buf.copy_(t)
        out = slot.buf.view(np.shape(a)).to(self.device, non_blocking=True)
        slot.record(torch.cuda.current_stream(self.device))
        return out

    def host_gains(self, samples, n_samples, target_db, max_gain_db=300.0):
        """The reference's normalisation gain evaluated where the reference evaluates it: the mean square comes from the
        device (bit-identical to numpy's), the scalar float32 expressions of ``rms_db`` / ``normalize`` / ``gain_db``
        (audio.py:256-264,287-304,519-529) run on THIS host's numpy, whose float32 log10 / power are not correctly rounded
        and differ between machines.  Returns linear gains [B] f32 (device); raises like ``normalize`` beyond max_gain_db."""
        return self.to_device(reference_gains(self.to_host(self.mean_square(samples, n_samples)), target_db, max_gain_db))

    def _db_mode(self, use_db_normalization, gain_in, B, return_gain):
        """-> (mode for the C ABI, gain tensor): 0 off / 1 device gains (returned in the tensor when asked) / 2 supplied gains"""
        if use_db_normalization and gain_in is not None:
            return 2, gain_in.to(device=self.device, dtype=torch.float32).contiguous().clone()
        gain = torch.ones(B, dtype=torch.float32, device=self.device) if return_gain else None
        return (1 if use_db_normalization else 0), gain

    def fbank_batch(self, samples, n_samples, use_db_normalization=True, target_db=-20.0, return_norm=False,
                    return_gain=False, gain_in=None):
        """samples int16 PCM or float32 [B, n_max] (device), n_samples int32 [B] (device)
        -> feats [B,T,80], frames [B] (+ normalised int16 samples, + linear gains).  ``gain_in`` [B]: linear gains supplied
        by the caller (``host_gains``) instead of the device's own evaluation."""
        B, n_max = samples.shape
        fmt = {torch.int16: 0, torch.float32: 1}[samples.dtype]
        T = 1 + (n_max - 400) // 160 if n_max >= 400 else 0
        feats = torch.empty(B, T, 80, dtype=torch.float32, device=self.device)
        frames = torch.empty(B, dtype=torch.int32, device=self.device)
        norm = torch.empty(B, n_max, dtype=torch.int16, device=self.device) if return_norm else None
        mode, gain = self._db_mode(use_db_normalization, gain_in, B, return_gain)
        check(self.lib.masr_fbank_batch(self.h, _ptr(samples), fmt, _ptr(n_samples), B, n_max,
                                        mode, float(target_db), _ptr(feats), _ptr(frames),
                                        _ptr(norm), _ptr(gain), _stream()))
        res = [feats, frames]
        if return_norm:
            res.append(norm)
        if return_gain:
            res.append(gain)
        return tuple(res)

    def mfcc_batch(self, samples, n_samples, n_mfcc=40, use_db_normalization=True, target_db=-20.0, return_gain=False,
                   gain_in=None):
        """kaldi.mfcc(num_mel_bins=80, num_ceps=n_mfcc) for a padded batch -> feats [B,T,n_mfcc], frames [B] (+ gains)."""
        B, n_max = samples.shape
        fmt = {torch.int16: 0, torch.float32: 1}[samples.dtype]
        T = 1 + (n_max - 400) // 160 if n_max >= 400 else 0
        feats = torch.empty(B, T, int(n_mfcc), dtype=torch.float32, device=self.device)
        frames = torch.empty(B, dtype=torch.int32, device=self.device)
        mode, gain = self._db_mode(use_db_normalization, gain_in, B, return_gain)
        check(self.lib.masr_mfcc_batch(self.h, _ptr(samples), fmt, _ptr(n_samples), B, n_max, mode,
                                       float(target_db), int(n_mfcc), _ptr(feats), _ptr(frames), _ptr(gain), _stream()))
        return (feats, frames, gain) if return_gain else (feats, frames)

    def linear_batch(self, samples, n_samples, use_db_normalization=True, target_db=-20.0, return_gain=False, gain_in=None):
        """linear log power spectrogram (20 ms / 10 ms, 161 bins) for a padded batch -> feats [B,T,161], frames [B]."""
        B, n_max = samples.shape
        fmt = {torch.int16: 0, torch.float32: 1}[samples.dtype]
        T = (n_max - 320) // 160 + 1 if n_max >= 320 else 0
        feats = torch.empty(B, T, 161, dtype=torch.float32, device=self.device)
        frames = torch.empty(B, dtype=torch.int32, device=self.device)
        mode, gain = self._db_mode(use_db_normalization, gain_in, B, return_gain)
        check(self.lib.masr_linear_batch(self.h, _ptr(samples), fmt, _ptr(n_samples), B, n_max,
                                         mode, float(target_db), _ptr(feats), _ptr(frames),
                                         _ptr(gain), _stream()))
        return (feats, frames, gain) if return_gain else (feats, frames)

    def features_batch(self, method, samples, n_samples, use_db_normalization=True, target_db=-20.0, n_mfcc=40,
                       return_gain=False, gain_in=None):
        """dispatch on the reference's ``feature_method`` (audio_featurizer.py:51-69)"""
        if method == 'fbank':
            return self.fbank_batch(samples, n_samples, use_db_normalization, target_db, return_gain=return_gain,
                                    gain_in=gain_in)
        if method == 'mfcc':
            return self.mfcc_batch(samples, n_samples, n_mfcc, use_db_normalization, target_db, return_gain=return_gain,
                                   gain_in=gain_in)
        if method == 'linear':
            return self.linear_batch(samples, n_samples, use_db_normalization, target_db, return_gain=return_gain,
                                     gain_in=gain_in)
        raise Exception('没有{}预处理方法'.format(method))

    # ---- encoder ----------------------------------------------------------------------------------
    def encode_full(self, feats, lens, decoding_chunk_size=-1):
        """feats f32 [B,T,80] (device, zero padded), lens int32 [B] (device) -> enc [B,T',d]."""
        B, T, _ = feats.shape
        Tp = self.out_frames(T)
        enc = torch.empty(B, Tp, self.enc_dim, dtype=torch.float32, device=self.device)
        check(self.lib.masr_encode_full(self.h, _ptr(feats), _ptr(lens), B, T, int(decoding_chunk_size), _ptr(enc),
                                        _stream()))
        return enc

    def out_frames(self, T):
        """encoder output frames for T feature frames (the Efficient Conformer halves the rate once more)."""
        Tp = subsampled_len(T, getattr(self, 'input_layer', 'conv2d'))
        return (Tp + 1) // 2 if getattr(self, 'use_model', 'conformer') == 'efficient_conformer' else Tp

    @property
    def min_frames(self):
        """the fewest feature frames that give one encoder frame (7 / 11 / 15 for conv2d / conv2d6 / conv2d8)"""
        return MIN_FRAMES[getattr(self, 'input_layer', 'conv2d')]

    def enc_frames(self, feat_frames):
        """valid encoder frames per utterance for its feature frames (tensor or array; mirrors launch_frame_counts in
        elementwise.hip: Conv2dSubsampling4 / 6 / 8, once more halved with ceil by the Efficient Conformer's stride layer)."""
        n4 = subsampled_len(feat_frames, getattr(self, 'input_layer', 'conv2d'))
        n4 = n4.clamp(min=0) if torch.is_tensor(n4) else np.maximum(n4, 0)
        return (n4 + 1) // 2 if self.use_model == 'efficient_conformer' else n4

    def ctc_probs(self, enc, want_argmax=False):
        M = enc.numel() // self.enc_dim
        probs = torch.empty(*enc.shape[:-1], self.vocab_size, dtype=torch.float32, device=self.device)
        idx = torch.empty(M, dtype=torch.int32, device=self.device) if want_argmax else None
        mp = torch.empty(M, dtype=torch.float32, device=self.device) if want_argmax else None
        check(self.lib.masr_ctc_probs(self.h, _ptr(enc), M, _ptr(probs), _ptr(idx), _ptr(mp), _stream()))
        return (probs, idx, mp) if want_argmax else probs

    def ctc_greedy_frames(self, enc):
        M = enc.numel() // self.enc_dim
        idx = torch.empty(enc.shape[:-1], dtype=torch.int32, device=self.device)
        mp = torch.empty(enc.shape[:-1], dtype=torch.float32, device=self.device)
        check(self.lib.masr_ctc_greedy_frames(self.h, _ptr(enc), M, _ptr(idx), _ptr(mp), _stream()))
        return idx, mp

    def ctc_collapse(self, idx, maxp, n_frames=None, blank=0):
        B, Tp = idx.shape
        tokens = torch.empty(B, Tp, dtype=torch.int32, device=self.device)
        ntok = torch.empty(B, dtype=torch.int32, device=self.device)
        score = torch.empty(B, dtype=torch.float32, device=self.device)
        check(self.lib.masr_ctc_collapse(self.h, _ptr(idx), _ptr(maxp), _ptr(n_frames), B, Tp, blank, _ptr(tokens),
                                         _ptr(ntok), _ptr(score), _stream()))
        return tokens, ntok, score

    def ctc_align(self, post, n_frames, tokens, n_tokens, input_is_log=False, out=None):
        """masr_ctc_align on the current stream and the active lane: ``post`` [B, T', V] float32 (probabilities as ``ctc_probs``
        writes them, or log-probabilities with ``input_is_log=True``), ``n_frames`` [B] int32, ``tokens`` [B, Lmax] int32,
        ``n_tokens`` [B] int32 (all device tensors) -> (start, end [B, Lmax] int32, peak [B, Lmax] float32, score [B] float32,
        status [B] int32) device tensors (include/masr_hip.h: the tie rule and the meaning of ``status``).  ``out``: a flat int32
        device buffer of B * (3 Lmax + 2) elements = start | end | peak bits | score bits | status to write them into (so that
        ONE copy brings them back, ``unpack_alignment``); the five results are views of it.  Nothing is waited for."""
        B, Tp, V = post.shape
        Lmax = tokens.shape[1]
        if out is None:
            out = torch.empty(B * (3 * Lmax + 2), dtype=torch.int32, device=self.device)
        flat = out.view(-1)
        n = B * Lmax
        start, end = flat[:n].view(B, Lmax), flat[n:2 * n].view(B, Lmax)
        peak = flat[2 * n:3 * n].view(torch.float32).view(B, Lmax)
        score, status = flat[3 * n:3 * n + B].view(torch.float32), flat[3 * n + B:3 * n + 2 * B]
        if not (post.is_contiguous() and tokens.is_contiguous() and post.dtype == torch.float32 and tokens.dtype == torch.int32
                and n_frames.dtype == torch.int32 and n_tokens.dtype == torch.int32):
            raise ValueError('ctc_align: contiguous float32 posteriors and int32 tokens / n_frames / n_tokens expected')
        check(self.lib.masr_ctc_align(self.h, _ptr(post), 1 if input_is_log else 0, B, Tp, V, _ptr(n_frames), _ptr(tokens),
                                      _ptr(n_tokens), Lmax, _ptr(start), _ptr(end), _ptr(peak), _ptr(score), _ptr(status),
                                      _stream()))
        return start, end, peak, score, status

    def ctc_align_rows(self, rows, frame_row, n_frames, tokens, n_tokens, input_is_log=False, out=None):
        """masr_ctc_align_rows on the current stream and the active lane: ``ctc_align`` over frames that are not contiguous.
        ``rows`` [n_rows, V] float32 (a row pool), ``frame_row`` [B, Tmax] int64: frame t of utterance b is row ``frame_row[b, t]``
        (any order, entries behind ``n_frames[b]`` are never read; a number outside [0, n_rows) gives status 2 for that utterance);
        ``n_frames``, ``tokens``, ``n_tokens``, ``input_is_log`` and the packed ``out`` of B * (3 Lmax + 2) int32 as in
        ``ctc_align``, and the same five views come back, bit for bit what ``ctc_align`` gives on ``rows[frame_row]``.  Nothing is
        waited for."""
        n_rows, V = rows.shape
        B, Tmax = frame_row.shape
        Lmax = tokens.shape[1]
        if out is None:
            out = torch.empty(B * (3 * Lmax + 2), dtype=torch.int32, device=self.device)
        flat = out.view(-1)
        n = B * Lmax
        start, end = flat[:n].view(B, Lmax), flat[n:2 * n].view(B, Lmax)
        peak = flat[2 * n:3 * n].view(torch.float32).view(B, Lmax)
        score, status = flat[3 * n:3 * n + B].view(torch.float32), flat[3 * n + B:3 * n + 2 * B]
        if not (rows.is_contiguous() and frame_row.is_contiguous() and tokens.is_contiguous() and rows.dtype == torch.float32
                and frame_row.dtype == torch.int64 and tokens.dtype == torch.int32 and n_frames.dtype == torch.int32
                and n_tokens.dtype == torch.int32):
            raise ValueError('ctc_align_rows: contiguous float32 rows, int64 frame_row and int32 tokens / n_frames / n_tokens expected')
        check(self.lib.masr_ctc_align_rows(self.h, _ptr(rows), n_rows, V, 1 if input_is_log else 0, _ptr(frame_row), B, Tmax,
                                           _ptr(n_frames), _ptr(tokens), _ptr(n_tokens), Lmax, _ptr(start), _ptr(end), _ptr(peak),
                                           _ptr(score), _ptr(status), _stream()))
        return start, end, peak, score, status

    def frame_reduction(self):
        """masr_frame_reduction: feature frames per encoder frame of the loaded model (4 / 6 / 8 by the input layer, doubled by
        the Efficient Conformer's stride layer)"""
        r = C.c_int32()
        check(self.lib.masr_frame_reduction(self.h, C.byref(r)))
        return r.value

    def argmax_rows(self, probs):
        M, V = probs.shape
        idx = torch.empty(M, dtype=torch.int32, device=self.device)
        mp = torch.empty(M, dtype=torch.float32, device=self.device)
        check(self.lib.masr_argmax_rows(self.h, _ptr(probs), M, V, _ptr(idx), _ptr(mp), _stream()))
        return idx, mp

    def transcribe_batch(self, pcm, n_samples, use_db_normalization=True, target_db=-20.0, decode_all_frames=False,
                         out=None):
        """Whole offline hot path in one call, no host sync: PCM -> token ids."""
        B, n_max = pcm.shape
        Tp = self.out_frames(1 + (n_max - 400) // 160)
        if out is None:
            out = (torch.empty(B, Tp, dtype=torch.int32, device=self.device),
                   torch.empty(B, dtype=torch.int32, device=self.device),
                   torch.empty(B, dtype=torch.float32, device=self.device))
        tokens, ntok, score = out
        check(self.lib.masr_transcribe_batch(self.h, _ptr(pcm), _ptr(n_samples), B, n_max,
                                             1 if use_db_normalization else 0, float(target_db),
                                             1 if decode_all_frames else 0, _ptr(tokens), _ptr(ntok), _ptr(score),
                                             _stream()))
        return tokens, ntok, score

    def transcribe_rows(self, samples, n_samples, use_db_normalization=True, target_db=-20.0, gain_in=None,
                        decode_all_frames=False, out=None):
        """The same pass with the facade's inputs (int16 PCM or float32 samples, optionally the caller's gains: the bit-exact
        route of ``host_gains``) and ONE packed int32 row per utterance out: rows [B, T' + 2] = tokens | count | score bits."""
        B, n_max = samples.shape
        fmt = {torch.int16: 0, torch.float32: 1}[samples.dtype]
        Tp = self.out_frames(1 + (n_max - 400) // 160)
        rows = out if out is not None else torch.empty(B, Tp + 2, dtype=torch.int32, device=self.device)
        mode = 0 if not use_db_normalization else (2 if gain_in is not None else 1)
        check(self.lib.masr_transcribe_rows(self.h, _ptr(samples), fmt, _ptr(n_samples), B, n_max, mode, float(target_db),
                                            _ptr(gain_in), 1 if decode_all_frames else 0, _ptr(rows), _stream()))
        return rows

    # ---- streaming ----------------------------------------------------------------------------------
    def stream_open(self, max_frames_out=0):
        sid = C.c_int32()
        check(self.lib.masr_stream_open(self.h, int(max_frames_out), C.byref(sid)))
        return sid.value

    def stream_reset(self, sid):
        check(self.lib.masr_stream_reset(self.h, sid))

    def stream_close(self, sid):
        check(self.lib.masr_stream_close(self.h, sid))

    def stream_set_history(self, sid, required_cache_size):
        """forward_chunk's required_cache_size for this stream: < 0 keep all cached keys, >= 0 at most that many (input-rate
        frames; Conformer, Squeezeformer and Efficient-Conformer)"""
        check(self.lib.masr_stream_set_history(self.h, sid, int(required_cache_size)))

    def stream_offset(self, sid):
        off = C.c_int32()
        check(self.lib.masr_stream_offset(self.h, sid, C.byref(off)))
        return off.value

    def encode_chunk(self, stream_ids, feats, want_probs=True, want_argmax=False, want_enc=False):
        """feats f32 [n, Tc, 80] (device) -> probs [n, Tc', V] (+ argmax/maxprob [n, Tc']).  ``want_enc=True`` (attention
        families): masr_encode_chunk_enc, and a fourth value comes back, the step's encoder rows [n, Tc', d_model] -- what the CTC
        head read; without the flag the call and the three values are what they were."""
        n, Tc, _ = feats.shape
        Tq = self.out_frames(Tc)
        ids = (C.c_int32 * n)(*stream_ids)
        probs = torch.empty(n, Tq, self.vocab_size, dtype=torch.float32, device=self.device) if want_probs else None
        idx = torch.empty(n, Tq, dtype=torch.int32, device=self.device) if want_argmax else None
        mp = torch.empty(n, Tq, dtype=torch.float32, device=self.device) if want_argmax else None
        if want_enc:
            enc = torch.empty(n, Tq, self.d_model, dtype=torch.float32, device=self.device)
            check(self.lib.masr_encode_chunk_enc(self.h, ids, n, _ptr(feats), Tc, _ptr(probs), _ptr(idx), _ptr(mp), _ptr(enc),
                                                 _stream()))
            return probs, idx, mp, enc
        check(self.lib.masr_encode_chunk(self.h, ids, n, _ptr(feats), Tc, _ptr(probs), _ptr(idx), _ptr(mp), _stream()))
        return probs, idx, mp

    def stream_export_cache(self, sid):
        if self.use_model == 'deepspeech2':       # (h, c), each [num_rnn_layers, 1, 1, rnn_size] like the reference state
            h = torch.zeros(self.num_blocks, 1, 1, self.d_model, dtype=torch.float32, device=self.device)
            c = torch.zeros_like(h)
            check(self.lib.masr_stream_export_cache(self.h, sid, _ptr(h), _ptr(c), _stream()))
            return h, c
        n = C.c_int32(0)
        check(self.lib.masr_stream_cache_len(self.h, sid, C.byref(n)))       # att_cache.size(2) of the reference after the last step
        t = n.value
        dk = self.d_model // self.heads
        att = torch.zeros(self.num_blocks, self.heads, t, 2 * dk, dtype=torch.float32, device=self.device)
        cnn = torch.zeros(self.num_blocks, 1, self.d_model, self.cnn_kernel - 1, dtype=torch.float32, device=self.device)
        check(self.lib.masr_stream_export_cache(self.h, sid, _ptr(att), _ptr(cnn), _stream()))
        return att, cnn

    # ---- attention decoder (second pass) -----------------------------------------------------------------
    def rescore(self, enc, enc_lens, hyps, hyp_lens, with_right=True):
        """masr_rescore on the current stream and the active lane: ``enc`` [B, T', d] (the encoder output of a pass), ``enc_lens``
        [B] int32 valid encoder frames, ``hyps`` [B, N, Lmax] int32 token ids, ``hyp_lens`` [B, N] int32 (all device tensors) ->
        (att, r_att) [B, N] float32 device tensors: the left and the right decoder's summed log-probabilities of every hypothesis
        (``with_right=False``: r_att is zero).  Nothing is waited for."""
        B, Tp, _ = enc.shape
        _, N, Lmax = hyps.shape
        att = torch.empty(B, N, dtype=torch.float32, device=self.device)
        r_att = torch.empty(B, N, dtype=torch.float32, device=self.device)
        check(self.lib.masr_rescore(self.h, _ptr(enc), _ptr(enc_lens), B, Tp, _ptr(hyps), _ptr(hyp_lens), N, Lmax,
                                    1 if with_right else 0, _ptr(att), _ptr(r_att), _stream()))
        return att, r_att

    def rescore_rows(self, rows, frame_row, n_frames, hyps, hyp_lens, with_right=True):
        """masr_rescore_rows on the current stream and the active lane: ``rescore`` over encoder frames that are not contiguous.
        ``rows`` [n_rows, d] float32 (a row pool), ``frame_row`` [B, Tmax] int64: frame t of utterance b is row ``frame_row[b, t]``
        (any order; entries behind ``n_frames[b]`` are never used; a number outside [0, n_rows) among the valid ones stands for a
        frame of zeros), ``n_frames`` [B] int32; ``hyps`` / ``hyp_lens`` / ``with_right`` and the (att, r_att) that come back as
        in ``rescore``, bit for bit what it gives on ``rows[frame_row]``.  Nothing is waited for."""
        n_rows, d = rows.shape
        B, Tmax = frame_row.shape
        _, N, Lmax = hyps.shape
        if not (rows.is_contiguous() and frame_row.is_contiguous() and hyps.is_contiguous() and rows.dtype == torch.float32
                and frame_row.dtype == torch.int64 and n_frames.dtype == torch.int32 and hyps.dtype == torch.int32
                and hyp_lens.dtype == torch.int32 and d == self.d_model):
            raise ValueError('rescore_rows: contiguous float32 rows [n_rows, d_model], int64 frame_row and int32 n_frames / hyps / '
                             'hyp_lens expected')
        att = torch.empty(B, N, dtype=torch.float32, device=self.device)
        r_att = torch.empty(B, N, dtype=torch.float32, device=self.device)
        check(self.lib.masr_rescore_rows(self.h, _ptr(rows), n_rows, _ptr(frame_row), _ptr(n_frames), B, Tmax, _ptr(hyps),
                                         _ptr(hyp_lens), N, Lmax, 1 if with_right else 0, _ptr(att), _ptr(r_att), _stream()))
        return att, r_att

    def op_decoder_scores(self, enc, enc_lens, hyps, hyp_lens, with_right=True):
        """masr_op_decoder_scores: the decoder's launches driven alone from HOST tables (``enc_lens`` [B], ``hyps`` [B, N, Lmax],
        ``hyp_lens`` [B, N]; ``enc`` [B, T', d] on the device), every entry validated -> (att, r_att) [B, N] numpy; returns when
        the work has finished."""
        hyps = np.ascontiguousarray(hyps, np.int32)
        hyp_lens = np.ascontiguousarray(hyp_lens, np.int32)
        enc_lens = np.ascontiguousarray(enc_lens, np.int32)
        B, N, Lmax = hyps.shape
        att, r_att = np.zeros((B, N), np.float32), np.zeros((B, N), np.float32)
        as_p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(self.lib.masr_op_decoder_scores(self.h, _ptr(enc), as_p(enc_lens), B, enc.shape[1], as_p(hyps), as_p(hyp_lens), N, Lmax,
                                              1 if with_right else 0, as_p(att), as_p(r_att), _stream()))
        return att, r_att

    def attention_decode(self, enc, enc_lens, beam_size=10, max_len=0, lcap=None):
        """masr_attention_decode on the current stream and the active lane: left-to-right beam search with the left decoder over
        ``enc`` [B, T', d] / ``enc_lens`` [B] int32 (device tensors) -> (tokens [B, N, Lcap] int32, lens [B, N] int32, scores
        [B, N] float32) device tensors, best hypothesis first, and the number of steps launched.  ``lcap`` (default: the most
        steps any utterance of the batch may run) bounds the hypotheses' length.  The host waits only at the end polls."""
        B, Tp, _ = enc.shape
        N, max_len = int(beam_size), int(max_len)
        if lcap is None:
            lcap = max(1, min(Tp, self.max_pos - 1, max_len if max_len > 0 else Tp))
        tokens = torch.empty(B, max(N, 1), max(int(lcap), 1), dtype=torch.int32, device=self.device)
        lens = torch.empty(B, max(N, 1), dtype=torch.int32, device=self.device)
        scores = torch.empty(B, max(N, 1), dtype=torch.float32, device=self.device)
        steps = C.c_int32(0)
        check(self.lib.masr_attention_decode(self.h, _ptr(enc), _ptr(enc_lens), B, Tp, N, max_len, _ptr(tokens), int(lcap), _ptr(lens),
                                             _ptr(scores), C.byref(steps), _stream()))
        return tokens, lens, scores, steps.value

    def joint_decode(self, enc, enc_lens, post, beam_size=10, ctc_candidates=None, ctc_weight=0.3, length_bonus=0.0, max_len=0,
                     lcap=None, input_is_log=False):
        """masr_joint_decode on the current stream and the active lane: the search of ``attention_decode`` ranked by
        J = ((1 - ctc_weight) A + ctc_weight psi) + length_bonus n over ``enc`` [B, T', d] / ``enc_lens`` [B] int32 with the CTC
        posteriors ``post`` [B, T', V] (``ctc_probs`` of the same pass, or any others; ``input_is_log=True``: log-probabilities;
        None is accepted with ``ctc_weight`` 0) -> (tokens [B, N, Lcap] int32, lens [B, N] int32, J [B, N], A [B, N], psi [B, N]
        float32) device tensors, best hypothesis first, and the number of steps launched.  ``ctc_candidates`` (default
        min(2 N, 64, V)): the attention candidates per hypothesis that are CTC-scored.  The host waits only at the end polls."""
        B, Tp, _ = enc.shape
        N, max_len = int(beam_size), int(max_len)
        M = min(2 * N, 64, self.vocab_size) if ctc_candidates is None else int(ctc_candidates)
        if post is not None and (tuple(post.shape) != (B, Tp, self.vocab_size) or post.dtype != torch.float32 or not post.is_contiguous()):
            raise ValueError(f'joint_decode: contiguous float32 posteriors [{B}, {Tp}, {self.vocab_size}] expected')
        if lcap is None:
            lcap = max(1, min(Tp, self.max_pos - 1, max_len if max_len > 0 else Tp))
        tokens = torch.empty(B, max(N, 1), max(int(lcap), 1), dtype=torch.int32, device=self.device)
        lens = torch.empty(B, max(N, 1), dtype=torch.int32, device=self.device)
        scores, att, psi = (torch.empty(B, max(N, 1), dtype=torch.float32, device=self.device) for _ in range(3))
        steps = C.c_int32(0)
        check(self.lib.masr_joint_decode(self.h, _ptr(enc), _ptr(enc_lens), B, Tp, _ptr(post), 1 if input_is_log else 0, N, M,
                                         float(ctc_weight), float(length_bonus), max_len, _ptr(tokens), int(lcap), _ptr(lens),
                                         _ptr(scores), _ptr(att), _ptr(psi), C.byref(steps), _stream()))
        return tokens, lens, scores, att, psi, steps.value

    def joint_decode_lm(self, enc, enc_lens, post, language_model=None, lm_weight=0.0, beam_size=10, ctc_candidates=None,
                        ctc_weight=0.3, length_bonus=0.0, max_len=0, lcap=None, input_is_log=False):
        """masr_joint_decode_lm: ``joint_decode`` with the n-gram ``language_model`` (decoders.lm_scorer.LanguageModel, or None)
        fused into the key, J = (((1 - ctc_weight) A + ctc_weight psi) + lm_weight Lm) + length_bonus n with Lm the float32 sum
        of the model's conditional log-probabilities of the hypothesis' tokens -> ``joint_decode``'s results with Lm [B, N]
        float32 behind psi: (tokens, lens, J, A, psi, Lm, steps).  ``lm_weight`` 0 launches nothing of the model and returns
        ``joint_decode``'s bits (Lm = 0)."""
        B, Tp, _ = enc.shape
        N, max_len = int(beam_size), int(max_len)
        M = min(2 * N, 64, self.vocab_size) if ctc_candidates is None else int(ctc_candidates)
        if post is not None and (tuple(post.shape) != (B, Tp, self.vocab_size) or post.dtype != torch.float32 or not post.is_contiguous()):
            raise ValueError(f'joint_decode_lm: contiguous float32 posteriors [{B}, {Tp}, {self.vocab_size}] expected')
        if lcap is None:
            lcap = max(1, min(Tp, self.max_pos - 1, max_len if max_len > 0 else Tp))
        tokens = torch.empty(B, max(N, 1), max(int(lcap), 1), dtype=torch.int32, device=self.device)
        lens = torch.empty(B, max(N, 1), dtype=torch.int32, device=self.device)
        scores, att, psi, lm = (torch.empty(B, max(N, 1), dtype=torch.float32, device=self.device) for _ in range(4))
        steps = C.c_int32(0)
        check(self.lib.masr_joint_decode_lm(self.h, _ptr(enc), _ptr(enc_lens), B, Tp, _ptr(post), 1 if input_is_log else 0, N, M,
                                            float(ctc_weight), float(length_bonus), language_model.h if language_model is not None else None,
                                            float(lm_weight), max_len, _ptr(tokens), int(lcap), _ptr(lens), _ptr(scores), _ptr(att),
                                            _ptr(psi), _ptr(lm), C.byref(steps), _stream()))
        return tokens, lens, scores, att, psi, lm, steps.value

    def lm_scores(self, language_model, prefixes, prefix_lens, cands):
        """masr_op_lm_scores: the LM score kernel of the joint search alone from HOST tables.  ``prefixes`` [R, L] token ids with
        ``prefix_lens`` [R] in 0 .. L, ``cands`` [R, M] candidate ids (vocab_size - 1 is scored as ``</s>``) -> [R, M] numpy
        float32, ``language_model.cond_log_prob(prefix + [candidate])`` bit for bit; returns when the work has finished."""
        prefixes = np.ascontiguousarray(prefixes, np.int32)
        prefix_lens = np.ascontiguousarray(prefix_lens, np.int32)
        cands = np.ascontiguousarray(cands, np.int32)
        if prefixes.ndim != 2 or cands.ndim != 2 or prefix_lens.shape != (prefixes.shape[0],) or cands.shape[0] != prefixes.shape[0]:
            raise ValueError('lm_scores: prefixes [R, L], prefix_lens [R] and cands [R, M] expected')
        R, L = prefixes.shape
        M = cands.shape[1]
        out = np.zeros((R, max(M, 1)), np.float32)
        as_p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(self.lib.masr_op_lm_scores(self.h, language_model.h if language_model is not None else None, as_p(prefixes),
                                         as_p(prefix_lens), as_p(cands), R, L, M, as_p(out), _stream()))
        return out

    def ctc_prefix_scores(self, post, frames, row_utt, prefixes, prefix_lens, cands, input_is_log=False):
        """masr_op_ctc_prefix_scores: the CTC prefix scorer driven alone from HOST tables.  ``post`` [B, T', V] on the device,
        ``frames`` [B] valid frames, and R rows: ``row_utt`` [R] utterance of the row, ``prefixes`` [R, L] with ``prefix_lens``
        [R] in 0 .. L (ids in 1 .. V - 2), ``cands`` [R, M] candidate ids -> (psi of every prefix [R], psi of every prefix
        extended by every candidate [R, M]) numpy float32; returns when the work has finished."""
        frames = np.ascontiguousarray(frames, np.int32)
        row_utt = np.ascontiguousarray(row_utt, np.int32)
        prefixes = np.ascontiguousarray(prefixes, np.int32)
        prefix_lens = np.ascontiguousarray(prefix_lens, np.int32)
        cands = np.ascontiguousarray(cands, np.int32)
        B, Tp, V = post.shape
        R, L = prefixes.shape
        M = cands.shape[1]
        if (V != self.vocab_size or post.dtype != torch.float32 or not post.is_contiguous() or frames.shape != (B,)
                or row_utt.shape != (R,) or prefix_lens.shape != (R,) or cands.shape != (R, M)):
            raise ValueError('ctc_prefix_scores: contiguous float32 posteriors [B, T\', vocab_size], frames [B], row_utt / '
                             'prefix_lens [R], prefixes [R, L] and cands [R, M] expected')
        psi, psi_c = np.zeros(R, np.float32), np.zeros((R, max(M, 1)), np.float32)
        as_p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(self.lib.masr_op_ctc_prefix_scores(self.h, _ptr(post), 1 if input_is_log else 0, as_p(frames), B, Tp, as_p(row_utt),
                                                 as_p(prefixes), as_p(prefix_lens), R, L, as_p(cands), M, as_p(psi), as_p(psi_c),
                                                 _stream()))
        return psi, psi_c

    def op_decoder_step(self, enc, enc_lens, prefixes, prefix_lens, top_n=1, want_logp=True):
        """masr_op_decoder_step: the decode step driven alone from HOST tables, teacher forced.  ``enc`` [B, T', d] on the device,
        ``enc_lens`` [B], ``prefixes`` [B, N, L] tokens behind sos, ``prefix_lens`` [B, N] in 0 .. L -> (top ids [B, N, top_n]
        int32, top log-probabilities [B, N, top_n], log-probabilities [B, N, V] or None) numpy, of the position behind each
        prefix; returns when the work has finished."""
        prefixes = np.ascontiguousarray(prefixes, np.int32)
        prefix_lens = np.ascontiguousarray(prefix_lens, np.int32)
        enc_lens = np.ascontiguousarray(enc_lens, np.int32)
        B, N, L = prefixes.shape
        top_n = int(top_n)
        ids = np.zeros((B, N, max(top_n, 1)), np.int32)
        top = np.zeros((B, N, max(top_n, 1)), np.float32)
        logp = np.zeros((B, N, self.vocab_size), np.float32) if want_logp else None
        as_p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(self.lib.masr_op_decoder_step(self.h, _ptr(enc), as_p(enc_lens), B, enc.shape[1], as_p(prefixes), as_p(prefix_lens), N, L,
                                            top_n, as_p(ids), as_p(top), as_p(logp) if want_logp else None, _stream()))
        return ids, top, logp

    def decoder_info(self):
        """masr_decoder_info -> {'enabled', 'num_blocks', 'r_num_blocks', 'weight_bytes', 'workspace_bytes' (active lane)}"""
        en, nl, nr, wb, ws = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        check(self.lib.masr_decoder_info(self.h, C.byref(en), C.byref(nl), C.byref(nr), C.byref(wb), C.byref(ws)))
        return {'enabled': bool(en.value), 'num_blocks': nl.value, 'r_num_blocks': nr.value, 'weight_bytes': wb.value,
                'workspace_bytes': ws.value}

    # ---- single ops / profiling -----------------------------------------------------------------------
    def op_layernorm(self, x, w, b, eps=1e-5):
        y = torch.empty_like(x)
        check(self.lib.masr_op_layernorm(self.h, _ptr(x), _ptr(w), _ptr(b), _ptr(y), x.numel() // x.shape[-1],
                                         float(eps), _stream()))
        return y

    def op_ctc_collapse_rows(self, idx, maxp, n_frames, in_rows=None, Tp=None, blank=0):
        """masr_op_ctc_collapse_rows: the packed-row collapse of ``transcribe_rows`` (``in_rows`` None: ``idx`` / ``maxp`` [B, Tp]) or
        of the pool step (``in_rows`` [B] int32: utterance b reads row ``in_rows[b]`` of the history matrices ``idx`` / ``maxp``
        [*, ld_in], ``Tp`` frames at the most) -> rows [B, Tp + 2] int32 = tokens | count | score bits"""
        B = n_frames.shape[0]
        ld_in = idx.shape[1]
        Tp = ld_in if Tp is None else int(Tp)
        rows = torch.empty(B, Tp + 2, dtype=torch.int32, device=self.device)
        check(self.lib.masr_op_ctc_collapse_rows(self.h, _ptr(idx), _ptr(maxp), _ptr(n_frames), _ptr(in_rows), ld_in, B, Tp, blank,
                                                 _ptr(rows), _stream()))
        return rows

    def op_gemm(self, a, w, bias=None, res=None, act=0, alpha=1.0):
        M, K = a.shape
        N = w.shape[0]
        c = torch.empty(M, N, dtype=torch.float32, device=self.device)
        check(self.lib.masr_op_gemm(self.h, _ptr(a), _ptr(w), _ptr(bias), _ptr(res), _ptr(c), M, N, K, int(act),
                                    float(alpha), _stream()))
        return c

    def op_attention(self, q, k, v, out, ptab, bias_u, bias_v, seqs, heads, q_stride, kv_stride, chunk_size=0, pos_stride=1,
                     group=1, t_true=0, positional=True):
        """masr_op_attention: one attention launch on the caller's device buffers, written into ``out`` in place.  ``seqs``: one
        dict per sequence with the element offsets ``q_off`` / ``k_off`` / ``v_off`` / ``out_off`` of its first rows from the
        buffers' pointers and ``nq``, ``nk``, ``klen``, ``pos0``, ``q_abs0``.  ``positional=False`` (masr_op_attention_plain): the
        plain attention of pos_enc_layer_type abs_pos / no_pos -- ``ptab``, ``bias_u``, ``bias_v`` and ``pos0`` are not used."""
        n = len(seqs)
        col = lambda name, ct: (ct * max(n, 1))(*[int(s[name]) for s in seqs])
        if not positional:
            if group != 1:
                raise _lib.MasrError('op_attention: the plain attention has no grouped form')
            check(self.lib.masr_op_attention_plain(
                self.h, _ptr(q), _ptr(k), _ptr(v), _ptr(out), n,
                col('q_off', C.c_int64), col('k_off', C.c_int64), col('v_off', C.c_int64), col('out_off', C.c_int64),
                col('nq', C.c_int32), col('nk', C.c_int32), col('klen', C.c_int32), col('q_abs0', C.c_int32),
                int(heads), int(q_stride), int(kv_stride), int(chunk_size), int(pos_stride), _stream()))
            return out
        check(self.lib.masr_op_attention(
            self.h, _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(ptab), ptab.shape[0], _ptr(bias_u), _ptr(bias_v), n,
            col('q_off', C.c_int64), col('k_off', C.c_int64), col('v_off', C.c_int64), col('out_off', C.c_int64),
            col('nq', C.c_int32), col('nk', C.c_int32), col('klen', C.c_int32), col('pos0', C.c_int32), col('q_abs0', C.c_int32),
            int(heads), int(q_stride), int(kv_stride), int(chunk_size), int(pos_stride), int(group), int(t_true), _stream()))
        return out

    def profile_select(self, kind):
        check(self.lib.masr_profile_select(self.h, int(kind)))

    def profile_read(self, reset=True):
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        check(self.lib.masr_profile_read(self.h, C.byref(ms), C.byref(n), C.byref(fl), 1 if reset else 0))
        return ms.value, n.value, fl.value
