"""ctypes binding of libmasr_hip.so (C ABI: include/masr_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or cannot be loaded this
module raises, and so does everything that imports it.
"""
import collections
import contextlib
import ctypes as C
import os

import numpy as _np

from .build import LIB_PATH

_lib = None


class MasrConfig(C.Structure):
    _fields_ = [('model_kind', C.c_int32), ('d_model', C.c_int32), ('heads', C.c_int32), ('d_ff', C.c_int32),
                ('num_blocks', C.c_int32), ('cnn_kernel', C.c_int32), ('n_mels', C.c_int32),
                ('vocab_size', C.c_int32), ('causal', C.c_int32), ('max_pos', C.c_int32), ('device_id', C.c_int32),
                ('reserved', C.c_int32 * 5)]


class MasrError(RuntimeError):
    pass


_P = C.c_void_p
_I = C.c_int32
_F = C.c_float

# name -> argtypes (restype is int unless listed in _RESTYPE); mirrors include/masr_hip.h one to one
SIGNATURES = {
    'masr_last_error': [],
    'masr_version': [],
    'masr_create': [C.POINTER(MasrConfig), C.POINTER(_P)],
    'masr_destroy': [_P],
    'masr_load_tensor': [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I],
    'masr_finalize': [_P, _P],
    'masr_fbank_batch': [_P, _P, _I, _P, _I, _I, _I, _F, _P, _P, _P, _P, _P],
    'masr_encode_full': [_P, _P, _P, _I, _I, _I, _P, _P],
    'masr_ctc_probs': [_P, _P, _I, _P, _P, _P, _P],
    'masr_ctc_greedy_frames': [_P, _P, _I, _P, _P, _P],
    'masr_ctc_collapse': [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P],
    'masr_argmax_rows': [_P, _P, _I, _I, _P, _P, _P],
    'masr_ctc_topk': [_P, _P, _I, _I, _I, _F, _P, _P, _P, _P],
    'masr_ctc_topk_blank': [_P, _P, _I, _I, _I, _F, _I, _P, _P, _P, _P, _P],
    'masr_beam_create': [_I, _I, C.POINTER(_P)],
    'masr_beam_destroy': [_P],
    'masr_beam_reset': [_P],
    'masr_beam_advance': [_P, _P, _P, _P, _I, _I],
    'masr_beam_advance_lm': [_P, _P, _P, _P, _P, _I, _I],
    'masr_beam_result': [_P, _P, _I, C.POINTER(_I), C.POINTER(_F)],
    'masr_beam_search_batch': [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P],
    'masr_beam_search_gpu': [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P],
    'masr_gbeam_open': [_P, _I, _I, _I, C.POINTER(_I)],
    'masr_gbeam_advance': [_P, _I, _P, _P, _P, _I, _I, _P, _I, _P, _P, _P],
    'masr_gbeam_advance_lm': [_P, _I, _P, _P, _P, _P, _I, _I, _P, _I, _P, _P, _P],
    'masr_gbeam_reset': [_P, _I],
    'masr_gbeam_close': [_P, _I],
    'masr_gbeam_set_lm': [_P, _I, _P, _F, _F],
    'masr_beam_set_lm': [_P, _P, _F, _F],
    'masr_beam_search_batch_lm': [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _F, _F, _P, _P, _I, _P, _P],
    'masr_beam_search_gpu_lm': [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _F, _F, _P, _P, _I, _P, _P, _P],
    'masr_lm_load_arpa': [C.c_char_p, C.POINTER(C.c_char_p), _I, C.POINTER(_P)],
    'masr_lm_destroy': [_P],
    'masr_lm_last_error': [],
    'masr_lm_info': [_P, C.POINTER(_I), C.POINTER(C.c_int64), C.POINTER(_I), C.POINTER(C.c_int64)],
    'masr_lm_cond_log_prob': [_P, C.POINTER(_I), _I, C.POINTER(_F)],
    'masr_lm_sentence_log_prob': [_P, C.POINTER(_I), _I, C.POINTER(_F)],
    'masr_lm_word_id': [_P, C.c_char_p, C.POINTER(_I)],
    'masr_lm_dict_size': [_P, C.POINTER(_I)],
    'masr_vad_create': [_I, C.POINTER(_P)],
    'masr_vad_destroy': [_P],
    'masr_vad_last_error': [],
    'masr_vad_load_tensor': [_P, _I, C.c_char_p, _P, C.c_int64],
    'masr_vad_finalize': [_P, _I],
    'masr_vad_forward': [_P, _I, _P, _I, _I, _I, _P, _P, _P, _P],
    'masr_mean_square': [_P, _P, _I, _P, _I, _I, _P, _P],
    'masr_mfcc_batch': [_P, _P, _I, _P, _I, _I, _I, _F, _I, _P, _P, _P, _P],
    'masr_linear_batch': [_P, _P, _I, _P, _I, _I, _I, _F, _P, _P, _P, _P],
    'masr_transcribe_batch': [_P, _P, _P, _I, _I, _I, _F, _I, _P, _P, _P, _P],
    'masr_transcribe_rows': [_P, _P, _I, _P, _I, _I, _I, _F, _P, _I, _P, _P],
    'masr_pool_create': [_P, _I, _I, _I, _F, _I, C.POINTER(_P)],
    'masr_pool_destroy': [_P],
    'masr_pool_open': [_P, C.POINTER(_I)],
    'masr_pool_close': [_P, _I],
    'masr_pool_reset': [_P, _I],
    'masr_pool_step': [_P, _I, _P, _P, _P, _P, _P, _P, _P, C.POINTER(_I), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P),
                       C.POINTER(_I), C.POINTER(_P), _P],
    'masr_pool_profile': [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64), _I],
    'masr_pool_window_plan': [_I, _I, C.POINTER(_I), _I, C.POINTER(_I)],
    'masr_encoder_frames': [_P, _I, C.POINTER(_I)],
    'masr_frame_reduction': [_P, C.POINTER(_I)],
    'masr_ctc_align': [_P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P],
    'masr_ctc_align_rows': [_P, _P, C.c_int64, _I, _I, _P, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P],
    'masr_engine_info': [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)],
    'masr_stream_open': [_P, _I, C.POINTER(_I)],
    'masr_stream_reset': [_P, _I],
    'masr_stream_close': [_P, _I],
    'masr_stream_offset': [_P, _I, C.POINTER(_I)],
    'masr_stream_cache_len': [_P, _I, C.POINTER(_I)],
    'masr_stream_room': [_P, _I, C.POINTER(_I)],
    'masr_resample_f32': [_P, C.c_int64, C.c_double, _P, _P, C.c_int64, _I, _P, C.c_int64],
    'masr_resample_rows': [_P, _P, _I, C.c_int64, _P, _P, _I, C.c_double, _P, C.c_int64, _I, _P, _I, C.c_int64, _P],
    'masr_resample_rate_fill': [C.c_double, _P, C.c_int64, _I, _P],
    'masr_resample_tile_span': [_P],
    'masr_resample_plan': [_P, _I, _P, _I, C.c_int64, _I, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(_I),
                           C.POINTER(C.c_char_p)],
    'masr_resample_feeds': [_P, _P, C.c_int64, _P, _P, _I, _P, _P, _I, _P, _P, C.c_int64, _P, _I, C.c_int64, _P],
    'masr_pool_set_rate': [_P, _I, C.c_double, _P, C.c_int64, _I, C.POINTER(_I)],
    'masr_pool_step_rates': [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(_I), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P),
                             C.POINTER(_I), C.POINTER(_P), _P],
    'masr_stream_set_history': [_P, _I, _I],
    'masr_encode_chunk': [_P, C.POINTER(_I), _I, _P, _I, _P, _P, _P, _P],
    'masr_encode_chunk_enc': [_P, C.POINTER(_I), _I, _P, _I, _P, _P, _P, _P, _P],
    'masr_stream_export_cache': [_P, _I, _P, _P, _P],
    'masr_op_layernorm': [_P, _P, _P, _P, _P, _I, _F, _P],
    'masr_op_gemm': [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    'masr_op_ctc_collapse_rows': [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P],
    'masr_op_attention': [_P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    'masr_op_attention_plain': [_P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    'masr_decoder_enable': [_P, _I, _I, _I, _I],
    'masr_rescore': [_P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P],
    'masr_rescore_rows': [_P, _P, C.c_int64, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P],
    'masr_op_decoder_scores': [_P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P],
    'masr_decoder_info': [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    'masr_attention_decode': [_P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _P, C.POINTER(_I), _P],
    'masr_op_decoder_step': [_P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P],
    'masr_joint_decode': [_P, _P, _P, _I, _I, _P, _I, _I, _I, _F, _F, _I, _P, _I, _P, _P, _P, _P, C.POINTER(_I), _P],
    'masr_op_ctc_prefix_scores': [_P, _P, _I, _P, _I, _I, _P, _P, _P, _I, _I, _P, _I, _P, _P, _P],
    'masr_joint_decode_lm': [_P, _P, _P, _I, _I, _P, _I, _I, _I, _F, _F, _P, _F, _I, _P, _I, _P, _P, _P, _P, _P, C.POINTER(_I), _P],
    'masr_op_lm_scores': [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P],
    'masr_beam_search_batch_nbest': [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P],
    'masr_beam_nbest_gpu': [_P, _I, _I, _I, _P, _F, _F, _P, _I, _P, _P, _P, _P],
    'masr_gbeam_nbest': [_P, _I, _I, _P, _I, _P, _P, _P, _P],
    'masr_op_beam_nbest': [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _P, _P],
    'masr_side_stream': [_P, _I, C.POINTER(_P)],
    'masr_select_lane': [_P, _I],
    'masr_stage_rows': [_P, C.c_int64, _P, _P, _I, _I, _I],
    'masr_debug_set': [_P, _I, _I],
    'masr_debug_reset': [_P],
    'masr_debug_key_info': [_I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(C.c_char_p)],
    'masr_ffn_plan': [_I, _I, _I, C.POINTER(_I), C.POINTER(_I), _I, C.POINTER(_I)],
    'masr_mfma_order_probe': [_P, _P, _P, _P, _I, _P, _P],
    'masr_profile_select': [_P, _I],
    'masr_profile_read': [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), _I],
}
_RESTYPE = {'masr_last_error': C.c_char_p, 'masr_destroy': None, 'masr_beam_destroy': None, 'masr_lm_destroy': None,
            'masr_lm_last_error': C.c_char_p, 'masr_vad_last_error': C.c_char_p, 'masr_vad_destroy': None, 'masr_pool_destroy': None,
            'masr_resample_tile_span': C.c_int64}

# masr_resample_feed / masr_resample_rate of include/masr_hip.h as numpy record layouts (32 / 48 bytes)
RESAMPLE_FEED = _np.dtype([('src_offset', '<i8'), ('format', '<i4'), ('n_in', '<i4'), ('n_out', '<i4'), ('dst_row', '<i4'),
                           ('dst_offset', '<i4'), ('rate_slot', '<i4')])
RESAMPLE_RATE = _np.dtype([('ratio', '<f8'), ('time_increment', '<f8'), ('scale', '<f8'), ('table_dev', '<u8'), ('index_step', '<i4'),
                           ('nwin', '<i4'), ('num_table', '<i4'), ('reserved', '<i4')])
RESAMPLE_TILE, RESAMPLE_LDS_FLOATS = 256, 16000


# int gain_fn(const float* mean_square, int32 n, float target_db, float* gain_out, void* user)
GAIN_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_float), C.c_int32, C.c_float, C.POINTER(C.c_float), C.c_void_p)


def lib():
    """Load (once) and return the ctypes handle.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64.so (same soname): import it FIRST so that this library binds
    # to the HIP runtime torch already loaded -- two runtimes in one process cannot both see the GPU
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise MasrError(f'{LIB_PATH} not found: build it with `python -m masr_amd.build` '
                        f'(hipcc --offload-arch=gfx950). There is no CPU fallback.')
    h = C.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        fn = getattr(h, name)          # AttributeError if a declared symbol is not exported
        fn.argtypes = args
        fn.restype = _RESTYPE.get(name, C.c_int)
    _lib = h
    return h


def check(rc):
    if rc != 0:
        raise MasrError(lib().masr_last_error().decode('utf-8', 'replace'))


# the three per-engine keys of masr_debug_set (include/masr_hip.h); every other key is a row of masr_debug_key_info
_ENGINE_KEYS = {'beam_profile': 2, 'prof_stride': 16, 'skip_padding': 38}


def debug_key_table():
    """[(key, name, default, experimental)]: the process-wide masr_debug_set switches, as masr_debug_key_info lists them"""
    rows = []
    key, default, experimental, name = _I(), _I(), _I(), C.c_char_p()
    while lib().masr_debug_key_info(len(rows), C.byref(key), C.byref(default), C.byref(experimental), C.byref(name)) == 0:
        rows.append((key.value, name.value.decode(), default.value, bool(experimental.value)))
    return rows


FFN_KERNELS = ('X3', 'COOP', 'DUAL', 'ROWS16', 'PC')      # FfnKernel of csrc/ffn_plan.h
FfnPlan = collections.namedtuple('FfnPlan', 'kernel nsplit cpb ny packed tail_in_kernel head_in_kernel split_head prof')


def ffn_plan(d_ff, M, keys=None, d_model=256, affine=0, tail_n=0, tail_planar=0, head_ktaps=0, head_norm=0):
    """masr_ffn_plan: the launch plan of one FFN call on M rows under the switch defaults with ``keys`` {key number: value} on top
    (no engine, no GPU, process state untouched); ``kernel`` comes back as its name"""
    ask = (_I * 5)(affine, tail_n, tail_planar, head_ktaps, head_norm)
    flat = [int(v) for kv in (keys or {}).items() for v in kv]
    out = (_I * 9)()
    check(lib().masr_ffn_plan(d_model, d_ff, M, ask, (_I * max(1, len(flat)))(*flat), len(flat) // 2, out))
    return FfnPlan(FFN_KERNELS[out[0]], *out[1:])


@contextlib.contextmanager
def debug_keys(eng, by_name=None, **more):
    """Set masr_debug_set switches by name for the body -- debug_keys(eng, ffn16=0) or debug_keys(eng, {'ffn16': 0}); a key of the
    dict may also be the switch's number.  Raises MasrError when the library refuses a key (unknown, or experimental in a product
    build).  On exit masr_debug_reset puts EVERY process-wide switch, and this engine's prof_stride and skip_padding, back to the
    default -- not to what held before -- so blocks do not nest: give all the keys of one measurement to one block."""
    numbers = dict(_ENGINE_KEYS, **{name: key for key, name, _, _ in debug_key_table()})
    try:
        for name, value in dict(by_name or {}, **more).items():
            if not isinstance(name, int) and name not in numbers:
                raise MasrError(f'debug_keys: no switch is named {name!r}')
            check(lib().masr_debug_set(eng.h, name if isinstance(name, int) else numbers[name], int(value)))
        yield
    finally:
        check(lib().masr_debug_reset(eng.h))
