"""ctypes binding of libvitsmi.so (include/vitsmi.h).  Fails loudly if the library is missing
or cannot be built: there is no CPU fallback on the product path."""
import ctypes as C
import os

import numpy as np

from . import audio_encoding

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

VITS_MAX_DIMS = 4


class VitsNoise(C.Structure):
    _fields_ = [("noise_dp", C.c_void_p), ("noise_z", C.c_void_p), ("noise_z_stride", C.c_int64),
                ("seed", C.c_uint64)]


class VitsOutput(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_float)), ("dims", C.c_int64 * 4), ("y_lengths", C.POINTER(C.c_int64))]


class VitsStats(C.Structure):
    _fields_ = [("conv_flops", C.c_double), ("conv_bytes", C.c_double), ("dec_flops", C.c_double),
                ("dec_bytes", C.c_double), ("flow_flops", C.c_double), ("enc_flops", C.c_double),
                ("dp_flops", C.c_double), ("conv_ms", C.c_float), ("dec_ms", C.c_float), ("flow_ms", C.c_float),
                ("enc_ms", C.c_float), ("dp_ms", C.c_float), ("total_ms", C.c_float), ("conv_launches", C.c_int),
                ("total_launches", C.c_int), ("sx_flops", C.c_double), ("sx_ms", C.c_float), ("sx_launches", C.c_int),
                ("f16_peak_max", C.c_float), ("f16_peak_min", C.c_float), ("f16_tracked", C.c_int),
                ("f16_saturated", C.c_int), ("sx_bytes", C.c_double)]


class VitsLaunchRecord(C.Structure):
    _fields_ = [("kernel", C.c_char * 128), ("flops", C.c_double), ("bytes", C.c_double), ("ms", C.c_float),
                ("stage", C.c_int), ("cin", C.c_int), ("cout", C.c_int), ("k", C.c_int), ("dil", C.c_int), ("t", C.c_int)]


class VitsTestConvEpiArgs(C.Structure):
    """vits_test_conv_epi_args of include/vitsmi.h"""
    _fields_ = [(n, C.c_int) for n in ("B", "Cin", "T", "Cout", "K", "dil", "pad_l", "stride", "hint", "cfg", "ck", "flags")] + \
               [(n, C.c_float) for n in ("slope", "div", "oslope", "oslope2")] + [("wn_split", C.c_int)] + \
               [(n, C.c_void_p) for n in ("x", "w", "bias", "lens", "bias_b")] + [("bias_b_stride", C.c_int), ("res", C.c_void_p)] + \
               [(n, C.c_int) for n in ("x_cstride", "out_cstride", "out_rows", "out_row0")] + \
               [("old_out", C.c_void_p), ("old_out2", C.c_void_p), ("sentinel", C.c_float), ("out", C.c_void_p), ("out2", C.c_void_p),
                ("pl_rows", C.c_int), ("planes_out", C.c_void_p), ("kernel", C.c_char * 128), ("cfg_used", C.c_int), ("ck_used", C.c_int)]


class VitsTestConvSxEpiArgs(C.Structure):
    """vits_test_conv_sx_epi_args of include/vitsmi.h"""
    _fields_ = [(n, C.c_int) for n in ("B", "Cin", "T", "Cout", "K", "dil", "pad_l", "stride", "precision", "force16", "no_s16",
                                       "min_cfg", "run_cfg", "flags")] + \
               [(n, C.c_void_p) for n in ("x", "w", "bias", "res")] + \
               [("res_is_x", C.c_int), ("res_planes", C.c_int), ("res_slope", C.c_float), ("old_out", C.c_void_p),
                ("bias_b", C.c_void_p), ("bias_b_stride", C.c_int)] + \
               [(n, C.c_float) for n in ("div", "oslope", "oslope2", "islope")] + \
               [("lens", C.c_void_p), ("rag_add", C.c_int), ("rag_mul", C.c_int), ("sentinel", C.c_float), ("out", C.c_void_p),
                ("planes_out", C.c_void_p), ("res_seen", C.c_void_p), ("kernel", C.c_char * 128)] + \
               [(n, C.c_int) for n in ("pack_cfg", "run_cfg_used", "rawin", "s16", "ck")] + [("peak", C.c_float)]


class VitsTestConvPair16EpiArgs(C.Structure):
    """vits_test_conv_pair16_epi_args of include/vitsmi.h"""
    _fields_ = [(n, C.c_int) for n in ("B", "C", "T", "K", "dil1", "dil2", "chain", "precision", "flags")] + \
               [(n, C.c_float) for n in ("slope", "div", "sentinel")] + \
               [(n, C.c_void_p) for n in ("x", "w1", "b1", "w2", "b2", "old_out", "x_tail", "lens")] + \
               [("rag_add", C.c_int), ("rag_mul", C.c_int)] + \
               [(n, C.c_void_p) for n in ("out", "planes_out", "x_seen", "ms_out")] + [("kernel", C.c_char * 128)] + \
               [(n, C.c_int) for n in ("BN", "BNo", "ovl")] + [("peak", C.c_float), ("guard_ok", C.c_int)]


class VitsTestConvPairSxEpiArgs(C.Structure):
    """vits_test_conv_pair_sx_epi_args of include/vitsmi.h"""
    _fields_ = [(n, C.c_int) for n in ("B", "C", "T", "K", "dil1", "dil2", "chain", "flags")] + \
               [(n, C.c_float) for n in ("slope", "div")] + \
               [(n, C.c_void_p) for n in ("x", "w1", "b1", "w2", "b2", "lens", "out_init", "out")] + \
               [("kernel", C.c_char * 128), ("BNo", C.c_int)]


class VitsTestAttentionFormArgs(C.Structure):
    """vits_test_attention_form_args of include/vitsmi.h"""
    _fields_ = [("kernel", C.c_int), ("qkv", C.c_void_p), ("qkv_planes", C.c_void_p)] + \
               [(n, C.c_int) for n in ("B", "C", "T", "n_heads", "window")] + \
               [(n, C.c_void_p) for n in ("rel_k", "rel_v", "lens")] + \
               [(n, C.c_int) for n in ("want_out", "want_planes", "ns", "qt", "kh")] + \
               [("out", C.c_void_p), ("out_planes", C.c_void_p), ("peak", C.c_float), ("kernel_name", C.c_char * 128)]


class VitsOpenOptions(C.Structure):
    _fields_ = [("device_id", C.c_int), ("gen_precision", C.c_char_p), ("arena_dev", C.c_void_p),
                ("arena_bytes", C.c_size_t), ("host_only", C.c_int), ("layout_only", C.c_int)]


class VitsControls(C.Structure):
    _fields_ = [("scales_rows", C.c_void_p), ("seeds", C.c_void_p), ("durations", C.c_void_p), ("token_rate", C.c_void_p)]


class VitsFit(C.Structure):
    """vits_fit (vitsmi.h, "fitted durations"): group int32 [B], target_frames int64 [n_groups], mode int32 [n_groups]"""
    _fields_ = [("group", C.c_void_p), ("n_groups", C.c_int), ("target_frames", C.c_void_p), ("mode", C.c_void_p)]


VITS_FIT_MET, VITS_FIT_FLOOR, VITS_FIT_CEIL, VITS_FIT_KEPT = 0, 1, 2, 3


class VitsWarpSeg(C.Structure):
    """vits_warp_seg: one token's segment of a warped row (vitsmi.h, "intonation"); 40 bytes"""
    _fields_ = [("n0", C.c_int64), ("pos0", C.c_int64), ("k", C.c_int64), ("step", C.c_int32), ("c", C.c_int32),
                ("half_taps", C.c_int32), ("pad_", C.c_int32)]


class VitsIntonation(C.Structure):
    _fields_ = [("token_semitones", C.c_void_p), ("compensate", C.c_int)]


class VitsGlideSeg(C.Structure):
    """vits_glide_seg: one token's segment of a row with glides (vitsmi.h, "pitch contours"); 40 bytes"""
    _fields_ = [("n0", C.c_int64), ("pos0", C.c_int64), ("k", C.c_int64), ("step0", C.c_int32), ("step1", C.c_int32),
                ("pad_", C.c_int32 * 2)]


class VitsContour(C.Structure):
    _fields_ = [("token_semitones", C.c_void_p), ("token_semitones_end", C.c_void_p), ("compensate", C.c_int)]


class VitsSegment(C.Structure):
    _fields_ = [("row", C.c_int32), ("stream", C.c_int32), ("lead_samples", C.c_int64), ("normalize", C.c_int32),
                ("volume", C.c_float)]


class VitsTrim(C.Structure):
    _fields_ = [("mode", C.c_int32), ("threshold", C.c_float), ("keep_lead", C.c_int32), ("keep_tail", C.c_int32),
                ("tail_samples", C.c_int64)]


class VitsTestDdsLayer(C.Structure):
    _fields_ = [("dw_w", C.c_void_p), ("dw_b", C.c_void_p), ("ln1_g", C.c_void_p), ("ln1_b", C.c_void_p), ("pw_w", C.c_void_p),
                ("pw_b", C.c_void_p), ("ln2_g", C.c_void_p), ("ln2_b", C.c_void_p), ("dil", C.c_int32)]


class VitsLevel(C.Structure):
    _fields_ = [("mode", C.c_int32), ("target_lufs", C.c_float), ("max_gain_db", C.c_float), ("peak_ceiling", C.c_float)]


class VitsEnvPoint(C.Structure):
    _fields_ = [("pos", C.c_int32), ("gain", C.c_float)]


class VitsShape(C.Structure):
    _fields_ = [("fade_in", C.c_int32), ("fade_out", C.c_int32), ("curve", C.c_int32), ("n_points", C.c_int32),
                ("first_point", C.c_int64)]


class VitsLimit(C.Structure):
    _fields_ = [("mode", C.c_int32), ("ceiling", C.c_float), ("lookahead", C.c_int32), ("reserved", C.c_int32)]


class VitsStreamFormat(C.Structure):
    _fields_ = [("encoding", C.c_int32), ("ref_peak", C.c_void_p), ("volume", C.c_void_p)]


class VitsStreamShaping(C.Structure):
    pass


# int fn(void *user, int B, int T, const int64 *durations, const int64 *sample_counts, vits_stream_shaping *inout)
STREAM_PLAN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(VitsStreamShaping))

VitsStreamShaping._fields_ = [("shapes", C.c_void_p), ("points", C.c_void_p), ("n_points", C.c_int64), ("ceiling", C.c_void_p),
                              ("lookahead", C.c_int32), ("reserved", C.c_int32), ("plan", STREAM_PLAN_FN), ("plan_user", C.c_void_p)]


class VitsStreamOnset(C.Structure):
    _fields_ = [("mode", C.c_int32), ("threshold", C.c_float), ("keep_lead", C.c_int32), ("reserved", C.c_int32)]


# name -> (VITS_ENC_* code, element type): audio_encoding lists the names in the order of the header's enum
ENCODINGS = {name: (code, audio_encoding.DTYPES[name]) for code, name in enumerate(audio_encoding.ENCODINGS)}


# int fn(void *user, const float *samples, int B, int64 first_sample, int64 n_samples, int64 total_samples)
CHUNK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int64, C.c_int64, C.c_int64)

# int fn(void *user, const void *bytes, int B, int64 row_pitch_bytes, int64 first_sample, int64 n_samples,
#        const int32 *valid, const float *peak, int64 total_samples)
ENC_CHUNK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32),
                           C.POINTER(C.c_float), C.c_int64)

# ENC_CHUNK_FN with `const int32 *skip` behind valid
ENC_CHUNK_TRIM_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32),
                                C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int64)

VITS_E_RANGE = -6


EXPORTS = [
    "vits_open", "vits_open_with_arena", "vits_open_host", "vits_open_layout", "vits_open_opts", "vits_close",
    "vits_run_chunked", "vits_run_vocoder_chunked", "vits_last_error", "vits_num_inputs",
    "vits_input_name", "vits_meta", "vits_hparam", "vits_arena_bytes", "vits_arena_host", "vits_arena_device",
    "vits_run", "vits_free_output", "vits_run_device", "vits_sync", "vits_last_y_lengths", "vits_last_pcm16", "vits_run_vocoder",
    "vits_tap",
    "vits_set_timing", "vits_set_tails", "vits_reserve", "vits_get_stats", "vits_stream", "vits_test_conv1d", "vits_test_conv_transpose1d",
    "vits_test_attention", "vits_test_attention16", "vits_bench_conv1d", "vits_test_conv1d_sx", "vits_test_conv1d_sx_planar", "vits_test_conv1d_sx_gate", "vits_test_set_sx_small_max",
    "vits_test_conv_transpose1d_sx",
    "vits_bench_conv1d_sx", "vits_test_conv_pair_sx", "vits_fetch_output", "vits_run_async", "vits_host_alloc", "vits_host_free",
    "vits_launch_records", "vits_run_async_rows", "vits_run_device_rows", "vits_run_chunked_rows",
    "vits_run_async_ctl", "vits_run_chunked_ctl", "vits_last_durations",
    "vits_set_output_rate", "vits_last_sample_counts", "vits_resample_plan", "vits_test_resample", "vits_test_resample_pieces",
    "vits_set_output_rates", "vits_last_sample_rates", "vits_test_resample_rows",
    "vits_run_async_warped", "vits_last_token_spans", "vits_warp_token", "vits_warp_plan", "vits_test_warp",
    "vits_run_async_glided", "vits_glide_token", "vits_glide_cutoff", "vits_glide_plan", "vits_test_glide",
    "vits_warp_emit_end", "vits_glide_emit_end", "vits_warp_stream_cap", "vits_run_chunked_glided", "vits_run_chunked_enc_glided",
    "vits_test_warp_pieces", "vits_test_glide_pieces",
    "vits_set_pitch_at_rate", "vits_warp_token_rate", "vits_warp_plan_rate", "vits_glide_plan_rate", "vits_glide_cutoff_rate", "vits_glide_pos_rate",
    "vits_rate_identity_spans", "vits_test_warp_rate", "vits_test_glide_rate",
    "vits_warp_emit_end_rate", "vits_glide_emit_end_rate", "vits_identity_emit_end_rate", "vits_warp_stream_cap_rate",
    "vits_test_warp_rate_pieces", "vits_test_glide_rate_pieces",
    "vits_fit_plan", "vits_run_async_fitted", "vits_run_chunked_fitted", "vits_run_chunked_enc_fitted", "vits_last_fit",
    "vits_test_fit_durations",
    "vits_test_durations", "vits_test_expand_prior", "vits_test_fill_normal", "vits_test_fill_normal_rows", "vits_test_post_conv",
    "vits_delivery_plan", "vits_deliver", "vits_test_deliver",
    "vits_trim_range", "vits_delivery_plan_trimmed", "vits_deliver_trimmed", "vits_test_deliver_trimmed",
    "vits_loudness_filter", "vits_loudness_gate", "vits_level_gain", "vits_delivery_plan_leveled", "vits_deliver_leveled",
    "vits_test_loudness_blocks", "vits_test_deliver_leveled",
    "vits_shape_check", "vits_shape_gain", "vits_deliver_shaped", "vits_test_deliver_shaped",
    "vits_limit_check", "vits_limit_gains", "vits_deliver_limited", "vits_test_deliver_limited",
    "vits_run_chunked_enc", "vits_run_vocoder_chunked_enc", "vits_test_stream_pack",
    "vits_stream_shaping_check", "vits_stream_emit_range", "vits_run_chunked_enc_shaped", "vits_run_vocoder_chunked_enc_shaped",
    "vits_test_stream_pack_shaped",
    "vits_stream_onset_check", "vits_stream_onset_start", "vits_run_chunked_enc_trimmed", "vits_run_vocoder_chunked_enc_trimmed",
    "vits_test_stream_pack_trimmed",
    "vits_test_layernorm", "vits_test_dds", "vits_test_cf_pre", "vits_test_rqs_inverse", "vits_test_ea_logw",
    "vits_test_conv1d_epi", "vits_test_wn_gate", "vits_test_cond_matvec", "vits_test_conv1d_sx_epi",
    "vits_test_conv_pair16_epi", "vits_test_attention_form", "vits_test_conv_pair_sx_epi", "vits_test_split_forms", "vits_test_split_identity", "vits_test_split_identity_sweep",
]


G2P_EXPORTS = ["g2p_open", "g2p_close", "g2p_last_error", "g2p_hparam", "g2p_num_outputs", "g2p_output_name", "g2p_bucket",
               "g2p_run", "g2p_generate", "g2p_generate_batch", "g2p_test_forced_steps", "g2p_test_linear", "g2p_test_step",
               "g2p_test_attention", "g2p_test_rmsnorm", "g2p_test_argmax"]


def lib_path():
    # VITSMI_LIB: another build of the library (kernel experiments: variants compiled with -D switches side by side)
    return os.environ.get("VITSMI_LIB") or os.path.join(_HERE, "libvitsmi.so")


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.environ.get("VITSMI_LIB"):
        # the in-tree library must be the build of the in-tree sources: compared by content hash (_build_info.json, written
        # by phoonnx_amd/build.py), rebuilt when it is not - or, without a compiler, refused: never a stale binary
        from . import build as _build
        if _build.stale():
            try:
                _build.build()
            except Exception as e:
                raise RuntimeError(f"{path} is missing or was not built from the sources in this tree (source_sha "
                                   f"{_build.source_sha()} vs recorded {_build.read_build_info().get('source_sha')}) "
                                   f"and cannot be rebuilt here: {e}") from e
    lib = C.CDLL(path)
    vp, i64p, f32p = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_float)
    lib.vits_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    lib.vits_open_with_arena.argtypes = [C.c_char_p, C.c_int, vp, C.c_size_t, C.POINTER(vp)]
    lib.vits_open_host.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.vits_open_layout.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.vits_open_opts.argtypes = [C.c_char_p, C.POINTER(VitsOpenOptions), C.POINTER(vp)]
    lib.vits_run_chunked.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, C.POINTER(VitsNoise), C.c_int, CHUNK_FN, vp]
    lib.vits_run_vocoder_chunked.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, CHUNK_FN, vp]
    lib.vits_close.argtypes = [vp]
    lib.vits_close.restype = None
    lib.vits_last_error.argtypes = [vp]
    lib.vits_last_error.restype = C.c_char_p
    lib.vits_num_inputs.argtypes = [vp]
    lib.vits_input_name.argtypes = [vp, C.c_int]
    lib.vits_input_name.restype = C.c_char_p
    lib.vits_meta.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_size_t]
    lib.vits_hparam.argtypes = [vp, C.c_char_p, i64p]
    lib.vits_arena_bytes.argtypes = [vp]
    lib.vits_arena_bytes.restype = C.c_size_t
    lib.vits_arena_host.argtypes = [vp]
    lib.vits_arena_host.restype = vp
    lib.vits_arena_device.argtypes = [vp]
    lib.vits_arena_device.restype = vp
    run_args = [vp, vp, vp, C.c_int, C.c_int, vp, vp, C.POINTER(VitsNoise), C.POINTER(VitsOutput)]
    lib.vits_run.argtypes = run_args
    lib.vits_run_device.argtypes = run_args
    lib.vits_run_async.argtypes = run_args[:-1]
    # (row twins: scales host float32 [B][3], then a host uint64 [B] of seeds or NULL behind the noise)
    lib.vits_run_async_rows.argtypes = run_args[:-1] + [vp]
    lib.vits_run_device_rows.argtypes = run_args[:-1] + [vp, C.POINTER(VitsOutput)]
    lib.vits_run_chunked_rows.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, C.POINTER(VitsNoise), vp, C.c_int, CHUNK_FN, vp]
    # (controls twins: ids, lens, B, T, sid, noise, then the vits_controls struct in the place of scales / seeds)
    lib.vits_run_async_ctl.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsNoise), C.POINTER(VitsControls)]
    lib.vits_run_chunked_ctl.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsNoise), C.POINTER(VitsControls),
                                         C.c_int, CHUNK_FN, vp]
    # (encoded twins: the vits_stream_format struct in front of chunk_frames, the encoded callback type)
    lib.vits_run_chunked_enc.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsNoise), C.POINTER(VitsControls),
                                         C.POINTER(VitsStreamFormat), C.c_int, ENC_CHUNK_FN, vp]
    lib.vits_run_vocoder_chunked_enc.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsStreamFormat), C.c_int, ENC_CHUNK_FN, vp]
    lib.vits_stream_shaping_check.argtypes = [C.POINTER(VitsStreamShaping), C.POINTER(VitsStreamFormat), C.c_int]
    lib.vits_stream_emit_range.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int, i64p, i64p]
    lib.vits_run_chunked_enc_shaped.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsNoise), C.POINTER(VitsControls),
                                                C.POINTER(VitsStreamFormat), C.POINTER(VitsStreamShaping), C.c_int, ENC_CHUNK_FN, vp]
    lib.vits_run_vocoder_chunked_enc_shaped.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsStreamFormat),
                                                        C.POINTER(VitsStreamShaping), C.c_int, ENC_CHUNK_FN, vp]
    lib.vits_test_stream_pack_shaped.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(VitsStreamFormat),
                                                 C.POINTER(VitsStreamShaping), vp, C.c_size_t, vp, vp, vp, vp, vp, C.c_int]
    lib.vits_stream_onset_check.argtypes = [C.POINTER(VitsStreamOnset), C.POINTER(VitsStreamFormat), C.c_int]
    lib.vits_stream_onset_start.argtypes = [C.c_int64, C.c_int64, C.c_int64, i64p]
    lib.vits_run_chunked_enc_trimmed.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsNoise), C.POINTER(VitsControls),
                                                 C.POINTER(VitsStreamFormat), C.POINTER(VitsStreamShaping), C.POINTER(VitsStreamOnset),
                                                 C.c_int, ENC_CHUNK_TRIM_FN, vp]
    lib.vits_run_vocoder_chunked_enc_trimmed.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsStreamFormat),
                                                         C.POINTER(VitsStreamShaping), C.POINTER(VitsStreamOnset), C.c_int,
                                                         ENC_CHUNK_TRIM_FN, vp]
    lib.vits_test_stream_pack_trimmed.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(VitsStreamFormat),
                                                  C.POINTER(VitsStreamShaping), C.POINTER(VitsStreamOnset), vp, C.c_size_t, vp, vp, vp, vp,
                                                  vp, vp, vp, C.c_int]
    lib.vits_test_stream_pack.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(VitsStreamFormat), vp, C.c_size_t,
                                          vp, vp, vp, C.c_int]
    lib.vits_last_durations.argtypes = [vp, i64p, C.c_size_t]
    lib.vits_set_output_rate.argtypes = [vp, C.c_int, C.c_int]
    lib.vits_last_sample_counts.argtypes = [vp, i64p, C.c_int]
    lib.vits_resample_plan.argtypes = [C.c_int, C.c_int, i64p, i64p, i64p, vp, C.c_size_t]
    lib.vits_test_resample.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int64]
    lib.vits_test_resample_pieces.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp, C.c_int]
    lib.vits_set_output_rates.argtypes = [vp, C.c_int, vp, C.c_int]
    lib.vits_last_sample_rates.argtypes = [vp, vp, C.c_int]
    lib.vits_test_resample_rows.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_size_t, vp]
    lib.vits_run_async_warped.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsNoise), C.POINTER(VitsControls),
                                          C.POINTER(VitsIntonation)]
    lib.vits_last_token_spans.argtypes = [vp, i64p, C.c_size_t]
    lib.vits_warp_token.argtypes = [C.c_float, i64p, i64p, C.POINTER(C.c_int32)]
    lib.vits_warp_plan.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, i64p]
    lib.vits_test_warp.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int]
    lib.vits_run_async_glided.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsNoise), C.POINTER(VitsControls),
                                          C.POINTER(VitsContour)]
    lib.vits_glide_token.argtypes = [C.c_float, C.c_float, i64p, i64p, C.POINTER(C.c_float)]
    lib.vits_glide_cutoff.argtypes = [C.c_int64, i64p, C.POINTER(C.c_int32)]
    lib.vits_glide_plan.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, i64p]
    lib.vits_test_glide.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int]
    for name in ("vits_warp_emit_end", "vits_glide_emit_end"):
        getattr(lib, name).argtypes = [vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, i64p]
    lib.vits_warp_stream_cap.argtypes = [C.c_int64, C.c_int64]
    lib.vits_warp_stream_cap.restype = C.c_int64
    lib.vits_run_chunked_glided.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsNoise), C.POINTER(VitsControls),
                                            C.POINTER(VitsContour), C.c_int, CHUNK_FN, vp]
    lib.vits_run_chunked_enc_glided.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsNoise), C.POINTER(VitsControls),
                                                C.POINTER(VitsStreamFormat), C.POINTER(VitsStreamShaping), C.POINTER(VitsStreamOnset),
                                                C.POINTER(VitsContour), C.c_int, ENC_CHUNK_TRIM_FN, vp]
    for name in ("vits_test_warp_pieces", "vits_test_glide_pieces"):
        getattr(lib, name).argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp, C.c_int]
    lib.vits_set_pitch_at_rate.argtypes = [vp, C.c_int]
    lib.vits_warp_token_rate.argtypes = [C.c_float, C.c_int64, C.c_int64, i64p, i64p, C.POINTER(C.c_int32)]
    lib.vits_warp_plan_rate.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int64, C.c_int64, vp, vp, i64p]
    lib.vits_glide_plan_rate.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int64, C.c_int64, vp, vp, i64p]
    lib.vits_glide_cutoff_rate.argtypes = [C.c_int64, i64p, C.POINTER(C.c_int32)]
    lib.vits_glide_pos_rate.argtypes = [vp, C.c_int64, i64p, i64p]
    lib.vits_rate_identity_spans.argtypes = [vp, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, vp, i64p]
    for name in ("vits_warp_emit_end_rate", "vits_glide_emit_end_rate"):
        getattr(lib, name).argtypes = [vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int, i64p]
    lib.vits_identity_emit_end_rate.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, i64p]
    lib.vits_warp_stream_cap_rate.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int]
    lib.vits_warp_stream_cap_rate.restype = C.c_int64
    for name in ("vits_test_warp_rate_pieces", "vits_test_glide_rate_pieces"):
        getattr(lib, name).argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int]
    for name in ("vits_test_warp_rate", "vits_test_glide_rate"):
        getattr(lib, name).argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, vp]
    lib.vits_fit_plan.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(VitsFit), vp, vp, vp, vp]
    lib.vits_run_async_fitted.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsNoise), C.POINTER(VitsControls),
                                          C.POINTER(VitsFit)]
    lib.vits_run_chunked_fitted.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsNoise), C.POINTER(VitsControls),
                                            C.POINTER(VitsFit), C.c_int, CHUNK_FN, vp]
    lib.vits_run_chunked_enc_fitted.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsNoise), C.POINTER(VitsControls),
                                                C.POINTER(VitsStreamFormat), C.POINTER(VitsStreamShaping), C.POINTER(VitsStreamOnset),
                                                C.POINTER(VitsFit), C.c_int, ENC_CHUNK_TRIM_FN, vp]
    lib.vits_last_fit.argtypes = [vp, vp, vp, vp, C.c_int]
    lib.vits_test_fit_durations.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.POINTER(VitsFit), vp, vp, vp, vp, vp, vp]
    lib.vits_test_durations.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_float, vp, vp, vp, vp, vp]
    lib.vits_test_expand_prior.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int64, C.c_int,
                                           C.c_float, vp, vp, vp]
    lib.vits_test_fill_normal.argtypes = [C.c_int, C.c_int64, C.c_uint64, C.c_uint64, vp]
    lib.vits_test_fill_normal_rows.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_uint32, vp, C.c_int, vp]
    lib.vits_test_post_conv.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_float, vp, C.c_int, C.c_int, vp]
    lib.vits_test_layernorm.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp,
                                        C.c_int, C.c_int, vp, vp]
    lib.vits_test_dds.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.POINTER(VitsTestDdsLayer), C.c_int,
                                  vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp]
    lib.vits_test_cf_pre.argtypes = [C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.vits_test_rqs_inverse.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_float, vp]
    lib.vits_test_ea_logw.argtypes = [C.c_int, vp, C.c_int, C.c_float, C.c_float, vp, C.c_int, C.c_int, vp]
    lib.vits_delivery_plan.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, i64p]
    lib.vits_deliver.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp, vp]
    lib.vits_test_deliver.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp, vp]
    lib.vits_trim_range.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.POINTER(VitsTrim), i64p, i64p]
    lib.vits_delivery_plan_trimmed.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, i64p]
    lib.vits_deliver_trimmed.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp]
    lib.vits_test_deliver_trimmed.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t,
                                              vp, vp, vp, vp]
    lib.vits_loudness_filter.argtypes = [C.c_int, vp, vp]
    lib.vits_loudness_gate.argtypes = [vp, vp, C.c_int, C.c_int32, vp, vp, vp, vp]
    lib.vits_level_gain.argtypes = [C.c_double, C.c_float, C.POINTER(VitsLevel), C.POINTER(C.c_float)]
    lib.vits_delivery_plan_leveled.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, i64p]
    lib.vits_deliver_leveled.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
    lib.vits_test_loudness_blocks.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp, vp]
    lib.vits_test_deliver_leveled.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp,
                                              C.c_size_t, vp, vp, vp, vp, vp, vp]
    lib.vits_shape_check.argtypes = [vp, C.c_int, vp, C.c_int64]
    lib.vits_shape_gain.argtypes = [C.POINTER(VitsShape), vp, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_float)]
    lib.vits_deliver_shaped.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp,
                                        vp, vp, vp]
    lib.vits_test_deliver_shaped.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_int,
                                             C.c_int, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
    lib.vits_limit_check.argtypes = [vp, vp, C.c_int]
    lib.vits_limit_gains.argtypes = [vp, C.c_int64, C.POINTER(VitsLimit), vp]
    lib.vits_deliver_limited.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp,
                                         vp, vp, vp, vp, vp]
    lib.vits_test_deliver_limited.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int64, vp, C.c_int, C.c_int,
                                              C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
    lib.vits_free_output.argtypes = [vp, C.POINTER(VitsOutput)]
    lib.vits_free_output.restype = None
    lib.vits_sync.argtypes = [vp]
    lib.vits_last_y_lengths.argtypes = [vp, i64p, C.c_int]
    lib.vits_last_pcm16.argtypes = [vp, C.c_int, C.c_float, vp, C.c_size_t]
    lib.vits_run_vocoder.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.POINTER(VitsOutput)]
    lib.vits_tap.argtypes = [vp, C.c_char_p, vp, C.c_size_t, i64p]
    lib.vits_set_timing.argtypes = [vp, C.c_int]
    lib.vits_set_tails.argtypes = [vp, C.c_int]
    lib.vits_reserve.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.vits_get_stats.argtypes = [vp, C.POINTER(VitsStats)]
    lib.vits_stream.argtypes = [vp]
    lib.vits_stream.restype = vp
    lib.vits_fetch_output.argtypes = [vp, vp, C.c_size_t, C.c_size_t]
    lib.vits_host_alloc.argtypes = [C.c_size_t]
    lib.vits_host_alloc.restype = vp
    lib.vits_host_free.argtypes = [vp]
    lib.vits_host_free.restype = None
    lib.vits_launch_records.argtypes = [vp, C.POINTER(VitsLaunchRecord), C.c_int]
    lib.vits_test_conv1d.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_float, vp]
    lib.vits_test_conv_transpose1d.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int,
                                               C.c_int, vp]
    lib.vits_test_attention.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]
    lib.vits_test_attention16.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp,
                                          C.c_int, C.c_int, f32p]
    lib.vits_bench_conv1d.argtypes = [C.c_int] * 11 + [f32p]
    lib.vits_test_conv1d_sx.argtypes = lib.vits_test_conv1d.argtypes
    lib.vits_test_conv_transpose1d_sx.argtypes = lib.vits_test_conv_transpose1d.argtypes
    lib.vits_test_conv1d_sx_planar.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                               vp, vp, C.c_int, C.c_int, vp, vp]
    lib.vits_test_set_sx_small_max.argtypes = [C.c_longlong]
    lib.vits_test_set_sx_small_max.restype = C.c_longlong
    lib.vits_test_conv1d_sx_gate.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.vits_bench_conv1d_sx.argtypes = [C.c_int] * 9 + [f32p]
    lib.vits_test_conv1d_epi.argtypes = [C.c_int, C.POINTER(VitsTestConvEpiArgs)]
    lib.vits_test_conv1d_sx_epi.argtypes = [C.c_int, C.POINTER(VitsTestConvSxEpiArgs)]
    lib.vits_test_conv_pair16_epi.argtypes = [C.c_int, C.POINTER(VitsTestConvPair16EpiArgs)]
    lib.vits_test_conv_pair_sx_epi.argtypes = [C.c_int, C.POINTER(VitsTestConvPairSxEpiArgs)]
    lib.vits_test_split_identity.argtypes = [vp, C.c_int64, vp, vp]
    lib.vits_test_split_identity_sweep.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.vits_test_split_identity_sweep.restype = C.c_int64
    lib.vits_test_split_forms.argtypes = [C.c_int, vp, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp]
    lib.vits_test_attention_form.argtypes = [C.c_int, C.POINTER(VitsTestAttentionFormArgs)]
    lib.vits_test_wn_gate.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.vits_test_cond_matvec.argtypes = [C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp]
    lib.vits_test_conv_pair_sx.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_float, vp, f32p]
    lib.g2p_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    lib.g2p_close.argtypes = [vp]
    lib.g2p_close.restype = None
    lib.g2p_last_error.argtypes = [vp]
    lib.g2p_last_error.restype = C.c_char_p
    lib.g2p_hparam.argtypes = [vp, C.c_char_p, i64p]
    lib.g2p_num_outputs.argtypes = [vp]
    lib.g2p_output_name.argtypes = [vp, C.c_int]
    lib.g2p_output_name.restype = C.c_char_p
    lib.g2p_bucket.argtypes = [vp, C.c_int, C.c_int]
    lib.g2p_run.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, vp]
    lib.g2p_generate.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int64, C.c_int64, vp, C.POINTER(C.c_int)]
    lib.g2p_generate_batch.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int64, C.c_int64, vp, vp]
    lib.g2p_test_forced_steps.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, vp]
    lib.g2p_test_linear.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int64, C.c_int64, C.c_int, vp]
    lib.g2p_test_step.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_float, C.c_float, vp, vp]
    lib.g2p_test_attention.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int64, C.c_int, C.c_int64, vp, C.c_int, vp,
                                       C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int]
    lib.g2p_test_rmsnorm.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float]
    lib.g2p_test_argmax.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, vp, vp, C.c_int64, C.c_int]
    _LIB = lib
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def last_error(h=None):
    return load().vits_last_error(h).decode("utf-8", "replace")
