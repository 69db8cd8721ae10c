"""ctypes binding of libfs2hip.so (the C ABI declared in include/fs2hip.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc --offload-arch=gfx950)
into ``fs2amd/_lib/libfs2hip.so``; ``FS2_LIB`` overrides the path. There is no CPU fallback:
if the library is missing the import of :mod:`fs2amd.ops` raises.

``import torch`` must happen before the library is loaded so that its libamdhip64.so.7
resolves (by SONAME) to the HIP runtime torch already mapped: one runtime per process.
"""
import ctypes
import os

import torch  # noqa: F401  (load torch's HIP runtime first)

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "_lib", "libfs2hip.so")

FS2_F32, FS2_BF16, FS2_FP8 = 0, 1, 2
FS2_I16 = 3  # include/fs2hip_audio.h: int16 PCM, waveform input only
FS2_F64 = 4  # include/fs2hip_prep.h: IEEE double, the preprocessing entry points only
PITCH_T_MAX, PITCH_T_MAX_NOFILL, OUTLIER_LDS_BYTES = 131072, 4096, 65536  # FS2_PITCH_T_MAX, ..., of the same header
F0_GROUP, F0_LDS_BYTES = 8, 65536  # include/fs2hip_f0.h: FS2_F0_GROUP, FS2_F0_LDS_BYTES
RESAMPLE_LDS_BYTES = 81920  # include/fs2hip_resample.h: FS2_RESAMPLE_LDS_BYTES
# include/fs2hip_align.h: FS2_MAS_LDS_BYTES, FS2_MAS_LDS_SMALL, FS2_FORWARD_SUM_LDS_BYTES, FS2_MAS_AUTO / _LDS / _GLOBAL
MAS_LDS_BYTES, MAS_LDS_SMALL, FORWARD_SUM_LDS_BYTES = 163840, 32768, 65536
MAS_AUTO, MAS_LDS, MAS_GLOBAL = 0, 1, 2
ALIGN_SIZE_CAP = 1 << 24  # csrc/align_sizes.h: FS2_AL_SIZE_CAP
# include/fs2hip_eval.h: FS2_DTW_LDS_BYTES, FS2_DTW_LDS_SMALL, FS2_DTW_AUTO / _LDS / _GLOBAL
DTW_LDS_BYTES, DTW_LDS_SMALL = 163840, 32768
DTW_AUTO, DTW_LDS, DTW_GLOBAL = 0, 1, 2
EVAL_SIZE_CAP = 1 << 24  # csrc/eval_sizes.h: FS2_EV_SIZE_CAP
# include/fs2hip_f0_track.h: FS2_F0_TRACK_THR, _CAP_MAX, _BINS_MAX, _STEP_MAX, _TB, _LDS_BYTES
F0_TRACK_THR, F0_TRACK_CAP_MAX, F0_TRACK_BINS_MAX, F0_TRACK_STEP_MAX, F0_TRACK_TB = 100, 101, 256, 63, 64
F0_TRACK_LDS_BYTES = 65536
# include/fs2hip_vad.h: FS2_VAD_SUMS_BYTES, _AREA_BYTES, _TILE_FRAMES, _CHUNK_FRAMES, _B_MAX
VAD_SUMS_BYTES, VAD_AREA_BYTES, VAD_TILE_FRAMES, VAD_CHUNK_FRAMES, VAD_B_MAX = 32768, 32768, 192, 256, 65535
# include/fs2hip_pvoc.h: FS2_PVOC_BLOCK, _J_CAP, _B_MAX
PVOC_BLOCK, PVOC_J_CAP, PVOC_B_MAX = 64, 2 ** 31 - 1, 65535
# include/fs2hip_iir.h: FS2_IIR_BLOCK, _CHUNK, _S_MAX, _TABLE_LEN, _B_MAX, FS2_LOUD_H_MAX
IIR_BLOCK, IIR_CHUNK, IIR_S_MAX, IIR_TABLE_LEN, IIR_B_MAX, LOUD_H_MAX = 64, 16384, 8, 412, 65535, 32768
FS2_OK, FS2_EINVAL, FS2_ELAUNCH, FS2_EUNSUPPORTED = 0, 1, 2, 3
(EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_TANH, EPI_BIAS_RES, EPI_RES_LN, EPI_RELU_LN, EPI_RELU_LN_DOT, EPI_BIAS_LRELU,
 EPI_RES_SUM, EPI_RELU_GRAD) = range(10)
DUR_I64, DUR_F32, DUR_LOGPRED = 0, 1, 2

_p = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_f = ctypes.c_float
_d = ctypes.c_double


class PackDesc(ctypes.Structure):
    """Mirror of ``fs2_pack_desc`` (include/fs2hip.h)."""

    _fields_ = [("src", _p), ("fwd", _p), ("tr", _p), ("N", _i), ("C", _i), ("KS", _i), ("n_off", _i),
                ("N_tot", _i), ("f32_copy", _i), ("C_tot", _i), ("tiles_c", _i), ("blk0", _i)]


class LossArgs(ctypes.Structure):
    """Mirror of ``fs2_loss_args`` (include/fs2hip.h)."""

    _fields_ = [("mel", _p), ("postnet", _p), ("mel_tgt", _p), ("tgt_bs", _i64), ("tgt_ts", _i64), ("mel_valid", _p),
                ("B", _i), ("T", _i), ("n_mel", _i), ("p_pred", _p), ("p_tgt", _p), ("p_mask", _p), ("n_p", _i64),
                ("e_pred", _p), ("e_tgt", _p), ("e_mask", _p), ("n_e", _i64), ("logd_pred", _p), ("d_tgt", _p),
                ("d_mask", _p), ("n_d", _i64)]


class AdamParam(ctypes.Structure):
    """Mirror of ``fs2_adam_param`` (include/fs2hip.h)."""

    _fields_ = [("p", _p), ("m", _p), ("v", _p), ("step", _p), ("off", _i64), ("numel", _i64)]


class ReduceDesc(ctypes.Structure):
    """Mirror of ``fs2_reduce_desc`` (include/fs2hip.h)."""

    _fields_ = [("part", _p), ("M", _i64), ("S", _i), ("kind", _i), ("KS", _i), ("N", _i), ("C", _i), ("split", _i),
                ("accumulate", _i), ("pad_", _i), ("out0", _p), ("out1", _p), ("out2", _p), ("blk0", _i64)]


REDUCE_BATCH_MAX = 32


class ReduceBatch(ctypes.Structure):
    """Mirror of ``fs2_reduce_batch`` (include/fs2hip.h)."""

    _fields_ = [("n", _i), ("pad_", _i), ("d", ReduceDesc * REDUCE_BATCH_MAX)]


class ConvDesc(ctypes.Structure):
    """Mirror of ``fs2_conv_desc`` (include/fs2hip.h)."""

    _fields_ = [
        ("x", _p), ("x_dtype", _i), ("x_row_stride", _i64),
        ("w", _p), ("bias", _p),
        ("B", _i), ("T", _i), ("Cin", _i), ("Cin_pad", _i), ("N", _i), ("KS", _i), ("pad", _i),
        ("compute", _i), ("epilogue", _i),
        ("residual", _p), ("res_dtype", _i), ("res_row_stride", _i64),
        ("ln_gamma", _p), ("ln_beta", _p), ("ln_eps", _f),
        ("lens", _p), ("addvec1", _p), ("addvec2", _p),
        ("dot_w", _p), ("dot_b", _f),
        ("out", _p), ("out_dtype", _i), ("out_row_stride", _i64),
        ("rows_dev", _p), ("row_pos", _p), ("a_rowmap", _p),
        ("col_scale", _p), ("out_scale", _f), ("out2", _p), ("out2_scale", _f),
        ("cin_block", _i), ("cin_src", _i * 4), ("out_split", _i),
        ("splitk_ws", _p), ("splitk_ws_bytes", _i64),
        ("dilation", _i), ("act_slope", _f), ("out2_act", _i), ("out2_slope", _f), ("out2_f32", _i),
        ("residual2", _p), ("out_div", _f),
        ("group_n", _i), ("group_cin", _i),
    ]


class Ffn8Desc(ctypes.Structure):
    """Mirror of ``fs2_ffn8_desc`` (include/fs2hip.h)."""

    _fields_ = [
        ("x8", _p), ("x8_row_stride", _i64), ("res", _p), ("res_row_stride", _i64), ("w", _p),
        ("cs1", _p), ("b1", _p), ("inv_sf", _f), ("cs2", _p), ("b2", _p),
        ("B", _i), ("T", _i), ("D", _i), ("F", _i), ("KS", _i), ("pad", _i),
        ("ln_gamma", _p), ("ln_beta", _p), ("ln_eps", _f),
        ("out", _p), ("out_row_stride", _i64), ("out8", _p), ("out8_row_stride", _i64), ("out8_scale", _f),
        ("rows_dev", _p), ("row_pos", _p), ("rows_max", _i),
    ]


class WconvDesc(ctypes.Structure):
    """Mirror of ``fs2_wconv_desc`` (include/fs2hip.h)."""

    _fields_ = [
        ("x", _p), ("x_row_stride", _i64), ("w", _p), ("bias", _p),
        ("B", _i), ("T", _i), ("Cin", _i), ("N", _i), ("KS", _i), ("pad", _i), ("epilogue", _i),
        ("out", _p), ("out_row_stride", _i64), ("w2", _p), ("bias2", _p), ("residual", _p), ("res_row_stride", _i64),
        ("rows_dev", _p), ("row_pos", _p), ("rows_max", _i),
    ]


class PnHead3Desc(ctypes.Structure):
    """Mirror of ``fs2_pn_head3_desc`` (include/fs2hip_postnet.h)."""

    _fields_ = [
        ("x", _p), ("x_row_stride", _i64), ("x_rows", _i64), ("rowmap", _p), ("mel_w", _p), ("mel_b", _p),
        ("mel", _p), ("mel_row_stride", _i64), ("mel_bf16", _p), ("w", _p * 3), ("bias", _p * 3),
        ("B", _i), ("T", _i), ("out", _p), ("out_row_stride", _i64),
    ]


class CondDesc(ctypes.Structure):
    """Mirror of ``fs2_cond_desc`` (include/fs2hip.h)."""

    _fields_ = [
        ("speakers", _p), ("speaker_table", _p), ("n_speaker", _i), ("emotions", _p), ("emo_table", _p),
        ("n_emo", _i), ("d_emo", _i), ("arousals", _p), ("aro_table", _p), ("n_aro", _i), ("d_aro", _i),
        ("valences", _p), ("val_table", _p), ("n_val", _i), ("d_val", _i), ("lin_w", _p), ("lin_b", _p),
        ("spk_out", _p), ("emo_out", _p),
    ]


class CondMixDesc(ctypes.Structure):
    """Mirror of ``fs2_cond_mix_desc`` (include/fs2hip_cond_mix.h)."""

    _fields_ = [
        ("speakers", _p), ("spk_kind", _i), ("speaker_table", _p), ("n_speaker", _i),
        ("emotions", _p), ("emo_kind", _i), ("emo_table", _p), ("n_emo", _i), ("d_emo", _i),
        ("arousals", _p), ("aro_kind", _i), ("aro_table", _p), ("n_aro", _i), ("d_aro", _i),
        ("valences", _p), ("val_kind", _i), ("val_table", _p), ("n_val", _i), ("d_val", _i),
        ("lin_w", _p), ("lin_b", _p), ("B", _i), ("D", _i), ("spk_out", _p), ("emo_out", _p),
    ]


class CondGrads(ctypes.Structure):
    """Mirror of ``fs2_cond_grads`` (include/fs2hip.h)."""

    _fields_ = [("d_speaker_table", _p), ("d_emo_table", _p), ("d_aro_table", _p), ("d_val_table", _p),
                ("d_lin_w", _p), ("d_lin_b", _p)]


class FfnDesc(ctypes.Structure):
    """Mirror of ``fs2_ffn_desc`` (include/fs2hip.h)."""

    _fields_ = [
        ("x", _p), ("x_row_stride", _i64),
        ("w", _p), ("b1", _p), ("b2", _p),
        ("B", _i), ("T", _i), ("D", _i), ("F", _i), ("KS", _i), ("pad", _i),
        ("ln_gamma", _p), ("ln_beta", _p), ("ln_eps", _f),
        ("lens", _p), ("addvec1", _p), ("addvec2", _p),
        ("out", _p), ("out_row_stride", _i64),
        ("rows_dev", _p), ("row_pos", _p),
        ("nsplit", _i), ("splitk_ws", _p), ("splitk_ws_bytes", _i64), ("rows_max", _i),
        ("tile_rows", _i),
        ("wqkv", _p), ("bqkv", _p), ("qkv_out", _p), ("qkv_row_stride", _i64), ("nqkv", _i),
        ("pre_att", _p), ("pre_att_row_stride", _i64), ("pre_w", _p), ("pre_b", _p), ("pre_gamma", _p),
        ("pre_beta", _p), ("pre_eps", _f),
    ]


class VpFusedDesc(ctypes.Structure):
    """Mirror of ``fs2_vp_fused_desc`` (include/fs2hip.h)."""

    _fields_ = [
        ("x", _p), ("x_row_stride", _i64), ("w", _p), ("vec", _p), ("lin_b", _p), ("ln_eps", _f),
        ("B", _i), ("L", _i), ("G", _i), ("lens", _p), ("pred", _p), ("embed_group", _i),
        ("x_out", _p), ("x_out_row_stride", _i64), ("target", _p), ("control", _f), ("bins", _p),
        ("n_bins", _i), ("table", _p),
    ]


class VpFusedMapDesc(ctypes.Structure):
    """Mirror of ``fs2_vp_fused_map_desc`` (include/fs2hip_prosody.h)."""

    _fields_ = [("base", VpFusedDesc), ("control_map", _p)]


class MelDesc(ctypes.Structure):
    """Mirror of ``fs2_mel_desc`` (include/fs2hip_audio.h)."""

    _fields_ = [
        ("wav", _p), ("wav_dtype", _i), ("max_wav_value", _f), ("wav_row_stride", _i64), ("lens", _p),
        ("lens_host", _p), ("B", _i), ("n_max", _i), ("T_out", _i), ("n_fft", _i), ("hop", _i), ("win", _i),
        ("n_mel", _i), ("basis", _p), ("mel_basis", _p), ("clip_val", _f), ("mel", _p), ("energy", _p), ("mag", _p),
        ("frames_out", _p),
    ]


class StftDesc(ctypes.Structure):
    """Mirror of ``fs2_stft_desc`` (include/fs2hip_audio_inv.h)."""

    _fields_ = [
        ("wav", _p), ("wav_row_stride", _i64), ("lens", _p), ("lens_host", _p), ("B", _i), ("n_max", _i),
        ("T_out", _i), ("n_fft", _i), ("hop", _i), ("win", _i), ("clip", _i), ("basis", _p), ("mag_target", _p),
        ("mag_row_stride", _i64), ("spec", _p), ("mag", _p), ("recomb", _p), ("frames_out", _p),
    ]


class IstftDesc(ctypes.Structure):
    """Mirror of ``fs2_istft_desc`` (include/fs2hip_audio_inv.h)."""

    _fields_ = [
        ("recomb", _p), ("recomb_row_stride", _i64), ("frames", _p), ("frames_host", _p), ("B", _i), ("T_in", _i),
        ("n_out_max", _i), ("n_fft", _i), ("hop", _i), ("win", _i), ("inv_packed", _p), ("wsum_table", _p),
        ("wav", _p), ("wav_row_stride", _i64), ("lens_out", _p),
    ]


class PvocDesc(ctypes.Structure):
    """Mirror of ``fs2_pvoc_desc`` (include/fs2hip_pvoc.h)."""

    _fields_ = [
        ("spec", _p), ("spec_row_stride", _i64), ("frames", _p), ("frames_host", _p), ("rates", _p), ("rates_host", _p),
        ("B", _i), ("NB", _i), ("T_max", _i), ("J_max", _i), ("recomb", _p), ("recomb_row_stride", _i64),
        ("frames_out", _p),
    ]


ISTFT_KPAD = 1032  # FS2_ISTFT_KPAD: the 1026 recomb channels padded to 129 groups of 8

# name -> (restype, argtypes)
SIGNATURES = {
    "fs2_version": (ctypes.c_char_p, []),
    "fs2_build_id": (ctypes.c_char_p, []),
    "fs2_status_string": (ctypes.c_char_p, [_i]),
    "fs2_conv_cin_pad": (_i, [_i, _i]),
    "fs2_conv1d": (_i, [ctypes.POINTER(ConvDesc), _p]),
    "fs2_ffn": (_i, [ctypes.POINTER(FfnDesc), _p]),
    "fs2_ffn_wide": (_i, [ctypes.POINTER(FfnDesc), _p, ctypes.c_int64, _p]),
    "fs2_ffn_weight_elems": (ctypes.c_int64, [_i, _i]),
    "fs2_ffn8": (_i, [ctypes.POINTER(Ffn8Desc), _p]),
    "fs2_ffn8_weight_bytes": (ctypes.c_int64, [_i, _i]),
    "fs2_wconv": (_i, [ctypes.POINTER(WconvDesc), _p]),
    "fs2_wconv_weight_elems": (ctypes.c_int64, [_i, _i, _i]),
    "fs2_attention": (_i, [_p, _i, _i64, _p, _i, _i, _i, _i, _f, _p, _i64, _p, _p, _p]),
    "fs2_attention_ex": (_i, [_p, _i, _i64, _p, _i, _i, _i, _i, _f, _p, _i64, _p, _p, _i, _p, _i64, _i64, _p]),
    "fs2_attention_split_ws_bytes": (_i64, [_i, _i, _i, _i64]),
    "fs2_attention_items": (_i, [_p, _i, _i, _i, _p, _i64, _i64, _p]),
    "fs2_embed_pe": (_i, [_p, _p, _i, _p, _i, _i, _i, _p, _i, _p, _p]),
    "fs2_attention_bwd": (_i, [_p, _i, _i64, _p, _i64, _p, _i64, _p, _i, _i, _i, _i, _f, _p, _i64, _p, _p, _i64, _p,
                               _p]),
    "fs2_cond_vectors": (_i, [_p, _p, _i, _p, _p, _i, _i, _p, _p, _i, _i, _p, _p, _i, _i, _p, _p, _i, _i, _p, _p,
                              _p]),
    "fs2_variance_embed": (_i, [_p, _i, _p, _p, _f, _p, _i, _p, _i, _i, _p]),
    "fs2_variance_embed_ex": (_i, [_p, _i, _p, _p, _i, _p, _i, _i, _p, _p, _p]),
    "fs2_lr_backward": (_i, [_p, _p, _i, _i, _i, _i, _p, _p]),
    "fs2_lr_durations": (_i, [_p, _i, _f, _i, _i, _p, _p, _p, _p]),
    "fs2_lr_expand": (_i, [_p, _i, _p, _p, _i, _i, _i, _i, _p, _p, _i, _p, _p, _p]),
    "fs2_pack_rows": (_i, [_p, _i, _p, _p, _i, _p, _p, _i64, _p]),
    "fs2_postnet_assemble": (_i, [_p, _p, _p, _i, _i, _i, _p, _p, _i, _p, _p]),
    "fs2_seq_layout_margin": (_i, [_p, _i, _i, _i, _p, _p, _p, _p]),
    "fs2_len_stats": (_i, [_p, _i, _p, _p, _p]),
    "fs2_seq_layout": (_i, [_p, _i, _i, _p, _p, _p, _p]),
    "fs2_vp_norm": (_i, [_p, _i64, _i, _i, _i, _p, _p, _f, _p, _i64, _p]),
    "fs2_vp_head": (_i, [_p, _i64, _i, _i, _i, _i, _p, _p, _f, _p, _p, _p, _p, _i, _p, _i, _i64, _i, _p, _f, _p, _i, _p,
                         _p]),
    "fs2_vp_fused": (_i, [ctypes.POINTER(VpFusedDesc), _p]),
    "fs2_vp_fused_weight_elems": (ctypes.c_int64, [_i]),
    "fs2_lr_fused": (_i, [_p, _i, _p, _i, _f, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p]),
    "fs2_enc_attn_block": (_i, [_p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _f, _i, _i, _f, _p, _p, _i64, _p]),
    "fs2_enc_embed_attn_block": (_i, [_p, _p, _i, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _f, _i, _i, _f, _p, _p, _p,
                                      _i, _p, _p, _p, _i64, _p]),
    "fs2_lr_fused_proj": (_i, [_p, _i, _p, _i, _f, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p,
                               _p, _p, _i, _p, _p]),
    "fs2_hifigan_mrf": (_i, [_p, _p, _p, _p, _i, _i, _i, _f, _p, _p]),
    "fs2_hifigan_mrf_weight_elems": (ctypes.c_int64, [_i]),
    "fs2_hifigan_pair": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _f, _f, _i, _p, _p]),
    "fs2_hifigan_post": (_i, [_p, _p, _f, _i, _i, _i, _i, _p, _p]),
    "fs2_res_ln_fwd": (_i, [_p, _p, _i, _p, _p, _p, _i64, _i, _i, _f, _f, _p, _i, _p, _p, _p, _p, _p]),
    "fs2_res_ln_bwd_ws_bytes": (_i64, [_i]),
    "fs2_pack_train_plan": (_i, [_p, _i, _p]),
    "fs2_pack_train": (_i, [_p, _i, _i, _p]),
    "fs2_res_ln_bwd": (_i, [_p, _p, _p, _p, _p, _i64, _i, _i, _f, _p, _i, _p, _p, _p, _p, _p, _i, _i, _p, _i64, _p]),
    "fs2_relu_ln_fwd": (_i, [_p, _p, _p, _i64, _i, _f, _f, _p, _i, _p, _p, _p, _p, _p]),
    "fs2_relu_ln_bwd": (_i, [_p, _p, _p, _p, _p, _i64, _i, _f, _p, _i, _p, _p, _p, _p, _i, _i, _p, _i64, _p]),
    "fs2_relu_ln_head_fwd": (_i, [_p, _p, _p, _i64, _i, _f, _f, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p]),
    "fs2_relu_ln_head_bwd_ws_bytes": (_i64, [_i]),
    "fs2_relu_ln_head_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _f, _p, _i, _p, _p, _p, _p, _p, _p, _i, _i,
                                  _p, _i64, _p]),
    "fs2_embedding_bwd": (_i, [_p, _i64, _p, _i64, _i, _i, _i, _p, _i, _p]),
    "fs2_loss_ws_bytes": (_i64, []),
    "fs2_loss_fwd": (_i, [_p, _p, _p, _p, _i64, _p]),
    "fs2_loss_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "fs2_bn_train_ws_bytes": (_i64, [_i]),
    "fs2_bn_train_fwd": (_i, [_p, _i64, _i, _p, _p, _f, _f, _p, _p, _i, _f, _p, _i, _p, _p, _p, _p, _p, _p, _i64, _p]),
    "fs2_bn_train_bwd": (_i, [_p, _p, _i64, _i, _p, _p, _p, _p, _i, _f, _p, _i, _p, _p, _p, _i, _p, _i64, _p]),
    "fs2_adam_ws_bytes": (_i64, []),
    "fs2_adam_flat": (_i, [_p, _i64, _p, _i, _p, _f, _f, _f, _f, _f, _f, _p, _i64, _p]),
    "fs2_colsum_ws_bytes": (_i64, [_i]),
    "fs2_colsum": (_i, [_p, _i, _i64, _i, _i64, _p, _i, _p, _i64, _p]),
    "fs2_conv_wgrad_ws_bytes": (_i64, [_i, _i, _i, _i, _i]),
    "fs2_conv_wgrad": (_i, [_p, _i, _i64, _p, _i64, _i, _i, _i, _i, _i, _i, _p, _p, _i, _i, _p, _p, _p, _p, _i, _p,
                            _i64, _p]),
    "fs2_conv_wgrad_splits": (_i, [_i, _i, _i, _i, _i]),
    "fs2_ln_bwd_parts": (_i, [_i64]),
    "fs2_reduce_batch_launch": (_i, [_p, _p]),
    "fs2_cond_bwd_ws_bytes": (_i64, [_i, _i]),
    "fs2_cond_bwd": (_i, [_p, _i, _i, _i, _p, _p, _p, _i64, _p]),
    "fs2_length_masks": (_i, [_p, _i, _i, _p, _p]),
    "fs2_length_regulate": (_i, [_p, _i, _p, _i, _f, _i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p]),
}


# include/fs2hip_prosody.h: the control-map siblings (the scalar entry's arguments plus the map
# pointer after the scalar control; NULL = the scalar)
SIGNATURES_PROSODY = {
    "fs2_lr_durations_map": (_i, [_p, _i, _f, _p, _i, _i, _p, _p, _p, _p]),
    "fs2_length_regulate_map": (_i, [_p, _i, _p, _i, _f, _p, _i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p]),
    "fs2_lr_fused_proj_map": (_i, [_p, _i, _p, _i, _f, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _i, _p, _p,
                                   _p, _p, _p, _i, _p, _p]),
    "fs2_variance_embed_map": (_i, [_p, _i, _p, _p, _f, _p, _p, _i, _p, _i, _i, _p]),
    "fs2_vp_head_map": (_i, [_p, _i64, _i, _i, _i, _i, _p, _p, _f, _p, _p, _p, _p, _i, _p, _i, _i64, _i, _p, _f, _p, _p,
                             _i, _p, _p]),
    "fs2_vp_fused_map": (_i, [ctypes.POINTER(VpFusedMapDesc), _p]),
}


# include/fs2hip_audio.h: waveform -> log-mel + energy, and the phoneme-level segment mean
SIGNATURES_AUDIO = {
    "fs2_mel_spectrogram": (_i, [ctypes.POINTER(MelDesc), _p]),
    "fs2_segment_mean": (_i, [_p, _p, _i, _i, _i, _p, _p]),
}


# include/fs2hip_audio_inv.h: waveform -> spectrum (with the Griffin-Lim projection) and back
SIGNATURES_AUDIO_INV = {
    "fs2_stft": (_i, [ctypes.POINTER(StftDesc), _p]),
    "fs2_istft": (_i, [ctypes.POINTER(IstftDesc), _p]),
}


# include/fs2hip_prep.h: pitch targets, outlier fence + moments, their running merge, normalisation
SIGNATURES_PREP = {
    "fs2_pitch_targets": (_i, [_p, _i64, _p, _p, _i, _i, _i, _p, _p, _p, _p]),
    "fs2_outlier_moments": (_i, [_p, _i, _i64, _p, _i, _i, _p, _p, _p, _p, _p, _p]),
    "fs2_moments_merge": (_i, [_p, _p, _p, _i, _p, _p]),
    "fs2_normalize_minmax_ws_bytes": (_i64, [_i]),
    "fs2_normalize_minmax": (_i, [_p, _i, _i64, _p, _i, _i, _d, _d, _p, _p, _p, _i64, _p]),
}


# include/fs2hip_f0.h: waveform -> F0 contour (YIN, float64)
SIGNATURES_F0 = {
    "fs2_f0_lds_bytes": (_i64, [_i, _i, _i]),
    "fs2_f0_yin": (_i, [_p, _i, _i64, _p, _i, _i, _d, _i, _i, _i, _i, _d, _d, _d, _p, _p, _p, _p]),
}


# include/fs2hip_resample.h: raw audio -> resampled f64 / f32 rows with their peak -> int16
SIGNATURES_RESAMPLE = {
    "fs2_resample_out_len": (_i64, [_i64, _i64, _i64]),
    "fs2_resample_lds_bytes": (_i64, [_i64, _i64]),
    "fs2_resample": (_i, [_p, _i, _i64, _p, _i, _i, _i, _i, _p, _i, _p, _p, _p, _p, _p]),
    "fs2_peak_int16": (_i, [_p, _p, _p, _i, _i, _f, _p, _p]),
}


# include/fs2hip_align.h: monotonic alignment search, the forward-sum loss and its gradient
SIGNATURES_ALIGN = {
    "fs2_mas_lds_bytes": (_i64, [_i, _i, _i]),
    "fs2_mas_ws_bytes": (_i64, [_i, _i, _i]),
    "fs2_forward_sum_lds_bytes": (_i64, [_i, _i]),
    "fs2_mas": (_i, [_p, _i, _i64, _i64, _p, _p, _i, _i, _i, _i, _p, _i64, _p, _p, _p, _p]),
    "fs2_forward_sum": (_i, [_p, _i, _i64, _i64, _p, _p, _i, _i, _i, _d, _p, _p, _p, _p]),
    "fs2_forward_sum_bwd": (_i, [_p, _i, _i64, _i64, _p, _p, _i, _i, _i, _d, _p, _p, _p, _p, _p]),
}


def mas_lds_bytes(T_max, L_max, in_lds=True):
    """The Python mirror of csrc/align_sizes.h (al_mas_lds_bytes): two v rows of L_max + 1 f64, then the
    decision bitmap of T_max rows of ceil(L_max / 64) 64-bit words when it lives in LDS. 0 for a size
    below 1, 2^63 - 1 beyond the cap."""
    if T_max < 1 or L_max < 1:
        return 0
    if max(T_max, L_max) > ALIGN_SIZE_CAP:
        return (1 << 63) - 1
    return 8 * (2 * (L_max + 1) + (T_max * ((L_max + 63) // 64) if in_lds else 0))


def mas_ws_bytes(B, T_max, L_max):
    """al_mas_ws_bytes: the bitmap of the global form, B * T_max * ceil(L_max / 64) * 8 bytes."""
    if B < 1 or T_max < 1 or L_max < 1:
        return 0
    n = 8 * B * T_max * ((L_max + 63) // 64)
    return (1 << 63) - 1 if max(B, T_max, L_max) > ALIGN_SIZE_CAP or n > (1 << 63) - 1 else n


def forward_sum_lds_bytes(T_max, L_max):
    """al_fs_lds_bytes: two state rows of 2 L_max + 5 f64, then the max and the log-sum of every frame."""
    if T_max < 1 or L_max < 1:
        return 0
    if max(T_max, L_max) > ALIGN_SIZE_CAP:
        return (1 << 63) - 1
    return 8 * (2 * (2 * L_max + 5) + 2 * T_max)


def mas_form(T_max, L_max, bitmap=MAS_AUTO):
    """al_mas_form: (status, MAS_LDS or MAS_GLOBAL or None)."""
    if T_max < 1 or L_max < 1 or bitmap not in (MAS_AUTO, MAS_LDS, MAS_GLOBAL):
        return FS2_EINVAL, None
    if mas_lds_bytes(T_max, L_max, False) > MAS_LDS_BYTES:
        return FS2_EUNSUPPORTED, None
    fits = mas_lds_bytes(T_max, L_max, True) <= MAS_LDS_BYTES
    if bitmap == MAS_LDS and not fits:
        return FS2_EUNSUPPORTED, None
    return FS2_OK, MAS_GLOBAL if bitmap == MAS_GLOBAL or not fits else MAS_LDS


# include/fs2hip_eval.h: mel cepstra, pairwise distances, dynamic time warping, statistics along the path
SIGNATURES_EVAL = {
    "fs2_dtw_lds_bytes": (_i64, [_i, _i, _i]),
    "fs2_dtw_ws_bytes": (_i64, [_i, _i, _i]),
    "fs2_mel_cepstrum": (_i, [_p, _i, _i64, _i64, _p, _p, _i, _i, _i, _i, _p, _p]),
    "fs2_pair_dist": (_i, [_p, _p, _i, _i64, _i64, _i64, _i64, _p, _p, _i, _i, _i, _i, _i, _p, _p]),
    "fs2_dtw": (_i, [_p, _p, _i, _i64, _i64, _i64, _i64, _p, _p, _i, _i, _i, _i, _i, _p, _i64, _p, _p, _p, _p, _p]),
    "fs2_path_stats": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p]),
}


def dtw_bitmap_words(Tx_max, Ty_max):
    """ev_dtw_bitmap_words of csrc/eval_sizes.h: two bit planes of ceil(Tx_max / 64) 64-bit words for
    each of the Tx_max + Ty_max - 1 anti-diagonals."""
    return (Tx_max + Ty_max - 1) * 2 * ((Tx_max + 63) // 64)


def dtw_lds_bytes(Tx_max, Ty_max, in_lds=True):
    """The Python mirror of csrc/eval_sizes.h (ev_dtw_lds_bytes): three anti-diagonals of Tx_max + 3
    f64, then the step bitmap when it lives in LDS. 0 for a size below 1, 2^63 - 1 beyond the cap."""
    if Tx_max < 1 or Ty_max < 1:
        return 0
    if max(Tx_max, Ty_max) > EVAL_SIZE_CAP:
        return (1 << 63) - 1
    return 8 * (3 * (Tx_max + 3) + (dtw_bitmap_words(Tx_max, Ty_max) if in_lds else 0))


def dtw_ws_bytes(B, Tx_max, Ty_max):
    """ev_dtw_ws_bytes: the bitmap of the global form, B * dtw_bitmap_words * 8 bytes."""
    if B < 1 or Tx_max < 1 or Ty_max < 1:
        return 0
    n = 8 * B * dtw_bitmap_words(Tx_max, Ty_max)
    return (1 << 63) - 1 if max(B, Tx_max, Ty_max) > EVAL_SIZE_CAP or n > (1 << 63) - 1 else n


def dtw_form(Tx_max, Ty_max, bitmap=DTW_AUTO):
    """ev_dtw_form: (status, DTW_LDS or DTW_GLOBAL or None)."""
    if Tx_max < 1 or Ty_max < 1 or bitmap not in (DTW_AUTO, DTW_LDS, DTW_GLOBAL):
        return FS2_EINVAL, None
    if dtw_lds_bytes(Tx_max, Ty_max, False) > DTW_LDS_BYTES:
        return FS2_EUNSUPPORTED, None
    fits = dtw_lds_bytes(Tx_max, Ty_max, True) <= DTW_LDS_BYTES
    if bitmap == DTW_LDS and not fits:
        return FS2_EUNSUPPORTED, None
    return FS2_OK, DTW_GLOBAL if bitmap == DTW_GLOBAL or not fits else DTW_LDS


# include/fs2hip_f0_track.h: the cmnd table of fs2_f0_yin -> an F0 path through the utterance (Viterbi)
SIGNATURES_F0_TRACK = {
    "fs2_f0_track_lds_bytes": (_i64, [_i, _i]),
    "fs2_f0_track_workspace_bytes": (_i64, [_i, _i, _i, _i, _i]),
    "fs2_f0_track": (_i, [_p, _p, _i, _i, _i, _d, _i, _i, _d, _d, _p, _p, _p, _p, _p, _i, _p, _p, _i, _d, _d, _p, _i64,
                          _p, _p, _p, _p]),
}


# include/fs2hip_vad.h: frame power, activity mask / intervals / trim, the ragged cut
SIGNATURES_VAD = {
    "fs2_vad_frames": (_i64, [_i64, _i64]),
    "fs2_vad_workspace_bytes": (_i64, [_i64, _i64, _i64, _i64]),
    "fs2_vad_lds_bytes": (_i64, [_i64, _i64]),
    "fs2_vad_power": (_i, [_p, _i, _i64, _p, _i, _i, _i, _i, _p, _p, _p, _i64, _p]),
    "fs2_vad_intervals": (_i, [_p, _p, _p, _i, _i, _i, _d, _d, _i, _i64, _i, _i, _p, _p, _p, _p, _p]),
    "fs2_vad_cut": (_i, [_p, _i, _i64, _p, _i, _i, _i, _p, _p, _p]),
}


# include/fs2hip_pvoc.h: the phase vocoder between fs2_stft and fs2_istft
SIGNATURES_PVOC = {
    "fs2_pvoc_frames": (_i64, [_i64, _d]),
    "fs2_phase_vocoder": (_i, [ctypes.POINTER(PvocDesc), _p]),
}


# include/fs2hip_postnet.h: mel_linear + the PostNet's layers 0..2 in one launch
SIGNATURES_POSTNET = {
    "fs2_pn_head3": (_i, [ctypes.POINTER(PnHead3Desc), _p]),
}

# include/fs2hip_iir.h: cascaded second-order sections, BS.1770 gating, the loudness gain
SIGNATURES_IIR = {
    "fs2_iir_blocks": (_i64, [_i64]),
    "fs2_iir_chunks": (_i64, [_i64]),
    "fs2_loudness_blocks": (_i64, [_i64, _i64]),
    "fs2_loudness_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "fs2_sosfilt": (_i, [_p, _i, _i64, _p, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p]),
    "fs2_loudness_gate": (_i, [_p, _p, _i, _i, _i, _d, _d, _p, _p, _p, _i64, _p]),
    "fs2_gain_int16": (_i, [_p, _i, _i64, _p, _i, _i, _p, _d, _d, _p, _p, _p, _p, _p, _p]),
}


# include/fs2hip_cond_mix.h: conditioning vectors from weights over the embedding rows
COND_NONE, COND_IDS, COND_MIX, COND_ROWS = 0, 1, 2, 3  # FS2_COND_NONE / _IDS / _MIX / _ROWS
SIGNATURES_COND_MIX = {
    "fs2_cond_mix": (_i, [ctypes.POINTER(CondMixDesc), _p]),
    "fs2_cond_mix_rows": (_i, [ctypes.POINTER(CondMixDesc), _i, _p, _i, _p]),
}


def iir_blocks(n):
    """iir_blocks of csrc/iir_sizes.h: 0 for n < 1, else ceil(n / 64)."""
    return 0 if n < 1 else (n - 1) // IIR_BLOCK + 1


def iir_chunks(n):
    """iir_chunks: 0 for n < 1, else ceil(n / 16384)."""
    return 0 if n < 1 else (n - 1) // IIR_CHUNK + 1


def loudness_blocks(n, H):
    """loud_blocks: the gating blocks of n samples at hop H >= 1, 0 for n < 4 H, else (n - 4 H) // H + 1."""
    return 0 if n < 1 or n < 4 * H else (n - 4 * H) // H + 1


def loudness_workspace_bytes(B, n_max, H):
    """loud_workspace_bytes: J + 3 sub-block sums and the two tree buffers (J and (J + 1) // 2) per row as
    f64; 0 for a size below 1 or no block; 2^63 - 1 where it does not fit."""
    if B < 1 or n_max < 1 or H < 1:
        return 0
    J = loudness_blocks(n_max, H)
    if J < 1:
        return 0
    return min(8 * B * ((J + 3) + J + (J + 1) // 2), (1 << 63) - 1)


def iir_status(B, n_max, S, row_stride):
    """iir_check: the status fs2_sosfilt gives these sizes."""
    if B < 1 or n_max < 1 or S < 1 or row_stride < n_max:
        return FS2_EINVAL
    return FS2_EUNSUPPORTED if S > IIR_S_MAX or B > IIR_B_MAX else FS2_OK


def loudness_status(B, n_max, H):
    """loud_check: the status fs2_loudness_gate gives these sizes."""
    if B < 1 or n_max < 1 or H < 1:
        return FS2_EINVAL
    if H > LOUD_H_MAX or B > IIR_B_MAX or loudness_workspace_bytes(B, n_max, H) == (1 << 63) - 1:
        return FS2_EUNSUPPORTED
    return FS2_OK


def gain_status(B, n_max, row_stride):
    """gain_check: the status fs2_gain_int16 gives these sizes."""
    if B < 1 or n_max < 1 or row_stride < n_max:
        return FS2_EINVAL
    return FS2_EUNSUPPORTED if B > IIR_B_MAX else FS2_OK


def pvoc_frames(T, rate):
    """pvoc_frames of csrc/pvoc_sizes.h: the number of j >= 0 with fl(j * rate) < T, saturated at
    PVOC_J_CAP; 0 for T < 1 and for a rate that is not finite or is <= 0."""
    import math

    T, rate = int(T), float(rate)
    if T < 1 or not rate > 0.0 or not math.isfinite(rate):
        return 0
    t = float(min(T, PVOC_J_CAP))
    q = t / rate  # IEEE: an overflow gives inf
    if not q < 2147483649.0:  # ceil(q) < 2147483650
        return PVOC_J_CAP
    j = math.ceil(q)
    while j > 0 and not float(j - 1) * rate < t:
        j -= 1
    while float(j) * rate < t:
        j += 1
    return min(j, PVOC_J_CAP)


def pvoc_status(B, NB, T_max, J_max, spec_row_stride, recomb_row_stride):
    """pvoc_check: the status fs2_phase_vocoder gives these sizes."""
    if B < 1 or NB < 1 or T_max < 1 or J_max < 1 or spec_row_stride < T_max or recomb_row_stride < J_max:
        return FS2_EINVAL
    return FS2_EUNSUPPORTED if B > PVOC_B_MAX else FS2_OK


def vad_frames(n, hop):
    """vad_frames of csrc/vad_sizes.h: 0 for n < 1, else 1 + n // hop."""
    return 0 if n < 1 else 1 + n // hop


def vad_tile_frames(frame_length, hop):
    """vad_tile_frames: frames per workgroup of fs2_vad_power, 0 where one frame's block sums do not fit."""
    import math

    g = math.gcd(frame_length, hop)
    q, h = frame_length // g, hop // g
    if q > VAD_SUMS_BYTES // 8:
        return 0
    return min((VAD_SUMS_BYTES // 8 - q) // h + 1, VAD_TILE_FRAMES)


def vad_workspace_bytes(B, F_max, frame_length, hop):
    """vad_workspace_bytes: one f64 maximum per tile and row. 0 for a size below 1, hop > frame_length or
    a geometry without a tile, 2^63 - 1 where it does not fit."""
    if B < 1 or F_max < 1 or frame_length < 1 or hop < 1 or hop > frame_length:
        return 0
    G = vad_tile_frames(frame_length, hop)
    return min(8 * B * ((F_max + G - 1) // G), (1 << 63) - 1) if G >= 1 else 0


def vad_lds_bytes(frame_length, hop):
    """vad_lds_bytes: one frame's block sums as f64 and one block of f32 samples at its padded stride."""
    import math

    if frame_length < 1 or hop < 1 or hop > frame_length:
        return 0
    g = math.gcd(frame_length, hop)
    return 8 * (frame_length // g) + 4 * (g | 1)


def vad_status(B, n_max, frame_length, hop):
    """vad_check: the status fs2_vad_power gives these sizes."""
    import math

    if B < 1 or n_max < 1 or frame_length < 1 or hop < 1 or hop > frame_length:
        return FS2_EINVAL
    g = math.gcd(frame_length, hop)
    F = vad_frames(n_max, hop)
    if B > VAD_B_MAX or 8 * (frame_length // g) > VAD_SUMS_BYTES or 4 * (g | 1) > VAD_AREA_BYTES \
            or F > 2 ** 31 - 1 or B * F > (2 ** 31 - 1) // 8:
        return FS2_EUNSUPPORTED
    return FS2_OK


def f0_track_cap(tau_min, tau_max):
    """ft_cap of csrc/f0_track_sizes.h: the candidates of one frame that can survive."""
    return min((tau_max - tau_min + 1) // 2, F0_TRACK_CAP_MAX)


def f0_track_workspace_bytes(B, F_max, tau_min, tau_max, n_bins):
    """The Python mirror of csrc/f0_track_sizes.h (f0_track_sizes): the frame heads, the three candidate
    lists and the predecessor bytes, each rounded up to 8 bytes. 0 for a size below 1, 2^63 - 1 where
    it does not fit."""
    if B < 1 or F_max < 1 or n_bins < 1 or tau_min < 2 or tau_min >= tau_max:
        return 0
    frames = B * F_max
    ents = frames * f0_track_cap(tau_min, tau_max)
    r8 = lambda a: (a + 7) // 8 * 8  # noqa: E731
    n = r8(8 * frames) + 16 * ents + r8(4 * ents) + r8(frames * 2 * n_bins)
    return min(n, (1 << 63) - 1)


def f0_track_lds_bytes(n_bins, max_step):
    """f0_track_lds_bytes of the same header."""
    if n_bins < 1 or max_step < 0:
        return 0
    if max(n_bins, max_step) > 1 << 24:
        return (1 << 63) - 1
    return 8 * (4 * (n_bins + 2 * max_step) + 2 * n_bins) + F0_TRACK_TB * 2 * n_bins + 8


def f0_dp_ulps(W, tau):
    """FS2_F0_DP_ULPS of the same header: the bound on dp's relative error, in units of 2^-53."""
    return 2 * W + tau + 6


def header_symbols(header_path):
    """Every ``fs2_*`` function declared in include/fs2hip.h (for the export test)."""
    import re

    text = open(header_path).read()
    return sorted(set(re.findall(r"\b(fs2_[a-z0-9_]+)\s*\(", text)) - {"fs2_conv_desc"})


_LIB = None
CSRC = os.path.join(os.path.dirname(HERE), "csrc")
HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "fs2hip.h")
HEADER_PROSODY = os.path.join(os.path.dirname(HEADER), "fs2hip_prosody.h")
# public headers beside fs2hip.h that the sources include: part of the build id
HEADER_AUDIO = os.path.join(os.path.dirname(HEADER), "fs2hip_audio.h")
HEADER_AUDIO_INV = os.path.join(os.path.dirname(HEADER), "fs2hip_audio_inv.h")
HEADER_PREP = os.path.join(os.path.dirname(HEADER), "fs2hip_prep.h")
HEADER_F0 = os.path.join(os.path.dirname(HEADER), "fs2hip_f0.h")
HEADER_RESAMPLE = os.path.join(os.path.dirname(HEADER), "fs2hip_resample.h")
HEADER_ALIGN = os.path.join(os.path.dirname(HEADER), "fs2hip_align.h")
HEADER_EVAL = os.path.join(os.path.dirname(HEADER), "fs2hip_eval.h")
HEADER_F0_TRACK = os.path.join(os.path.dirname(HEADER), "fs2hip_f0_track.h")
HEADER_VAD = os.path.join(os.path.dirname(HEADER), "fs2hip_vad.h")
HEADER_PVOC = os.path.join(os.path.dirname(HEADER), "fs2hip_pvoc.h")
HEADER_IIR = os.path.join(os.path.dirname(HEADER), "fs2hip_iir.h")
HEADER_POSTNET = os.path.join(os.path.dirname(HEADER), "fs2hip_postnet.h")
HEADER_COND_MIX = os.path.join(os.path.dirname(HEADER), "fs2hip_cond_mix.h")
EXTRA_HEADERS = ("fs2hip_prosody.h", "fs2hip_audio.h", "fs2hip_audio_inv.h", "fs2hip_prep.h", "fs2hip_f0.h",
                 "fs2hip_resample.h", "fs2hip_align.h", "fs2hip_eval.h", "fs2hip_f0_track.h", "fs2hip_vad.h",
                 "fs2hip_pvoc.h", "fs2hip_iir.h", "fs2hip_postnet.h", "fs2hip_cond_mix.h")


def source_build_id(csrc=CSRC, header=HEADER):
    """sha256 (first 16 hex digits) of csrc/*.hip, csrc/*.h, include/fs2hip.h and the EXTRA_HEADERS
    beside it, in name order: the id __graft_entry__.build_hip embeds as fs2_build_id(). None when
    the sources are absent."""
    import hashlib

    if not os.path.isdir(csrc) or not os.path.exists(header):
        return None
    h = hashlib.sha256()
    for name in sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h"))):
        h.update(name.encode())
        with open(os.path.join(csrc, name), "rb") as f:
            h.update(f.read())
    with open(header, "rb") as f:
        h.update(b"fs2hip.h")
        h.update(f.read())
    for name in EXTRA_HEADERS:
        with open(os.path.join(os.path.dirname(header), name), "rb") as f:
            h.update(name.encode())
            h.update(f.read())
    return h.hexdigest()[:16]


def lib_path():
    return os.environ.get("FS2_LIB", DEFAULT_LIB)


def load():
    """Load (once) and return the ctypes library; raises if it was not built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"fs2amd: HIP library not found at {path}. Build it with `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    # FS2_LIB_ALLOW_MISSING=1 (A/B runs against an older library build only): skip entry points
    # the override library does not export; calling one of them then raises AttributeError.
    allow_missing = "FS2_LIB" in os.environ and os.environ.get("FS2_LIB_ALLOW_MISSING") == "1"
    for name, (res, args) in list(SIGNATURES.items()) + list(SIGNATURES_PROSODY.items()) + \
            list(SIGNATURES_AUDIO.items()) + list(SIGNATURES_AUDIO_INV.items()) + list(SIGNATURES_PREP.items()) + \
            list(SIGNATURES_F0.items()) + list(SIGNATURES_RESAMPLE.items()) + list(SIGNATURES_ALIGN.items()) + \
            list(SIGNATURES_EVAL.items()) + list(SIGNATURES_F0_TRACK.items()) + list(SIGNATURES_VAD.items()) + \
            list(SIGNATURES_PVOC.items()) + list(SIGNATURES_IIR.items()) + list(SIGNATURES_POSTNET.items()) + \
            list(SIGNATURES_COND_MIX.items()):
        if allow_missing and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    # provenance: the default in-tree library must have been built from the sources beside it
    # (FS2_LIB overrides are A/B builds of other trees and are not checked)
    if "FS2_LIB" not in os.environ:
        want = source_build_id()
        got = lib.fs2_build_id().decode()
        if want is not None and got != want:
            raise RuntimeError(f"fs2amd: {path} was built from other sources (fs2_build_id {got}, sources "
                               f"{want}); rebuild with `python -c 'import __graft_entry__ as g; g.build()'`")
    _LIB = lib
    return lib


def check(rc, what):
    if rc != FS2_OK:
        msg = load().fs2_status_string(rc).decode()
        raise RuntimeError(f"{what} failed: fs2 status {rc} ({msg})")
