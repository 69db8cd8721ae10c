/*
 * fs2hip_prosody.h — per-phoneme prosody control maps: the entry points of libfs2hip.so that take a
 * pitch / energy / duration control per phoneme instead of one scalar per launch.
 *
 * The reference's VarianceAdaptor multiplies the pitch and energy predictions and the rounded
 * durations by `control` (model/modules.py:80-100,117-135), a plain broadcast: a [B, L_src] tensor
 * there gives each phoneme its own factor. Every entry of fs2hip.h that consumes a control has a
 * sibling here with the same arguments plus a map pointer:
 *
 *   control map: f32 [B, L] contiguous in device memory, indexed like the values it scales (b*L + i:
 *   as `dur` for the duration entries, as `target` / `pred` for the pitch / energy entries). NULL
 *   means "use the scalar argument": the call is then exactly the fs2hip.h entry (which is itself a
 *   call of the same implementation with a NULL map). With a map the scalar argument is ignored.
 *   Every slot of the map is read, padded ones too (their predictions are 0, so the value does not
 *   matter as long as it is finite). The launches are those of the scalar entries: one more
 *   coalesced f32 load per phoneme, no extra launch.
 *
 * The control values then live in memory, not in kernel arguments: a captured graph serves every
 * map of its shape.
 */
#ifndef FS2HIP_PROSODY_H
#define FS2HIP_PROSODY_H

#include "fs2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Duration maps. d_map scales the rounded log-duration prediction per phoneme:
 *   d_rounded[b, i] = clamp(round_half_even(exp(d[b, i]) - 1) * d_map[b, i], min=0)   (f32)
 * and the frame count is its truncation, as with the scalar. A map is defined for
 * FS2_DUR_LOGPRED only: d_map != NULL with another dur_kind (or, for the fused entry, without
 * `dur`) is FS2_EINVAL. Other arguments, limits and outputs as the entry of the same name without
 * the _map suffix.
 */
int fs2_lr_durations_map(const void *dur, int dur_kind, float d_control, const float *d_map, int B, int L,
                         int32_t *cum, int64_t *mel_len, float *d_rounded, fs2_stream_t stream);
int fs2_length_regulate_map(const void *x, int x_dtype, const void *dur, int dur_kind, float d_control,
                            const float *d_map, int B, int L, int D, int T_out, const float *pe, void *out,
                            int out_dtype, int32_t *cum, int64_t *mel_len, float *d_rounded, int32_t *index_map,
                            fs2_stream_t stream);
int fs2_lr_fused_proj_map(const void *x, int x_dtype, const void *dur, int dur_kind, float d_control,
                          const float *d_map, const int32_t *cum_in, const int64_t *mel_len_in, int B, int L, int D,
                          int T_out, const float *pe, const int64_t *layout_lens, int32_t *cu, int32_t *row_pos,
                          int32_t *rowmap, void *out, int out_dtype, int32_t *cum, int64_t *mel_len,
                          float *d_rounded, const float *proj_src, const float *proj_pe, int NP, void *proj_out,
                          fs2_stream_t stream);

/*
 * Pitch / energy maps. control_map scales the prediction per row before the bucketize:
 *   v = target ? target[m] : (pred[m] *= control_map[m]);  x[m, :] += table[bucketize(v, bins)]
 * With a target the map is unused (the prediction stays unscaled), as the scalar is.
 */
int fs2_variance_embed_map(void *x, int x_dtype, float *pred, const float *target, float control,
                           const float *control_map, const float *bins, int n_bins, const float *table, int M, int D,
                           fs2_stream_t stream);
int fs2_vp_head_map(const float *y, int64_t y_row_stride, int B, int T, int G, int C, const float *gamma,
                    const float *beta, float eps, const float *lin_w, const float *lin_b, const int64_t *lens,
                    float *pred, int embed_group, void *x, int x_dtype, int64_t x_row_stride, int D,
                    const float *target, float control, const float *control_map, const float *bins, int n_bins,
                    const float *table, fs2_stream_t stream);

typedef struct fs2_vp_fused_map_desc {
  fs2_vp_fused_desc base;   /* as fs2_vp_fused                                                      */
  const float *control_map; /* f32 [B*L] or NULL: scales the embed group's prediction per row       */
} fs2_vp_fused_map_desc;

int fs2_vp_fused_map(const fs2_vp_fused_map_desc *d, fs2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FS2HIP_PROSODY_H */
