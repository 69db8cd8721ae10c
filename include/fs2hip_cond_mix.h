/*
 * fs2hip_cond_mix.h — the conditioning vectors of fs2hip.h's fs2_cond_vectors, with weights over the
 * rows of each embedding table in place of one id: utterance mixtures, and per-phoneme emotion curves.
 * It is what the model computes when every nn.Embedding(ids) is replaced by weights @ table:
 *
 *   e = w_e . E,  a = w_a . A,  v = w_v . V          mixed in embedding space
 *   emo = relu(W . cat(e, a, v) + b)                  the emotion Linear and ReLU after the mixing
 *   spk = w_s . S
 *
 * Weights are used as given: not normalised, any sum, negative entries allowed. They must be finite
 * (not checked: no host sync). Each conditioning input has a kind:
 *
 *   FS2_COND_NONE   absent (speaker only: speaker_table NULL)
 *   FS2_COND_IDS    int64 [B]; clamped into the table as fs2_cond_vectors does; acts as a one-hot row
 *   FS2_COND_MIX    f32 [B, n], n = the table's row count: one weight row per utterance
 *   FS2_COND_ROWS   f32 [B * L, n]: one weight row per position (fs2_cond_mix_rows only)
 *
 * Arithmetic, all f32, every order fixed:
 *   mixed embedding   per channel an fmaf chain over the table rows j = 0 .. n - 1 from +0.0f:
 *                     acc = fmaf(w[j], table[j][k], acc). A one-hot row of exact 1.0f / 0.0f gives the
 *                     table row (an id reads the row itself).
 *   Linear + ReLU     fs2_cond_vectors' own code (csrc/cond.h, cond_linear_tile): k in four quarters,
 *                     each quarter an fmaf chain in ascending k from +0.0f, the sum
 *                     ((r0 + r1) + (r2 + r3)) + b, then fmaxf(., 0). With (d_emo + d_aro + d_val) % 16
 *                     != 0 the quarters are ceil(k / 4) wide and the loads scalar, as there.
 * So with ids, or with one-hot f32 rows, both entry points give the bits of fs2_cond_vectors. A row's
 * output depends on its own weights and the parameters alone: not on B, L, its place in the batch or
 * in a tile, or on which of the two entry points computed it. No atomics, no workgroup waits for
 * another, plain VALU (0.13 MFLOP per row).
 */
#ifndef FS2HIP_COND_MIX_H
#define FS2HIP_COND_MIX_H

#include "fs2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS2_COND_NONE 0
#define FS2_COND_IDS 1
#define FS2_COND_MIX 2
#define FS2_COND_ROWS 3

typedef struct fs2_cond_mix_desc {
  const void *speakers; int spk_kind; const float *speaker_table; int n_speaker;   /* table [n_speaker, D] */
  const void *emotions; int emo_kind; const float *emo_table; int n_emo, d_emo;    /* table [n_emo, d_emo] */
  const void *arousals; int aro_kind; const float *aro_table; int n_aro, d_aro;
  const void *valences; int val_kind; const float *val_table; int n_val, d_val;
  const float *lin_w, *lin_b;   /* [D, d_emo + d_aro + d_val], [D] */
  int B, D;
  float *spk_out, *emo_out;     /* f32 [B, D] each (fs2_cond_mix) */
} fs2_cond_mix_desc;

/*
 * Utterance level, one launch: spk_out[b] and emo_out[b], fs2_cond_vectors' outputs, which the
 * encoder's addvec epilogues take unchanged. speaker_table NULL: no speaker part (spk_kind
 * FS2_COND_NONE, spk_out not written); emo_table NULL: no emotion part. Tiles of 64 channels x 8
 * utterances, the grid of fs2_cond_vectors.
 *
 * FS2_EINVAL, nothing launched:
 *   1. d NULL
 *   2. B < 0 or D <= 0
 *   3. speaker_table given and: spk_kind not FS2_COND_IDS / FS2_COND_MIX, speakers or spk_out NULL,
 *      or n_speaker <= 0
 *   4. emo_table given and: a kind of emotions / arousals / valences that is not FS2_COND_IDS /
 *      FS2_COND_MIX (FS2_COND_ROWS belongs to fs2_cond_mix_rows), one of the three pointers NULL
 *   5. emo_table given and: aro_table, val_table, lin_w, lin_b or emo_out NULL
 *   6. emo_table given and: n_emo, n_aro, n_val, d_emo, d_aro or d_val <= 0
 * FS2_EUNSUPPORTED: d_emo + d_aro + d_val > 1792 (the tile's LDS, 8 * (dc + 256) floats, is 64 KB at most).
 * FS2_OK without a launch: B == 0, or both tables NULL.
 */
int fs2_cond_mix(const fs2_cond_mix_desc *d, fs2_stream_t stream);

/*
 * Per-phoneme curves, one launch: x[b, i, :] += emo(b, i) in place for every i < L (padded positions
 * included), x [B, L, D] contiguous, f32 or bf16 (bf16: one rounding to nearest-even of
 * float(x) + emo). Each of emotions / arousals / valences is FS2_COND_IDS [B], FS2_COND_MIX [B, n]
 * (both broadcast over L) or FS2_COND_ROWS [B * L, n]. The speaker fields, spk_out and emo_out of d
 * are not read. Row tiles of 16 positions; the emotion vectors live in LDS only (no [B * L, D]
 * intermediate).
 *
 * FS2_EINVAL, nothing launched:
 *   1. d or x NULL
 *   2. B < 0, L < 0 or D <= 0
 *   3. emo_table NULL
 *   4. a kind of emotions / arousals / valences outside FS2_COND_IDS / _MIX / _ROWS, or one of the
 *      three pointers NULL
 *   5. aro_table, val_table, lin_w or lin_b NULL
 *   6. n_emo, n_aro, n_val, d_emo, d_aro or d_val <= 0
 * FS2_EUNSUPPORTED: x_dtype other than FS2_F32 / FS2_BF16; d_emo + d_aro + d_val > 768 (16 *
 * (dc + 256) floats of LDS, 64 KB at most); B * L >= 2^31.
 * FS2_OK without a launch: B * L == 0.
 */
int fs2_cond_mix_rows(const fs2_cond_mix_desc *d, int L, void *x, int x_dtype, fs2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FS2HIP_COND_MIX_H */
