/*
 * fs2hip_eval.h — objective evaluation of a synthesised utterance against its recording: mel
 * cepstra, pairwise distances, dynamic time warping (DTW) and statistics along the warping path,
 * over a ragged batch. Mel-cepstral distortion (Kubichek 1993) is the mean distance along the DTW
 * path (Sakoe & Chiba 1978) times 10 / ln 10 * sqrt 2; F0 error and voicing error are read along the
 * same path. The reference has none of this; the definitions below are the whole specification.
 *
 * Every operation below is one IEEE float64 operation, none contracted; float32 input is widened on
 * load (exact). Utterance b has T_b = clamp(lens[b], 0, T_max) frames (NULL: the maximum); nothing
 * outside an utterance's own lengths is read, so the padding may hold anything, NaN included.
 *
 * fs2_mel_cepstrum — mel [B, T_max, M], FS2_F32 or FS2_F64, unit stride along M, any row stride >= M
 *   and batch stride >= T_max rows; basis f64 [C, M] contiguous (the caller's table: Python uploads
 *   the orthonormal DCT-II rows 1 .. C, sqrt(2 / M) cos(pi / M (m + 1/2) q)):
 *     c[b,t,q] = sum_{m = 0 .. M-1} mel[b,t,m] * basis[q,m],   s = 0; s = s + mel * basis in index order
 *   out f64 [B, T_max, C] contiguous; rows t >= T_b are zeros. Determined bit for bit.
 *
 * fs2_pair_dist — x [B, Tx_max, D], y [B, Ty_max, D] (one dtype, FS2_F32 or FS2_F64; unit stride
 *   along D, any row stride >= D and batch stride):
 *     s = 0; for d = 0 .. D-1: e = x[b,i,d] - y[b,j,d]; s = s + e * e;     c[b,i,j] = sqrt(s)
 *   out f64 [B, Tx_max, Ty_max] contiguous, zeros outside [Tx_b, Ty_b]; with squared != 0 it holds s
 *   itself. s is determined bit for bit; sqrt is the device library's float64 square root.
 *
 * fs2_dtw — over the same x, y and the same c (one inlined device function serves both entries):
 *     A[0,0] = c[0,0]; otherwise p = A[i-1,j-1], u = A[i-1,j], l = A[i,j-1], a missing one is +inf;
 *     step[i,j] = 0 (diagonal) if p <= u && p <= l, else 1 (up, i - 1) if u <= l, else 2 (left, j - 1)
 *     A[i,j] = c[i,j] + (p, u or l by step[i,j])
 *   backtrack from (Tx_b - 1, Ty_b - 1) to (0, 0) by the stored steps.
 *   total f64 [B] = A[Tx_b-1, Ty_b-1]; K int32 [B] = cells on the path, max(Tx_b, Ty_b) <= K <=
 *   Tx_b + Ty_b - 1; path_i, path_j int32 [B, Tx_max + Ty_max - 1] in forward order ((0, 0) first),
 *   -1 from K_b on. An utterance with Tx_b = 0 or Ty_b = 0 is skipped: +inf, 0, all -1.
 *   One add and at most three comparisons per cell, no reduction: given c, everything is determined
 *   bit for bit. The tie rule is stated in the caller's (i, j) and the kernel never swaps x and y.
 *   A is never stored: one 256-thread workgroup walks the anti-diagonals e = i + j of one utterance
 *   at a time, three of them rotating in LDS as rows of Tx_max + 3 f64 indexed by i (slot 1 + i; the
 *   slots on either side of a diagonal's cells hold +inf), one barrier per anti-diagonal. The steps
 *   take 2 bits per cell: for anti-diagonal e and the 64 cells i = 64 w .. 64 w + 63 the ballot
 *   words of "step = 1" and "step = 2" at 64-bit words (e * W + w) * 2 and + 1, W = ceil(Tx_max / 64);
 *   that bitmap of (Tx_max + Ty_max - 1) * 2 W words lives in LDS when fs2_dtw_lds_bytes(Tx_max,
 *   Ty_max, 1) <= FS2_DTW_LDS_BYTES and in the caller's workspace (fs2_dtw_ws_bytes) otherwise, or
 *   when asked for. Same bits out either way.
 *
 * fs2_path_stats — tracks a [B, Tx_max, Ch], b [B, Ty_max, Ch], f64 contiguous, NaN = absent, along
 *   the path k = 0 .. K_b - 1 in that order (K_b clamped to [0, Tx_max + Ty_max - 1]; the walk ends
 *   early at an index outside [0, Tx_max) x [0, Ty_max)). Per utterance and channel:
 *   counts int64 [B, Ch, 4] = n_both, n_a_only, n_b_only, n_none;
 *   sums f64 [B, Ch, 2] = sum d, sum d * d over the both-present pairs, d = a[i_k] - b[j_k],
 *   s = s + d and s2 = s2 + d * d in k order from zero. One thread per (b, ch). Determined bit for bit.
 */
#ifndef FS2HIP_EVAL_H
#define FS2HIP_EVAL_H

#include "fs2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS2_DTW_LDS_BYTES 163840 /* the LDS of one workgroup: three anti-diagonals of (Tx_max + 3) f64, then
                                    (bitmap in LDS) (Tx_max + Ty_max - 1) * 2 * ceil(Tx_max / 64) 64-bit words */
#define FS2_DTW_LDS_SMALL 32768  /* launches that need no more than this use the small form: more than
                                    one workgroup per compute unit                                  */
#define FS2_DTW_AUTO 0
#define FS2_DTW_LDS 1
#define FS2_DTW_GLOBAL 2

/* bytes of LDS the DTW needs with the bitmap in LDS (in_lds != 0) or in the workspace; 0 for a size
 * < 1, INT64_MAX for a size beyond 2^24 */
int64_t fs2_dtw_lds_bytes(int Tx_max, int Ty_max, int in_lds);
/* bytes of the workspace of the global form: B * (Tx_max + Ty_max - 1) * 2 * ceil(Tx_max / 64) * 8
 * (0 for a size < 1, INT64_MAX beyond the cap or past 63 bits) */
int64_t fs2_dtw_ws_bytes(int B, int Tx_max, int Ty_max);

/* FS2_EINVAL: a NULL mel / basis / out, B / T_max / M / C < 1, strides too small, more than 2^31 - 1
 * outputs. FS2_EUNSUPPORTED: another dtype. */
int fs2_mel_cepstrum(const void *mel, int dtype, int64_t batch_stride, int64_t row_stride, const int64_t *lens,
                     const double *basis, int B, int T_max, int M, int C, double *out, fs2_stream_t stream);

/* FS2_EINVAL: a NULL x / y / out, a size < 1, strides too small, more than 2^31 - 1 outputs.
 * FS2_EUNSUPPORTED: another dtype. */
int fs2_pair_dist(const void *x, const void *y, int dtype, int64_t x_batch_stride, int64_t x_row_stride,
                  int64_t y_batch_stride, int64_t y_row_stride, const int64_t *x_lens, const int64_t *y_lens, int B,
                  int Tx_max, int Ty_max, int D, int squared, double *out, fs2_stream_t stream);

/*
 * bitmap: FS2_DTW_AUTO (LDS where it fits), FS2_DTW_LDS, FS2_DTW_GLOBAL. ws: device memory of at least
 * fs2_dtw_ws_bytes (global form; may be NULL otherwise). FS2_EINVAL: a NULL x / y / output, a size
 * < 1, strides too small, an unknown bitmap, a workspace too small. FS2_EUNSUPPORTED: another dtype,
 * FS2_DTW_LDS beyond FS2_DTW_LDS_BYTES, rows that do not fit the LDS at all.
 */
int fs2_dtw(const void *x, const void *y, int dtype, int64_t x_batch_stride, int64_t x_row_stride,
            int64_t y_batch_stride, int64_t y_row_stride, const int64_t *x_lens, const int64_t *y_lens, int B,
            int Tx_max, int Ty_max, int D, int bitmap, void *ws, int64_t ws_bytes, double *total, int32_t *K,
            int32_t *path_i, int32_t *path_j, fs2_stream_t stream);

/* FS2_EINVAL: a NULL pointer, a size < 1. */
int fs2_path_stats(const double *a, const double *b, const int32_t *path_i, const int32_t *path_j, const int32_t *K,
                   int B, int Tx_max, int Ty_max, int Ch, int64_t *counts, double *sums, fs2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FS2HIP_EVAL_H */
