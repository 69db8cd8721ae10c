/*
 * fs2hip_f0.h — F0 contours from waveforms: the one input of the corpus chain the reference takes
 * from outside (pyworld's DIO + StoneMask, preprocessor/preprocessor.py:255-261). This is NOT that
 * algorithm. It is YIN (difference function, cumulative-mean normalisation, absolute threshold,
 * parabolic refinement), stated operation by operation below, and its values do not equal
 * pyworld's. What it keeps is the interface fs2_pitch_targets consumes: one value per hop at
 * sample k * hop, the same length rule, f64 values with 0 for unvoiced, WORLD's default range.
 *
 * Per utterance b: samples x[0..n), n = clamp(lens[b], 0, n_max), int16 or f32, each converted to
 * double (no clipping, no scaling: a power-of-two scale cancels exactly in dp below).
 * F_b = n / hop + 1 frames (integer division). Frame k starts at s = k * hop - (W + tau_max) / 2
 * (integer division); samples outside [0, n) read as 0.
 *
 * The table, per frame:
 *   d(0) = 0,  d(tau) = sum_{j < W} (x[s + j] - x[s + j + tau])^2      for tau = 1 .. tau_max
 *     The difference form, always: the expanded form x^2 + y^2 - 2xy cancels where the signal is
 *     periodic and does not meet the bound below. The subtraction is one f64 operation; the square
 *     is fused into the accumulation (one FMA per term); the order of the sum is free. Here the
 *     sum of a hop-sized block of j is computed once and shared by the W / hop frames over it.
 *   cum(tau) = d(1) + ... + d(tau), accumulated left to right
 *   dp(0) = 1,  dp(tau) = cum(tau) == 0 ? 1 : (d(tau) * (double)tau) / cum(tau)
 *     (one multiply, one divide)
 *
 * The pick; every operation from here on is one IEEE round-to-nearest operation, none contracted:
 *   t   = the smallest t in [tau_min, tau_max - 1] with dp(t) < thr; none: the frame is unvoiced
 *   tau = t advanced while t + 1 < tau_max && dp(t + 1) < dp(t)
 *   a = dp(tau - 1), b = dp(tau), c = dp(tau + 1)
 *   den = (a - 2 * b) + c;  delta = den > 0 ? (0.5 * (a - c)) / den : 0
 *   f = sr / ((double)tau + delta);  f0_floor <= f && f <= f0_ceil: f0 = f, else unvoiced
 *   An unvoiced frame has f0 = 0 and tau = 0. A NaN never satisfies <, so a NaN sample leaves the
 *   frames that read it unvoiced. tau_min >= 2 keeps a in the table and off dp(0).
 *   The caller derives tau_min = floor(sr / f0_ceil), tau_max = ceil(sr / f0_floor): 27 and 311 for
 *   71 .. 800 Hz at 22050 Hz.
 *
 * Exactness. For int16 samples, and for f32 samples that are k * 2^-15 with |k| <= 2^15, every
 * term, every d, every cum and every d * tau is an integer (times one power of two) below 2^53
 * as long as W * tau_max < 2^21: a term is below 2^32, d below W * 2^32, cum and d * tau below
 * W * tau_max * 2^32. Under that condition the table is the same bits in any summation order and
 * f0 and tau are determined bit for bit.
 * Outside it, with u = 2^-53 and to first order in u: a term (x - y)^2 carries the rounding of
 * the subtraction twice and one rounding of the fused multiply-add, 3 u relative; the terms are
 * non-negative, so a sum of W of them in ANY order adds at most (W - 1) u: d is within
 * (W + 2) u of the exact value. cum(tau) adds tau - 1 roundings to that: (W + tau + 1) u. dp adds
 * one for the multiply and one for the divide: (W + 2) + (W + tau + 1) + 2 = (2 W + tau + 5) u,
 * stated with one u to spare for the second-order terms as
 *   |dp - exact| <= FS2_F0_DP_ULPS(W, tau) * 2^-53 * exact,   FS2_F0_DP_ULPS(W, tau) = 2 W + tau + 6.
 *
 * Layout: one workgroup of 256 threads per utterance and FS2_F0_GROUP consecutive frames. The
 * span (FS2_F0_GROUP - 1) * hop + W + tau_pad samples, tau_pad = 8 * ceil(tau_max / 8), is staged
 * once in LDS as f64; a thread holds 8 consecutive lags of one hop block in registers; the block
 * sums, then the tables of the group's frames, live in LDS; one wave picks per frame with ballots.
 * One launch, no atomics: an utterance's result does not depend on B, on its place in the batch,
 * on n_max or on the row stride.
 */
#ifndef FS2HIP_F0_H
#define FS2HIP_F0_H

#include "fs2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS2_F0_GROUP 8         /* frames per workgroup                                          */
#define FS2_F0_LDS_BYTES 65536 /* the staging limit: with tau_pad as above, q = W / hop,
                                  segs = (q ? FS2_F0_GROUP + q - 1 : 0) + (W % hop ? FS2_F0_GROUP : 0),
                                  span = (FS2_F0_GROUP - 1) * hop + W + tau_pad:
                                  8 * (max(span + span / 8 + 1, FS2_F0_GROUP * (tau_pad + 1))
                                       + segs * (tau_pad + 1)) may not exceed it
                                  (hop 256, W 1024, tau_max 311: 55704; a size above 2^24
                                  counts as beyond it)                                         */
#define FS2_F0_DP_ULPS(W, tau) (2 * (W) + (tau) + 6)

/* bytes of LDS a launch with these sizes needs: the formula beside FS2_F0_LDS_BYTES (0 for a size < 1) */
int64_t fs2_f0_lds_bytes(int hop, int W, int tau_max);

/*
 * wav [B, n_max] of dtype FS2_I16 or FS2_F32 with row_stride >= n_max elements between utterances;
 * lens int64 [B] or NULL (= n_max each). f0 f64 [B, F_max], F_max = n_max / hop + 1, 0 past F_b;
 * tau int32 [B, F_max] or NULL; cmnd f64 [B, F_max, tau_max + 1] or NULL: the dp values the pick
 * compared, 0 for frames past F_b. All device memory. One launch.
 * FS2_EINVAL: wav or f0 NULL, B / n_max / hop / W < 1, row_stride < n_max, tau_min < 2,
 * tau_min >= tau_max. FS2_EUNSUPPORTED: another dtype, B > 65535,
 * fs2_f0_lds_bytes(hop, W, tau_max) > FS2_F0_LDS_BYTES.
 */
int fs2_f0_yin(const void *wav, int dtype, int64_t row_stride, const int64_t *lens, int B, int n_max, double sr,
               int hop, int W, int tau_min, int tau_max, double thr, double f0_floor, double f0_ceil, double *f0,
               int32_t *tau, double *cmnd, fs2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FS2HIP_F0_H */
