/*
 * fs2hip_prep.h — corpus preprocessing after feature extraction: the phoneme-level pitch target
 * (the reference's preprocessor/preprocessor.py:263-291), the outlier fence and the running
 * mean / variance behind stats.json (:152-155, :367-375), and the normalisation pass with its
 * minimum and maximum (:161-180, :377-388). F0 estimation is not here: the contour is an input.
 *
 * Arithmetic. Every f64 operation named below (and every f32 one of the f32 percentile) is one
 * IEEE round-to-nearest operation on the device; none is contracted into an FMA.
 *
 * Pitch target, per utterance b over f0[b, :] (f64, 0 = unvoiced; anything != 0, NaN included,
 * is voiced, as numpy's `pitch != 0`):
 *   n         = min(max(frames[b], 0), T, sum_i max(dur[b, i], 0))
 *   voiced[b] = number of voiced frames among the first n
 *   voiced[b] <= 1: the reference drops the utterance; here its out and filled rows are 0.
 *   otherwise, with first / second / last the first, second and last voiced frame and t < n:
 *     t < first: filled[t] = f0[first];   t > last: filled[t] = f0[last];   else
 *     hi = first voiced frame >= t, but second when t == first;  lo = the voiced frame before hi
 *     slope = (f0[hi] - f0[lo]) / (double)(hi - lo)
 *     filled[t] = slope * (double)(t - lo) + f0[lo]
 *   which is scipy.interpolate.interp1d(kind="linear", bounds_error=False, fill_value=(f0[first],
 *   f0[last])) over the voiced frames, operation for operation: searchsorted(side="left") clipped
 *   to [1, voiced - 1]. A voiced frame other than the first goes through the formula with hi = t;
 *   it is not copied. filled[t] = 0 for n <= t < T.
 *   out[b, i] = mean(filled[s_i : min(s_i + d_i, n)]), s_i = sum_{j<i} max(dur[b, j], 0), summed left
 *   to right in f64 and divided once; 0 where the segment is empty (d_i <= 0 or s_i >= n). This is
 *   the plain mean: the reference's loop writes into the array it reads and equals it under the
 *   condition fs2hip_audio.h states for fs2_segment_mean. Padding entries of dur are 0 and so
 *   give 0.
 *   One workgroup per utterance. The index of the last voiced frame before t and of the first at
 *   or after t come from a forward max scan and a backward min scan over the voiced mask: inside a
 *   wave on its ballot word, across waves and across passes of 256 frames through carries kept in
 *   LDS. No atomics; the result for an utterance does not depend on B, on its place in the batch,
 *   on T or on the row stride.
 *
 * Outlier fence, per utterance over v = values[b, :n], n = clamp(lens[b], 0, n_max), in the
 * element type E (f32 or f64) throughout:
 *   sorted = sort(v) (bitonic network in LDS, padded with +inf)
 *   p_q for q = 25, 75: vi = (q / 100) * (E)(n - 1), lo = floor(vi), g = vi - lo (a multiple of
 *     0.25), a = sorted[lo], b = sorted[min(lo + 1, n - 1)], diff = b - a,
 *     p_q = g >= 0.5 ? b - diff * (1 - g) : a + diff * g          (numpy's default "linear" method)
 *   lower = p25 - 1.5 * (p75 - p25),  upper = p75 + 1.5 * (p75 - p25)
 *   inlier[i] = lower < v[i] && v[i] < upper    (strict: n = 1 has no inlier; NaN is never one)
 *   A NaN anywhere in v makes both quartiles NaN (as numpy does) and so leaves no inlier. n = 0
 *   gives NaN quartiles and count 0.
 *   count = number of inliers; mean = (sum of the inliers as f64) / count; m2 = sum of
 *   (v[i] - mean)^2 over the inliers, in f64. Both sums run over the original order: thread k of
 *   256 adds elements [k * per, (k + 1) * per), per = ceil(n / 256), left to right, and the 256
 *   partial sums are added in thread order. count = 0 gives mean = m2 = 0.
 *
 * The running state of fs2_moments_merge is {count, mean, m2} as three f64. Partials are folded in
 * index order with Chan's update: n = n_a + n_b, delta = mean_b - mean_a,
 * mean = mean_a + delta * (n_b / n), m2 = m2_a + m2_b + delta * delta * (n_a * n_b / n); an empty
 * partial is skipped and an empty state takes the first partial as it is. The population variance
 * sklearn's StandardScaler reports is m2 / count.
 *
 * Normalisation: out[b, i] = ((double)values[b, i] - mean) / std for i < n, 0 past it; minmax =
 * {min, max} of out over all valid entries (NaN entries are skipped; no valid entry at all gives
 * {DBL_MAX, -DBL_MAX}, the reference's initial values).
 */
#ifndef FS2HIP_PREP_H
#define FS2HIP_PREP_H

#include "fs2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one more element type beside the fs2hip.h dtype codes and FS2_I16, for the entry points below only */
#define FS2_F64 4 /* IEEE double */

#define FS2_PITCH_T_MAX 131072      /* frames per utterance row the scan carries cover            */
#define FS2_PITCH_T_MAX_NOFILL 4096 /* the same when filled is NULL (the contour is kept in LDS)  */
#define FS2_OUTLIER_LDS_BYTES 65536 /* n_max * sizeof(element) may not exceed it: 8192 f64         */

/*
 * f0 f64 [B, T] with f0_row_stride >= T elements between utterances; frames int64 [B] or NULL
 * (= T each); dur int64 [B, L] contiguous; out f64 [B, L]; filled f64 [B, T] contiguous or NULL
 * (not kept); voiced int32 [B]. All device memory. One launch.
 * FS2_EINVAL: a NULL required pointer, B / T / L < 1, f0_row_stride < T. FS2_EUNSUPPORTED:
 * T > FS2_PITCH_T_MAX, T > FS2_PITCH_T_MAX_NOFILL with filled NULL, B > 65535.
 */
int fs2_pitch_targets(const double *f0, int64_t f0_row_stride, const int64_t *frames, const int64_t *dur, int B, int T,
                      int L, double *out, double *filled, int32_t *voiced, fs2_stream_t stream);

/*
 * values [B, n_max] of dtype FS2_F32 or FS2_F64 with row_stride >= n_max elements; lens int64 [B]
 * or NULL (= n_max each); quartiles [B, 2] of the same dtype (p25, p75); inlier uint8 [B, n_max]
 * (0 / 1, 0 past n); count int64 [B]; mean, m2 f64 [B]. One launch, one workgroup per utterance.
 * FS2_EINVAL: a NULL required pointer, B / n_max < 1, row_stride < n_max. FS2_EUNSUPPORTED: another
 * dtype, n_max * sizeof(element) > FS2_OUTLIER_LDS_BYTES, B > 65535.
 */
int fs2_outlier_moments(const void *values, int dtype, int64_t row_stride, const int64_t *lens, int B, int n_max,
                        void *quartiles, uint8_t *inlier, int64_t *count, double *mean, double *m2,
                        fs2_stream_t stream);

/*
 * Folds count / mean / m2 [B] (as fs2_outlier_moments writes them) into state f64 [3] =
 * {count, mean, m2}, device memory, zero-initialised by the caller before the first call. One
 * launch of one wave. FS2_EINVAL: a NULL pointer or B < 1.
 */
int fs2_moments_merge(const int64_t *count, const double *mean, const double *m2, int B, double *state,
                      fs2_stream_t stream);

/* bytes of workspace fs2_normalize_minmax needs for B utterances (0 for B < 1) */
int64_t fs2_normalize_minmax_ws_bytes(int B);

/*
 * values / dtype / row_stride / lens / B / n_max as fs2_outlier_moments (no cap on n_max); mean
 * and std host doubles; out f64 [B, n_max]; minmax f64 [2]; ws device workspace of ws_bytes >=
 * fs2_normalize_minmax_ws_bytes(B). Two launches: per-utterance partial minima and maxima, then
 * one finishing workgroup; no atomics.
 * FS2_EINVAL: a NULL required pointer, B / n_max < 1, row_stride < n_max, a workspace too small.
 * FS2_EUNSUPPORTED: another dtype, B > 65535.
 */
int fs2_normalize_minmax(const void *values, int dtype, int64_t row_stride, const int64_t *lens, int B, int n_max,
                         double mean, double std, double *out, double *minmax, void *ws, int64_t ws_bytes,
                         fs2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FS2HIP_PREP_H */
