/*
 * fs2hip_resample.h — raw audio to the waveforms the corpus chain reads: the arithmetic of the
 * reference's prepare_align step (preprocessor/esd_chinese.py:145-147: load at the target rate,
 * wav / max(abs(wav)) * max_wav_value, astype(int16)) as a rational polyphase FIR resampler and a
 * peak normalisation. The resampler is NOT librosa's default (soxr_hq); it is scipy's
 * signal.resample_poly, restated operation by operation below and reproduced bit for bit.
 *
 * Ratio. g = gcd(target, source), up = target / g, down = source / g. One launch has one (up, down).
 *
 * Taps (host: fs2amd.audio.resample_taps, float64; scipy's default design).
 *   half = 10 * max(up, down), N = 2 * half + 1, c = 1 / max(up, down)
 *   h0[k] = c * sinc(c * (k - half)) * kaiser(N, beta = 5)[k], divided by its sum
 *   h[k]  = h0[k] * up   (one f64 multiply per tap, as scipy does); the launch takes h.
 *
 * Resample. Per utterance b: samples x[0..n), n = clamp(lens[b], 0, n_max), int16 or f32, each
 * converted to double exactly.
 *   M = ceil(n * up / down)                                   (64-bit integers)
 *   for 0 <= m < M:  c = m * down + half
 *     lo = max(0, ceil((c - 2 * half) / up)),  hi = min(n - 1, floor(c / up))
 *     y[m] = sum over i = lo .. hi, ASCENDING, of h[c - i * up] * x[i]
 *   The accumulator starts at +0.0; each term is one f64 multiply, then one f64 add, never
 *   contracted into an FMA; an empty range gives +0.0. The order is fixed, so y is determined bit
 *   for bit: it equals scipy.signal.resample_poly(x, up, down, window=h0) for either sample type,
 *   and an f32 input k * 2^-15 gives exactly 2^-15 times the output of its int16 twin k.
 *   All index arithmetic is 64-bit (m * down passes 2^31 at about five minutes of 16 kHz audio).
 *   up == down == 1 skips the FIR: y[m] = (double)x[m] (scipy returns a copy); taps may be NULL.
 *
 * To int16.
 *   y32  = (float)y[m]                       one rounding
 *   peak = max |y32| over the utterance      exact and order-free (here: per-wave maxima merged by
 *                                            an integer atomic max on the bits of |y32|)
 *   v    = (y32 / peak) * max_wav_value      in f32: the quotient is computed as an f64 divide
 *                                            rounded to f32, which is the correctly rounded f32
 *                                            quotient (53 >= 2 * 24 + 2); then one f32 multiply
 *   q    = trunc(v) toward zero, SATURATED to [-32768, 32767]
 *   Saturation is the one deliberate departure from the reference: with max_wav_value = 32768 the
 *   positive peak is exactly 32768.0, whose cast to int16 is undefined in numpy and wraps to -32768
 *   on x86, a full-scale click. Everywhere else q equals v.astype(np.int16).
 *   peak == 0 or M == 0 gives zeros and peak = 0 (the reference divides by zero). Non-finite input
 *   is out of contract; nothing outside the output rows is written in any case.
 *
 * Layout: workgroups of 512 threads, at most two per compute unit, each staging the whole tap
 * table once in LDS (padded by one f64 per 32, since neighbouring outputs read taps `down` apart)
 * and then walking tiles of 2048 outputs of the batch, one output per thread at a time. An
 * utterance's result does not depend on B, on its place in the batch, on n_max or on the row stride.
 */
#ifndef FS2HIP_RESAMPLE_H
#define FS2HIP_RESAMPLE_H

#include "fs2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS2_RESAMPLE_LDS_BYTES 81920 /* the staging limit: 8 * (N + N / 32 + 1) bytes for N taps may not
                                        exceed it, so max(up, down) <= 496 (441/320: 72776 bytes; a
                                        size above 2^24 counts as beyond it)                          */

/* ceil(n * up / down) in 64 bits; 0 for n < 1; -1 for up or down < 1 */
int64_t fs2_resample_out_len(int64_t n, int64_t up, int64_t down);

/* bytes of LDS a launch with this ratio stages: the formula beside FS2_RESAMPLE_LDS_BYTES with
 * N = 20 * max(up, down) + 1 (0 for up or down < 1) */
int64_t fs2_resample_lds_bytes(int64_t up, int64_t down);

/*
 * wav [B, n_max] of dtype FS2_I16 or FS2_F32 with row_stride >= n_max elements between utterances;
 * lens int64 [B] or NULL (= n_max each); taps f64 [n_taps] = h above, n_taps = 20 * max(up, down) + 1
 * (ignored, and may be NULL, when up == down == 1). With M_max = fs2_resample_out_len(n_max, up, down):
 * y f64 [B, M_max] or NULL, y32 f32 [B, M_max], both 0 past M_b; peak f32 [B]; out_lens int64 [B]
 * = M_b, or NULL. All device memory. One launch after a memset of peak.
 * FS2_EINVAL: wav, y32 or peak NULL, taps NULL where needed, B / n_max < 1, row_stride < n_max, up
 * or down < 1, n_taps != 20 * max(up, down) + 1. FS2_EUNSUPPORTED: another dtype,
 * fs2_resample_lds_bytes(up, down) > FS2_RESAMPLE_LDS_BYTES, M_max > INT32_MAX.
 */
int fs2_resample(const void *wav, int dtype, int64_t row_stride, const int64_t *lens, int B, int n_max, int up,
                 int down, const double *taps, int n_taps, double *y, float *y32, float *peak, int64_t *out_lens,
                 fs2_stream_t stream);

/*
 * y32 f32 [B, M_max], peak f32 [B], out_lens int64 [B] or NULL (= M_max each) -> q int16 [B, M_max]
 * by the rule above, 0 at and past out_lens[b] and for peak[b] == 0. One launch.
 * FS2_EINVAL: y32, peak or q NULL, B / M_max < 1. FS2_EUNSUPPORTED: B > 65535.
 */
int fs2_peak_int16(const float *y32, const float *peak, const int64_t *out_lens, int B, int M_max,
                   float max_wav_value, int16_t *q, fs2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FS2HIP_RESAMPLE_H */
