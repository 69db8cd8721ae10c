/*
 * fs2hip_pvoc.h — the phase vocoder between the two transforms of include/fs2hip_audio_inv.h: a
 * spectrum of T frames resampled along time to J frames at `rate` input frames per output frame, with a
 * running phase per bin. It is the rule of librosa.phase_vocoder (and, with the Python layers,
 * librosa.effects.time_stretch / pitch_shift), stated here as this project's own arithmetic in float64.
 * It is librosa's rule, NOT librosa's bits, and it is written without angles: librosa accumulates
 * phase_acc += phi_advance + wrap(angle(D1) - angle(D0) - phi_advance) and outputs mag * exp(i phase_acc);
 * under exp the wrap and phi_advance cancel, so the output phasor is a running product of the unit
 * rotors unit(D1) * conj(unit(D0)). Only * + - / sqrt in float64 are used, each correctly rounded and
 * none contracted into an FMA, so the result is determined bit for bit.
 *
 * Per row b: spec f32 [2 NB, T_max], real rows then imaginary rows, as fs2_stft writes it;
 * T = clamp(frames[b], 0, T_max); rate = rates[b], f64.
 *
 * 1. Output frames. J = the number of j >= 0 with fl((double)j * rate) < T, saturated at
 *    FS2_PVOC_J_CAP = 2^31 - 1; J = 0 for a rate that is not finite or is <= 0 (NaN included) and for
 *    T = 0. fs2_pvoc_frames(T, rate) gives the same value on the host. This is the project's own rule:
 *    it equals len(numpy.arange(0, T, rate)), librosa's count, except at rounding edges (6 of 20,000
 *    random (T, rate) pairs differed).
 *
 * 2. Per input frame i < T, with re, im widened to double exactly:
 *      m[i] = sqrt(re * re + im * im)           each square exact; one rounded add, one sqrt
 *      e[i] = (re / m[i], im / m[i]), or (1, 0) where m[i] == 0
 *    Frame T is the zero pad: m[T] = 0, e[T] = (1, 0).
 *
 * 3. Per output frame j < J: p = (double)j * rate, i = floor(p), alpha = p - i (exact); i <= T - 1.
 *      mag_j   = (1 - alpha) * m[i] + alpha * m[i + 1]        one subtract, two multiplies, one add
 *      rotor_j = e[i + 1] * conj(e[i]) = (a1 * a0 + b1 * b0, b1 * a0 - a1 * b0)
 *    with e[i] = (a0, b0), e[i + 1] = (a1, b1).
 *
 * 4. The scan. s_0 = e[0], s_k = rotor_{k - 1} for k >= 1. P_j is the inclusive prefix of s under
 *    (x, y) (*) (u, v) = (x * u - y * v, x * v + y * u), every product and sum rounded on its own.
 *    (*) is commutative bit for bit but not associative, so the order is fixed: blocks of
 *    FS2_PVOC_BLOCK = 64 consecutive j. Inside a block a Kogge-Stone scan: for d = 1, 2, 4, .., 32,
 *    x[k] = x[k - d] (*) x[k] for all k >= d at once. Block 0 is taken as it stands; block c >= 1 is
 *    carry_c (*) x[k] with carry_c = P_{64 c - 1}, the last element of the block before it. The order
 *    depends on j and the row's own data only: not on B, the batch slot, T_max, J_max, a stride or
 *    the launch.
 *
 * 5. Output. recomb[k, j] = (float)(mag_j * P_j.re), recomb[NB + k, j] = (float)(mag_j * P_j.im) for
 *    j < min(J, J_max); columns from there to J_max are written 0. frames_out[b] = J, the true count,
 *    also where J > J_max. P is not renormalised: its modulus drifts by under 1e-13 over 4,000 frames,
 *    far below the f32 output.
 *
 * Layout. One launch, no workspace, no atomics: a wave owns one (row, bin) and walks the output in
 * blocks of 64 frames, a lane per frame (spec and recomb are bin-major with time contiguous, so reads
 * and writes are coalesced); the Kogge-Stone steps are shuffles, the carry is lane 63 of the block
 * before. Four waves, on neighbouring bins, per workgroup.
 */
#ifndef FS2HIP_PVOC_H
#define FS2HIP_PVOC_H

#include "fs2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS2_PVOC_BLOCK 64         /* output frames per block of the scan                                  */
#define FS2_PVOC_J_CAP 2147483647 /* the count of output frames saturates here                           */
#define FS2_PVOC_B_MAX 65535      /* rows per launch                                                     */

typedef struct fs2_pvoc_desc {
  const float *spec;          /* f32 [B, 2 NB, >= T_max], device; only columns below frames[b] are read  */
  int64_t spec_row_stride;    /* elements between bin rows, >= T_max (batch stride is 2 NB rows)         */
  const int64_t *frames;      /* int64 [B] frames per row, DEVICE memory; NULL = T_max each; values
                                 outside [0, T_max] are clamped                                          */
  const int64_t *frames_host; /* optional HOST copy of frames, used only to validate J_max               */
  const double *rates;        /* f64 [B], DEVICE memory                                                  */
  const double *rates_host;   /* optional HOST copy of rates, used only to validate J_max                */
  int B, NB, T_max, J_max;    /* host ints                                                               */
  float *recomb;              /* f32 [B, 2 NB, J_max], real rows then imaginary rows                     */
  int64_t recomb_row_stride;  /* elements between bin rows, >= J_max (batch stride is 2 NB rows)         */
  int64_t *frames_out;        /* optional int64 [B]: J                                                   */
} fs2_pvoc_desc;

/* J of rule 1 for a row of T frames; 0 for T < 1; a T above 2^31 - 1 counts as 2^31 - 1 */
int64_t fs2_pvoc_frames(int64_t T, double rate);

/*
 * FS2_EINVAL: a NULL descriptor / spec / rates / recomb, B / NB / T_max / J_max < 1, a row stride smaller
 * than its row, or J_max smaller than a count the host can see (rates_host[b] with frames_host[b], or
 * with T_max when frames is NULL). FS2_EUNSUPPORTED: B > FS2_PVOC_B_MAX. Nothing is launched then.
 */
int fs2_phase_vocoder(const fs2_pvoc_desc *d, fs2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FS2HIP_PVOC_H */
