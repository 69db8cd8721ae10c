/*
 * fs2hip_audio_inv.h — the other half of the reference's audio/ package: STFT.transform with its
 * full spectrum, STFT.inverse (audio/stft.py:52-127) and the two launches of a Griffin-Lim
 * iteration (audio/audio_processing.py:66-82), over ragged batches.
 *
 * Per utterance b with T = frames[b] frames (restates audio/stft.py:83-122):
 *   recomb    [2*513, T]                        real rows, then imaginary rows
 *   y_t[n]    = sum_c recomb[c, t] * inverse_basis[c, n]            n < 1024
 *   ola[p]    = sum over t with 256 t <= p < 256 t + 1024 of y_t[p - 256 t]    p < 1024 + 256 (T - 1)
 *   wsum[p]   = the reference's window_sumsquare: f32 accumulator, frames added in ascending order
 *   wav[s]    = ola[s + 512] / wsum[s + 512] * 4                    s < 256 (T - 1)
 * lens_out[b] = 256 * max(T - 1, 0); samples at or past it, up to n_out_max, are written 0.
 *
 * The projection of a Griffin-Lim step takes a spectrum z = (re, im) and a target magnitude m per
 * (bin, frame) and writes recomb = m * (re, im) / |z|, and (m, 0) where re = im = 0: what the
 * reference's cos(atan2(im, re)), sin(atan2(im, re)) give, without atan2 / cos / sin. (re, im) are
 * divided by max(|re|, |im|) before they are squared, so no magnitude underflows into the zero
 * branch.
 *
 * All products are exact-f32 MFMA / fmaf chains (v_mfma_f32_32x32x2_f32). The summation order of
 * every output depends only on the utterance's own data and the output's index: not on B, on the
 * batch slot, on n_max / T_in / T_out / n_out_max or on a stride.
 */
#ifndef FS2HIP_AUDIO_INV_H
#define FS2HIP_AUDIO_INV_H

#include "fs2hip_audio.h"

#ifdef __cplusplus
extern "C" {
#endif

/* inverse basis as fs2_istft reads it: K = 1026 channels padded to 1032 (129 groups of 8) */
#define FS2_ISTFT_KPAD 1032
#define FS2_ISTFT_PACKED_ELEMS (4 * FS2_ISTFT_KPAD * 256) /* floats */
#define FS2_ISTFT_WSUM_ELEMS (16 * 256)                   /* floats */

typedef struct fs2_stft_desc {
  const float *wav;         /* f32 [B, n_max] samples, device; NOT clipped unless clip != 0          */
  int64_t wav_row_stride;   /* elements between utterances, >= n_max                                 */
  const int64_t *lens;      /* int64 [B] samples per utterance, DEVICE memory; NULL = n_max each     */
  const int64_t *lens_host; /* optional HOST copy of lens, used only to validate T_out               */
  int B, n_max, T_out;      /* host ints                                                             */
  int n_fft, hop, win;      /* 1024, 256, 1024 (FS2_EUNSUPPORTED otherwise)                          */
  int clip;                 /* != 0: clip samples to [-1, 1] on load, as get_mel_from_wav does       */
  const float *basis;       /* f32 [2*513, 1024]: windowed Fourier basis, re rows then im rows       */
  const float *mag_target;  /* optional f32 [B, 513, >= T_out]: target magnitudes of the projection;
                               only columns below the utterance's frame count are read               */
  int64_t mag_row_stride;   /* elements between bin rows of mag_target, >= T_out (batch stride is
                               513 rows)                                                             */
  float *spec;              /* optional f32 [B, 1026, T_out], re rows then im rows                   */
  float *mag;               /* optional f32 [B, 513, T_out]                                          */
  float *recomb;            /* f32 [B, 1026, T_out]; given exactly when mag_target is                */
  int64_t *frames_out;      /* optional int64 [B]: 1 + lens/hop, or 0 (lens <= n_fft/2)              */
} fs2_stft_desc;

/*
 * One launch: frame t of utterance b is padded[t*hop : t*hop + n_fft] of the signal reflect-padded
 * by n_fft/2 at the utterance's own ends; frames[b] = 1 + lens[b] / hop, or 0 when lens[b] <=
 * n_fft/2. Outputs are bin-major, as the reference's conv1d gives them; columns at or past
 * frames[b], up to T_out, are written 0.
 * FS2_EINVAL: a NULL descriptor / wav / basis, no output at all, mag_target without recomb or
 * recomb without mag_target, B / n_max / T_out < 1, wav_row_stride < n_max, mag_row_stride < T_out
 * (with mag_target), or T_out smaller than a frame count the host can see (lens_host[b], or n_max
 * when lens is NULL). FS2_EUNSUPPORTED: any shape other than n_fft = win = 1024, hop = 256.
 */
int fs2_stft(const fs2_stft_desc *d, fs2_stream_t stream);

typedef struct fs2_istft_desc {
  const float *recomb;       /* f32 [B, 1026, >= T_in], device; only columns below frames[b] are read */
  int64_t recomb_row_stride; /* elements between channel rows, >= T_in (batch stride is 1026 rows)    */
  const int64_t *frames;     /* int64 [B] frames per utterance, DEVICE memory; NULL = T_in each;
                                values outside [0, T_in] are clamped                                  */
  const int64_t *frames_host; /* optional HOST copy of frames, used only to validate n_out_max        */
  int B, T_in, n_out_max;    /* host ints                                                             */
  int n_fft, hop, win;       /* 1024, 256, 1024 (FS2_EUNSUPPORTED otherwise)                          */
  const float *inv_packed;   /* f32 [FS2_ISTFT_PACKED_ELEMS]: the inverse basis [1026, 1024] (pinv of
                                the scaled Fourier basis, cast to f32, times the f32 window) repacked:
                                element (((g*4 + q)*256 + r)*2 + h)*4 + e holds
                                inverse_basis[8g + 2e + h, 256q + r], 0 for channels >= 1026          */
  const float *wsum_table;   /* f32 [16, 256]: window sum of phase r when the frames q = 0..3 hop
                                blocks back that exist are the set bits of the row index (bit q),
                                accumulated as the reference does (f32 accumulator, ascending frame)  */
  float *wav;                /* f32 [B, n_out_max]                                                    */
  int64_t wav_row_stride;    /* elements between utterances, >= n_out_max                             */
  int64_t *lens_out;         /* optional int64 [B]: 256 * max(frames - 1, 0)                          */
} fs2_istft_desc;

/*
 * One launch, a gather with no atomics: for hop block j and phase r,
 *   ola[256 j + r] = sum_{g} sum_{q=0..3} sum_{c in group g} recomb[c, j - q] * inverse_basis[c, 256 q + r].
 * FS2_EINVAL: a NULL required pointer, B / T_in / n_out_max < 1, a stride smaller than its row, or
 * n_out_max smaller than 256 * (frames - 1) for a frame count the host can see (frames_host[b], or
 * T_in when frames is NULL). FS2_EUNSUPPORTED: any shape other than n_fft = win = 1024, hop = 256.
 */
int fs2_istft(const fs2_istft_desc *d, fs2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FS2HIP_AUDIO_INV_H */
