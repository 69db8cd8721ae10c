/*
 * fs2hip_audio.h — training-target extraction: waveform -> log-mel spectrogram and frame energy
 * (the reference's audio/stft.py:130-178 TacotronSTFT.mel_spectrogram behind audio/tools.py:8-15
 * get_mel_from_wav), and the phoneme-level mean of preprocessor/preprocessor.py:293-302.
 *
 * Per utterance b with n = lens[b] samples (the reference runs one utterance at a time):
 *   x        = clip(wav[b, :n], -1, 1)            (int16 PCM: wav * (1 / max_wav_value) first)
 *   padded   = reflect-pad x by n_fft/2 on both sides, AT THE UTTERANCE'S OWN ENDS (sample 0 and
 *              sample n-1), never at n_max; done by index arithmetic, no padded copy exists
 *   frame t  = padded[t*hop : t*hop + n_fft],  t < frames[b] = 1 + n / hop   (integer division)
 *   re | im  = basis[0:n_bins] . frame | basis[n_bins:2*n_bins] . frame,  n_bins = n_fft/2 + 1
 *   mag      = sqrt(re^2 + im^2)
 *   mel      = log(max(mel_basis . mag, clip_val))
 *   energy   = sqrt(sum_bins mag^2)
 * All products are exact-f32 MFMA / fmaf chains (v_mfma_f32_32x32x2_f32); no operand is rounded
 * below f32. The summation order of every output depends only on the utterance's own samples and
 * the frame index: not on B, on the utterance's place in the batch, on n_max or on the row stride,
 * so an utterance gives the same bits alone and in any batch.
 *
 * Rows t >= frames[b] of mel / energy / mag (up to T_out) are written as 0.
 *
 * Short utterances: lens[b] <= n_fft/2 cannot be reflect-padded (the reference raises). Here such
 * an utterance — lens[b] <= 0 included — has 0 frames: all its rows are 0 and frames_out[b] = 0.
 * lens[b] > n_max is read as n_max (no sample past the row is ever touched).
 */
#ifndef FS2HIP_AUDIO_H
#define FS2HIP_AUDIO_H

#include "fs2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one more element type beside the fs2hip.h dtype codes, for waveform input only */
#define FS2_I16 3 /* int16 PCM */

typedef struct fs2_mel_desc {
  const void *wav;          /* [B, n_max] samples, FS2_F32 or FS2_I16, device                       */
  int wav_dtype;            /* FS2_F32: clipped to [-1, 1] on load; FS2_I16: * (1/max_wav_value)     */
  float max_wav_value;      /* FS2_I16 only (32768 for 16-bit PCM)                                   */
  int64_t wav_row_stride;   /* elements between utterances, >= n_max                                 */
  const int64_t *lens;      /* int64 [B] samples per utterance, DEVICE memory; NULL = n_max each     */
  const int64_t *lens_host; /* optional HOST copy of lens, used only to validate T_out; NULL = the
                               host cannot see the lengths (then T_out is the caller's promise:
                               frames past T_out are dropped)                                         */
  int B, n_max, T_out;      /* host ints: a captured graph serves every wav / lens of these sizes    */
  int n_fft, hop, win, n_mel; /* 1024, 256, 1024, 80 (FS2_EUNSUPPORTED otherwise)                    */
  const float *basis;       /* f32 [2*(n_fft/2+1), n_fft]: windowed Fourier basis, re rows then im   */
  const float *mel_basis;   /* f32 [n_mel, n_fft/2+1]                                                */
  float clip_val;           /* 1e-5: floor of the linear mel before the log (> 0)                    */
  float *mel;               /* f32 [B, T_out, n_mel], channels-last                                  */
  float *energy;            /* f32 [B, T_out]                                                        */
  float *mag;               /* optional f32 [B, T_out, n_fft/2+1]; NULL = not written                */
  int64_t *frames_out;      /* optional int64 [B]: 1 + lens/hop, or 0 (short utterance)              */
} fs2_mel_desc;

/*
 * One launch. FS2_EINVAL: a NULL required pointer, B / n_max / T_out < 1, wav_row_stride < n_max,
 * clip_val <= 0, an unknown wav_dtype, or T_out smaller than a frame count the host can see
 * (lens_host[b], or n_max when lens is NULL). FS2_EUNSUPPORTED: any shape other than n_fft = win =
 * 1024, hop = 256, n_mel = 80 (the fields are there so that wider shapes can be added).
 * A linear mel at or below clip_val gives exactly (float)log((double)clip_val).
 */
int fs2_mel_spectrogram(const fs2_mel_desc *d, fs2_stream_t stream);

/*
 * Phoneme-level mean of a frame-level track: out[b, i] = mean(values[b, s_i : s_i + d_i]) with
 * s_i = sum(d[b, :i]) (negative d counts as 0), and 0 where d_i = 0 or the segment starts at or
 * past T (a segment that crosses T averages the frames it has, as a numpy slice does). Each
 * segment is summed left to right in f32 and divided once. values f32 [B, T], dur int64 [B, L],
 * out f32 [B, L], all contiguous, device.
 *
 * The reference's loop (preprocessor.py:293-302) writes the means into the array it reads from.
 * It equals this plain mean exactly when sum(d[:i]) >= i for every i (every read then lies at or
 * past every earlier write); durations of real alignments satisfy it unless they start with
 * zero-length phonemes.
 */
int fs2_segment_mean(const float *values, const int64_t *dur, int B, int T, int L, float *out, fs2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FS2HIP_AUDIO_H */
