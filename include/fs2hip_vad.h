/*
 * fs2hip_vad.h — silence trimming and splitting of raw waveforms: the rule of librosa.effects.trim /
 * librosa.effects.split (frame power against the utterance's own maximum, top_db as the threshold),
 * stated here as this project's own arithmetic in float64. It is librosa's rule, NOT librosa's bits:
 * librosa frames a float32 signal, takes a float32 RMS and a base-10 logarithm; here the power is
 * float64 in a fixed order and the device takes no logarithm. With frame_length = win_length and
 * hop = hop_length the frames are the mel frames (1 + n / hop of them, centred).
 *
 * Frame power. Per row b: samples x[0..n), n = clamp(lens[b], 0, n_max), int16 or f32, each widened to
 * double exactly; each square x * x is then exact (at most 48 significant bits).
 *   F = 0 for n == 0, else 1 + n / hop                                      (integer division)
 *   frame f covers samples [a, a + frame_length), a = f * hop - frame_length / 2; samples outside
 *   [0, n) count as +0.0 (zero padding, not reflection).
 *   With g = gcd(frame_length, hop), the samples from -(frame_length / 2) on fall into blocks of g:
 *   block k covers [k * g - frame_length / 2, (k + 1) * g - frame_length / 2), and frame f is exactly the
 *   q = frame_length / g blocks from f * (hop / g) on. Two kinds of sum, each add one f64 operation:
 *     a leaf:  8 neighbouring squares (fewer at a block's end), ((s_0 + s_1) + s_2) + .., ASCENDING
 *     a tree T(v_0 .. v_{m-1}):  t_0 = v;  t_{l+1}[j] = t_l[2 j] + t_l[2 j + 1], a last element without a
 *              partner carried up unchanged; the one element left is the value
 *     S_k  = T(the leaves of block k, in order)         leaf j holds the block's samples 8 j .. 8 j + 7
 *     P[f] = T(S_{f h}, S_{f h + 1}, .., S_{f h + q - 1}) / frame_length          h = hop / g
 *   Nothing is contracted into an FMA. Adding a +0.0 changes no sum, so the value does not depend on
 *   how far past [0, n) a block reaches. This order makes overlapping frames cheap (each sample is
 *   squared once, each block summed once, where hop divides frame_length), it is fixed, so P is
 *   determined bit for bit, and it is a pairwise order: the error grows with log2(frame_length), a
 *   few ulp of P against the exact sum, where one long chain would lose sqrt(frame_length) of them.
 *   For int16 input and frame_length <= 2^23 every sum is exact besides.
 *   P[b, f] = +0.0 for F <= f < F_max, F_max = fs2_vad_frames(n_max, hop). Pmax[b] = max_f P[b, f]
 *   (order-free: P >= 0 and no NaN for finite input), +0.0 for F == 0.
 *   P does not depend on B, on the row's place in the batch, on n_max, on the row stride or on the launch.
 *
 * Activity. threshold and floor are f64 arguments (Python: threshold = 10 ** (-top_db / 10),
 * floor = (1e-5 * full_scale) ** 2: librosa's amin on amplitude; full_scale 1.0 for float input,
 * 32768 for int16-valued input).
 *   ref = max(Pmax[b], floor);  frame f < F is active iff max(P[f], floor) > threshold * ref
 *   (strict; threshold * ref is one f64 multiply). A row below the floor everywhere has no active frame
 *   for threshold >= 1 only; for threshold < 1 every frame of it is active, as in librosa.
 *
 * Short silences. min_silence >= 1. A maximal run of inactive frames that lies strictly between two
 * active frames and is shorter than min_silence counts as active. Runs at either end are never filled.
 * min_silence = 1 fills nothing (librosa's behaviour).
 *
 * Intervals. For every maximal active run [s, e) of frames after the fill, in increasing order:
 * [s * hop, min(n, e * hop)) in samples, int64. count[b] is the true number of runs; only the first
 * max_intervals are written and the rest of the table is zero.
 *
 * Trim. No active frame: (0, 0). Otherwise start = max(0, first_active * hop - margin),
 * end = min(n, (last_active + 1) * hop + margin), margin >= 0 in samples.
 *
 * Cut. out[b, 0 .. end - start) = x[b, start .. end) in the input's dtype, 0 from there to M_max;
 * out_lens[b] = end - start. start and end are clamped to 0 <= start <= end <= min(n_max, start + M_max).
 *
 * Layout. fs2_vad_power: one workgroup of 256 threads per tile of up to FS2_VAD_TILE_FRAMES frames of
 * a row. It stages the tile's samples in LDS one pass of whole blocks at a time (coalesced reads; each
 * block padded to an odd bank stride), one thread sums each block, the block sums stay in LDS, one
 * thread per frame adds its q of them. A sample is read from memory once per tile that covers it, not
 * frame_length / hop times. The tile maxima go to the workspace and a second, tiny launch reduces
 * them to Pmax (no atomics, no memset).
 * fs2_vad_intervals: one workgroup per row walks the frames in chunks of chunk_frames; run edges by
 * ballot and prefix sum, the last active frame and the run count carried from chunk to chunk. The
 * result does not depend on chunk_frames.
 */
#ifndef FS2HIP_VAD_H
#define FS2HIP_VAD_H

#include "fs2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS2_VAD_SUMS_BYTES 32768   /* LDS of a fs2_vad_power workgroup for its block sums (4096 f64)         */
#define FS2_VAD_AREA_BYTES 32768   /* ... and for one pass of samples                                        */
#define FS2_VAD_TILE_FRAMES 192    /* frames per workgroup of fs2_vad_power, at most                         */
#define FS2_VAD_CHUNK_FRAMES 256   /* frames per step of fs2_vad_intervals' walk (the default)               */
#define FS2_VAD_B_MAX 65535        /* rows per launch                                                        */

/* 0 for n < 1, else 1 + n / hop; -1 for hop < 1 */
int64_t fs2_vad_frames(int64_t n, int64_t hop);

/* bytes of fs2_vad_power's workspace: 8 * B * ceil(F_max / G) with G = min(FS2_VAD_TILE_FRAMES,
 * (4096 - frame_length / g) / (hop / g) + 1) frames per tile; 0 for a size below 1, hop > frame_length
 * or a geometry that is refused; INT64_MAX where it does not fit */
int64_t fs2_vad_workspace_bytes(int64_t B, int64_t F_max, int64_t frame_length, int64_t hop);

/* the least LDS a launch with this geometry needs: 8 * (frame_length / g) for one frame's block sums
 * and 4 * (g | 1) for one block of samples; 0 for a size below 1 or hop > frame_length. A launch is
 * refused when the first part exceeds FS2_VAD_SUMS_BYTES or the second FS2_VAD_AREA_BYTES: g may not
 * exceed 8191 and frame_length / g may not exceed 4096. */
int64_t fs2_vad_lds_bytes(int64_t frame_length, int64_t hop);

/*
 * wav [B, n_max] of dtype FS2_I16 or FS2_F32 with row_stride >= n_max elements between rows; lens int64
 * [B] or NULL (= n_max each; values are clamped to [0, n_max]). P f64 [B, F_max], Pmax f64 [B],
 * workspace of at least fs2_vad_workspace_bytes(B, F_max, frame_length, hop) bytes, 8-byte aligned.
 * All device memory. Two launches. FS2_EINVAL: wav, P, Pmax or workspace NULL, B / n_max / frame_length / hop < 1,
 * hop > frame_length, row_stride < n_max, workspace_bytes too small. FS2_EUNSUPPORTED: another dtype,
 * B > FS2_VAD_B_MAX, a geometry beyond the two LDS limits above, F_max > INT32_MAX or
 * 8 * B * F_max > INT32_MAX. Nothing is launched then.
 */
int fs2_vad_power(const void *wav, int dtype, int64_t row_stride, const int64_t *lens, int B, int n_max,
                  int frame_length, int hop, double *P, double *Pmax, void *workspace, int64_t workspace_bytes,
                  fs2_stream_t stream);

/*
 * P f64 [B, F_max], Pmax f64 [B], lens int64 [B] or NULL (= n_max each), n_max and hop as given to
 * fs2_vad_power (F_max = fs2_vad_frames(n_max, hop)) -> active uint8 [B, F_max] (after the fill, 0 from
 * F on), count int32 [B], intervals int64 [B, max_intervals, 2], trim int64 [B, 2]. chunk_frames: 0
 * (= FS2_VAD_CHUNK_FRAMES), 64, 128 or 256. One launch.
 * FS2_EINVAL: a NULL pointer (intervals may be NULL when max_intervals == 0), B / n_max / hop /
 * min_silence < 1, margin or max_intervals < 0, another chunk_frames, a threshold or floor that is
 * negative or NaN. FS2_EUNSUPPORTED: B > FS2_VAD_B_MAX, F_max > INT32_MAX, 8 * B * F_max or
 * 16 * B * max_intervals > INT32_MAX.
 */
int fs2_vad_intervals(const double *P, const double *Pmax, const int64_t *lens, int B, int n_max, int hop,
                      double threshold, double floor, int min_silence, int64_t margin, int max_intervals,
                      int chunk_frames, uint8_t *active, int32_t *count, int64_t *intervals, int64_t *trim,
                      fs2_stream_t stream);

/*
 * The ragged gather: out [B, M_max] of wav's dtype, out[b, m] = wav[b, start + m] for m < end - start,
 * 0 beyond; (start, end) = trim[b] clamped as stated above; out_lens int64 [B] or NULL. One launch.
 * FS2_EINVAL: wav, trim or out NULL, B / n_max / M_max < 1, row_stride < n_max. FS2_EUNSUPPORTED:
 * another dtype, B > FS2_VAD_B_MAX.
 */
int fs2_vad_cut(const void *wav, int dtype, int64_t row_stride, const int64_t *trim, int B, int n_max, int M_max,
                void *out, int64_t *out_lens, fs2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FS2HIP_VAD_H */
