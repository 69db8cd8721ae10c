/*
 * fs2hip_iir.h — recursive (IIR) filtering of ragged batches and, on top of it, the integrated
 * loudness of ITU-R BS.1770-4 / EBU R128 and a loudness gain. It is BS.1770's rule, stated here as this
 * project's own arithmetic in float64: NOT the bits of scipy.signal.sosfilt, pyloudnorm or ffmpeg.
 * Only * + - / and sqrt in float64 are used, each correctly rounded and none contracted into an FMA,
 * and every order is fixed, so each output is determined bit for bit. No output depends on B, on the
 * row's place in the batch, on n_max, on a row stride or on the launch shape. The device takes no
 * logarithm. One channel per row.
 *
 * ---- fs2_sosfilt: cascaded second-order sections -----------------------------------------------------
 *
 * Per row b: samples x[0..n), n = clamp(lens[b], 0, n_max), int16, f32 or f64, each widened to double
 * exactly. sos f64 [S, 6] in scipy's layout (b0 b1 b2 a0 a1 a2) with a0 == 1 (a0 is not read). Section
 * s + 1 reads the whole output y of section s. One section, with state (z1, z2):
 *
 * 1. The recurrence R (scipy's transposed direct form II), per sample, in this order:
 *      y  = b0 * x + z1
 *      z1 = (b1 * x - a1 * y) + z2
 *      z2 = b2 * x - a2 * y
 *
 * 2. Blocks. The row is cut into blocks of FS2_IIR_BLOCK = 64 samples; block k holds samples
 *    [64 k, min(n, 64 k + 64)). R is run over block k from the state (0, 0): its outputs are y0, its end
 *    state is c_k (for a block shorter than 64 the state after its last sample; only the row's last
 *    block can be, and its c is then never used).
 *
 * 3. Tables (host, float64; fs2amd.ops.sos_tables; FS2_IIR_TABLE_LEN doubles per section). On a zero
 *    input R is  y = z1;  z1 = z2 - a1 * y;  z2 = -(a2 * y).  Run 64 steps of that
 *      from (1, 0): the outputs are p[0..64), the end state is (M11, M21)
 *      from (0, 1): the outputs are q[0..64), the end state is (M12, M22)
 *    M = [[M11, M12], [M21, M22]] carries a state across one full block. With the 2x2 product
 *      (A B)_rc = A_r1 * B_1c + A_r2 * B_2c          two products, one add
 *      P_0 = M, P_{j+1} = P_j P_j            for j = 0..4   (P_j = "M^(2^j)")
 *      Q_0 = I, Q_{i+1} = M Q_i              for i = 0..63  (Q_i = "M^i", i = 0..64)
 *    Layout of one section's table: p[64], q[64], P_0..P_5 (4 each, row-major), Q_0..Q_64 (4 each).
 *
 * 4. Incoming states. s_k is the state block k starts from: s_{k+1} = M s_k + c_k in exact arithmetic.
 *    With (A v) = (A11 * v1 + A12 * v2, A21 * v1 + A22 * v2), two products and one add per component:
 *    blocks are taken in groups of 64 (group g = blocks 64 g .. 64 g + 63, lane i = k - 64 g).
 *      v_i = c_k. For j = 0..5, d = 2^j, for all lanes i >= d at once:   v_i = (P_j v_{i-d}) + v_i
 *      (a Kogge-Stone scan; lanes past the row's last block never feed a lane below them).
 *      s_k = carry_g                       for i == 0
 *      s_k = (Q_i carry_g) + v_{i-1}       for i >= 1
 *      carry_{g+1} = (Q_64 carry_g) + v_63
 *    carry_0 = zi[b, s, :], or (+0.0, +0.0) where zi is NULL.
 *
 * 5. Output. For sample t of block k, i = t - 64 k:   y[t] = (y0[t] + p[i] * s_k.z1) + q[i] * s_k.z2
 *
 * 6. zf[b, s, :], the state after the last sample, is R's state update applied to the shipped samples:
 *      n == 0:  zf = carry_0
 *      z2f = b2 * x[n-1] - a2 * y[n-1]
 *      z1f = (b1 * x[n-1] - a1 * y[n-1]) + w,   w = b2 * x[n-2] - a2 * y[n-2]  (n >= 2),  carry_0.z2 (n == 1)
 *    with x the section's input and y its output of rule 5.
 *
 * y f64 [B, n_max] is the last section's output, y32 its rounding to f32; both are +0.0 from n on.
 * Against a direct recurrence in extended precision the error of rule 5 is a few 1e-13 of max |y| for
 * the K-weighting sections; a section with a near-double pole close to z = 1 makes Q_i ill-conditioned
 * and loses about three more digits (DESIGN 9.10 has the measurements).
 *
 * Layout. One launch, one workgroup of 256 threads per row, no workspace, no atomics, and no workgroup
 * waits for another. The row streams through LDS in chunks of FS2_IIR_CHUNK = 16384 samples (256
 * blocks, four groups), each block at a stride of 65 doubles so that the 64 lanes of a wave, one block
 * each, read different banks. Per chunk and section: a thread per block runs rule 2 in place, a wave
 * per group scans by shuffles, the group carries are chained through LDS, and rule 5 is one coalesced
 * pass; the carry of every section is kept in LDS from chunk to chunk. int16 and f32 samples of the next
 * chunk are loaded into registers before the work on the chunk at hand, which hides their latency.
 *
 * ---- fs2_loudness_gate: BS.1770-4 gating of one filtered channel --------------------------------------
 *
 * y f64 [B, n_max] contiguous, n as above. H = the hop in samples (Python: round(fs / 10)), T = 4 H.
 *   S_m  = the sum of the squares of samples [m H, (m + 1) H) in the order of include/fs2hip_vad.h: leaves
 *          of 8 neighbouring squares added ascending, then that header's pairwise tree T() over the
 *          leaves in order.
 *   J    = 0 for n < T, else (n - T) / H + 1                               (integer division)
 *   z_j  = ((S_j + S_{j+1}) + (S_{j+2} + S_{j+3})) / (double)T            for 0 <= j < J
 *   A    = { j : z_j > abs_gate }
 *   mean_A = T(z_j for j in A, +0.0 for the others; all J values in order) / (double)|A|
 *   R    = { j in A : z_j > rel_factor * mean_A }                          one f64 multiply
 *   zbar = T(z_j for j in R, +0.0 for the others; all J values in order) / (double)|R|
 * |A| == 0 gives |R| == 0; |R| == 0 gives zbar = +0.0 (a row that is too short, or silent).
 * counts int32 [B, 3] = (J, |A|, |R|). Python passes abs_gate = 10 ** ((-70 + 0.691) / 10) times the
 * square of the full scale (1 for float input, 32768 for int16-valued input) and rel_factor = 0.1, and
 * takes the logarithm itself: LUFS = -0.691 + 10 log10(zbar / full_scale ** 2).
 * Layout: two launches. One workgroup per (row, sub-block) sums S_m through LDS; one workgroup per row
 * does the rest, its trees level by level between two buffers of the workspace.
 *
 * ---- fs2_gain_int16: the gain -------------------------------------------------------------------------
 *
 * x int16 or f32 [B, n_max] (the UNFILTERED samples), n as above.
 *   zbar[b] > 0:  gain = sqrt(target_z / zbar[b])        one f64 divide, one f64 sqrt
 *                 with peak_ceiling > 0 and peak[b] > 0:  lim = peak_ceiling / peak[b];  gain = lim
 *                 where gain > lim (the gain is lowered, never raised)
 *   otherwise:    gain = 1.0 and unmeasured[b] = 1 (else 0); the ceiling is not applied.
 *   peak[b] = max |x| as f64 over the row: exact and order-free (per-thread maxima merged by an integer
 *   atomic max on the bits, as fs2_resample merges its peak), +0.0 for n == 0.
 *   int16: v = x * gain (one f64 multiply), rounded to the nearest integer, ties to even, SATURATED to
 *          [-32768, 32767]; clipped[b] counts the samples that saturation changed (order-free).
 *   f32:   q = (float)(x * gain), not saturated; clipped[b] = 0.
 * q has x's dtype and is 0 from n on. Two launches after a memset (one when peak is NULL).
 */
#ifndef FS2HIP_IIR_H
#define FS2HIP_IIR_H

#include "fs2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS2_IIR_BLOCK 64        /* samples per block                                                      */
#define FS2_IIR_CHUNK 16384     /* samples a workgroup holds in LDS at a time (256 blocks)                */
#define FS2_IIR_S_MAX 8         /* sections per launch                                                    */
#define FS2_IIR_TABLE_LEN 412   /* doubles per section of the host tables: 64 + 64 + 6 * 4 + 65 * 4       */
#define FS2_IIR_B_MAX 65535     /* rows per launch, all three entry points                                */
#define FS2_LOUD_H_MAX 32768    /* the hop of fs2_loudness_gate, at most (its leaves are summed in LDS)   */

/* blocks (ceil(n / 64)) and chunks (ceil(n / 16384)) of a row of n samples; 0 for n < 1 */
int64_t fs2_iir_blocks(int64_t n);
int64_t fs2_iir_chunks(int64_t n);

/* J of fs2_loudness_gate for a row of n samples: 0 for n < 4 H, else (n - 4 H) / H + 1; -1 for H < 1 */
int64_t fs2_loudness_blocks(int64_t n, int64_t H);

/* bytes of fs2_loudness_gate's workspace: 8 * B * ((J + 3) + J + (J + 1) / 2) with J =
 * fs2_loudness_blocks(n_max, H), 0 for J == 0 or a size below 1, INT64_MAX where it does not fit */
int64_t fs2_loudness_workspace_bytes(int64_t B, int64_t n_max, int64_t H);

/*
 * wav [B, n_max] of dtype FS2_I16, FS2_F32 or FS2_F64 with row_stride >= n_max elements between rows;
 * lens int64 [B] or NULL (= n_max each; values are clamped to [0, n_max]); sos f64 [S, 6]; tables f64
 * [S, FS2_IIR_TABLE_LEN] (rule 3); zi f64 [B, S, 2] or NULL. -> y f64 [B, n_max]; y32 f32 [B, n_max] or
 * NULL; zf f64 [B, S, 2] or NULL. All device memory. One launch.
 * FS2_EINVAL: wav, sos, tables or y NULL, B / n_max / S < 1, row_stride < n_max.
 * FS2_EUNSUPPORTED: another dtype, S > FS2_IIR_S_MAX, B > FS2_IIR_B_MAX. Nothing is launched then.
 */
int fs2_sosfilt(const void *wav, int dtype, int64_t row_stride, const int64_t *lens, int B, int n_max,
                const double *sos, const double *tables, int S, const double *zi, double *y, float *y32, double *zf,
                fs2_stream_t stream);

/*
 * y f64 [B, n_max] contiguous, lens as above -> zbar f64 [B], counts int32 [B, 3]. workspace of at least
 * fs2_loudness_workspace_bytes(B, n_max, H) bytes, 8-byte aligned (may be NULL when that is 0).
 * FS2_EINVAL: y, zbar or counts NULL, B / n_max / H < 1, workspace NULL or too small where one is needed,
 * an abs_gate or rel_factor that is negative or NaN. FS2_EUNSUPPORTED: H > FS2_LOUD_H_MAX,
 * B > FS2_IIR_B_MAX, a workspace beyond INT64_MAX bytes. Nothing is launched then.
 */
int fs2_loudness_gate(const double *y, const int64_t *lens, int B, int n_max, int H, double abs_gate,
                      double rel_factor, double *zbar, int32_t *counts, void *workspace, int64_t workspace_bytes,
                      fs2_stream_t stream);

/*
 * wav [B, n_max] of dtype FS2_I16 or FS2_F32, row_stride and lens as above; zbar f64 [B] -> q [B, n_max]
 * of wav's dtype (contiguous), gain f64 [B], clipped int32 [B], unmeasured int32 [B] or NULL, peak f64 [B]
 * or NULL (needed when peak_ceiling > 0).
 * FS2_EINVAL: wav, zbar, q, gain or clipped NULL, B / n_max < 1, row_stride < n_max, target_z that is not
 * a positive finite number, a NaN or negative peak_ceiling, peak NULL with peak_ceiling > 0.
 * FS2_EUNSUPPORTED: another dtype, B > FS2_IIR_B_MAX. Nothing is launched then.
 */
int fs2_gain_int16(const void *wav, int dtype, int64_t row_stride, const int64_t *lens, int B, int n_max,
                   const double *zbar, double target_z, double peak_ceiling, void *q, double *gain, int32_t *clipped,
                   int32_t *unmeasured, double *peak, fs2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FS2HIP_IIR_H */
