/*
 * fs2hip_align.h — durations without a forced aligner: the two dynamic programmes of the
 * alignment-learning framework (Badlani et al. 2021, "One TTS Alignment To Rule Them All") over a
 * ragged batch of attention log-probabilities. Nothing of this exists in the reference, which takes
 * its durations from MFA; the definitions below are the whole specification.
 *
 * Input, both programmes: logp [B, T_max, L_max], FS2_F32 or FS2_F64, unit stride along L, any row
 * stride >= L_max and batch stride >= T_max rows. Utterance b has T_b = clamp(mel_lens[b], 0, T_max)
 * frames and L_b = clamp(text_lens[b], 0, L_max) phonemes (NULL: the maximum each). float32 input is
 * widened on load (exact); every operation below is one IEEE float64 operation, none contracted.
 * Nothing outside [T_b, L_b] is read. An utterance with T_b = 0, L_b = 0 or T_b < L_b is skipped.
 *
 * fs2_mas — monotonic alignment search (a Viterbi pass), x = logp[b]:
 *   v[0,0] = x[0,0], v[0,j] = -inf for j > 0
 *   t >= 1: d[t,j] = j >= 1 && v[t-1,j-1] >= v[t-1,j]          (a tie takes the diagonal)
 *           v[t,j] = x[t,j] + (d[t,j] ? v[t-1,j-1] : v[t-1,j])
 *   backtrack: j = L_b - 1; for t = T_b - 1 .. 0: frame t belongs to phoneme j; if t >= 1, j -= d[t,j]
 *   durations[b,j] = frames of phoneme j (0 for j >= L_b), score[b] = v[T_b-1, L_b-1],
 *   path[b,t] = the phoneme of frame t (-1 for t >= T_b). A skipped utterance: zeros, -inf, -1.
 *   One add and one comparison per cell, no reduction: durations, path and score are determined
 *   bit for bit. For finite input (and for -inf entries) every durations[b, j < L_b] >= 1 and the row
 *   sums to T_b: cell (t, t) can only be reached along the diagonal, which the tie rule takes.
 *   The v matrix is never stored: its previous row lives in LDS (two rows, ping-pong), the
 *   decisions as one BIT per cell, T_max rows of ceil(L_max / 64) 64-bit words, in LDS when
 *   fs2_mas_lds_bytes(T_max, L_max, 1) <= FS2_MAS_LDS_BYTES and in the caller's workspace
 *   (fs2_mas_ws_bytes) otherwise, or when asked for. Same bits out either way.
 *
 * fs2_forward_sum — the alignment loss, with z[t,0] = blank_logprob, z[t,j] = x[t,j-1] (j = 1..L_b):
 *   m_t = max_c z[t,c], lp[t,c] = (z[t,c] - m_t) - log(sum_c exp(z[t,c] - m_t))      (log-softmax)
 *   states s = 0 .. 2 L_b: class(s) = 0 (blank) for even s, (s + 1) / 2 for odd s
 *   alpha[0,0] = lp[0,0], alpha[0,1] = lp[0,1], alpha[0,s] = -inf otherwise
 *   t >= 1: a1 = alpha[t-1,s], a2 = alpha[t-1,s-1], a3 = alpha[t-1,s-2] for odd s >= 3, else -inf
 *           (missing states: -inf); m = max(a1, a2, a3), m = 0 if that is -inf;
 *           alpha[t,s] = ((log((exp(a1 - m) + exp(a2 - m)) + exp(a3 - m))) + m) + lp[t,class(s)]
 *   l1 = alpha[T_b-1, 2 L_b], l2 = alpha[T_b-1, 2 L_b - 1], m as above:
 *   nll[b] = -(log(exp(l1 - m) + exp(l2 - m)) + m); +inf for a skipped utterance.
 *   loss = (sum over b in index order of nll[b] / L_b, finite nll only) / B: torch's
 *   ctc_loss(..., zero_infinity=True) per utterance, in its CPU kernel's operation order.
 *   alpha f64 [B, T_max, 2 L_max + 1] is written inside [T_b, 2 L_b + 1] only.
 *
 * fs2_forward_sum_bwd — d loss / d logp, in logp's dtype, contiguous [B, T_max, L_max]:
 *   beta[T_b-1,s] = lp[T_b-1,class(s)] for s >= 2 L_b - 1, else -inf
 *   t < T_b-1: b1 = beta[t+1,s], b2 = beta[t+1,s+1], b3 = beta[t+1,s+2] for odd s with s + 2 < 2 L_b + 1;
 *           beta[t,s] = ((log((exp(b1 - m) + exp(b2 - m)) + exp(b3 - m))) + m) + lp[t,class(s)]
 *   grad[b,t,j] = (exp(lp[t,j+1]) - exp(((alpha[t,2j+1] + beta[t,2j+1]) + nll[b]) - lp[t,j+1]))
 *                 * (grad_out / (L_b * B))
 *   and exact zeros for t >= T_b, for j >= L_b and for an utterance whose nll is not finite.
 *   exp / log are the device library's (within 1 ulp); these two results are bounded, not exact.
 */
#ifndef FS2HIP_ALIGN_H
#define FS2HIP_ALIGN_H

#include "fs2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS2_MAS_LDS_BYTES 163840       /* the LDS of one workgroup: two v rows of (L_max + 1) f64, then
                                          (bitmap in LDS) T_max * ceil(L_max / 64) 64-bit words     */
#define FS2_MAS_LDS_SMALL 32768        /* launches that need no more than this use the small form:
                                          more than one workgroup per compute unit                */
#define FS2_FORWARD_SUM_LDS_BYTES 65536 /* two state rows of (2 L_max + 5) f64, then 2 T_max f64  */
#define FS2_MAS_AUTO 0
#define FS2_MAS_LDS 1
#define FS2_MAS_GLOBAL 2

/* bytes of LDS fs2_mas needs with the bitmap in LDS (in_lds != 0) or in the workspace; 0 for a
 * size < 1, INT64_MAX for a size beyond 2^24 */
int64_t fs2_mas_lds_bytes(int T_max, int L_max, int in_lds);
/* bytes of the workspace of the global form: B * T_max * ceil(L_max / 64) * 8 (0 for a size < 1) */
int64_t fs2_mas_ws_bytes(int B, int T_max, int L_max);
/* bytes of LDS fs2_forward_sum and fs2_forward_sum_bwd need */
int64_t fs2_forward_sum_lds_bytes(int T_max, int L_max);

/*
 * bitmap: FS2_MAS_AUTO (LDS where it fits), FS2_MAS_LDS, FS2_MAS_GLOBAL. ws: device memory of at least
 * fs2_mas_ws_bytes (global form; may be NULL otherwise). durations int64 [B, L_max], score f64 [B],
 * path int32 [B, T_max] or NULL. FS2_EINVAL: a NULL logp / durations / score, B / T_max / L_max < 1,
 * strides too small, an unknown bitmap, a workspace too small. FS2_EUNSUPPORTED: another dtype,
 * FS2_MAS_LDS beyond FS2_MAS_LDS_BYTES, rows that do not fit the LDS at all.
 */
int fs2_mas(const void *logp, int dtype, int64_t batch_stride, int64_t row_stride, const int64_t *mel_lens,
            const int64_t *text_lens, int B, int T_max, int L_max, int bitmap, void *ws, int64_t ws_bytes,
            int64_t *durations, double *score, int32_t *path, fs2_stream_t stream);

/* alpha f64 [B, T_max, 2 L_max + 1], nll f64 [B], loss f64 [1]. Two launches (the DP, then the sum). */
int fs2_forward_sum(const void *logp, int dtype, int64_t batch_stride, int64_t row_stride, const int64_t *mel_lens,
                    const int64_t *text_lens, int B, int T_max, int L_max, double blank_logprob, double *alpha,
                    double *nll, double *loss, fs2_stream_t stream);

/* alpha, nll as fs2_forward_sum wrote them for the same arguments; grad_out: a device f64 scalar;
 * grad [B, T_max, L_max] contiguous, of logp's dtype. One launch. */
int fs2_forward_sum_bwd(const void *logp, int dtype, int64_t batch_stride, int64_t row_stride,
                        const int64_t *mel_lens, const int64_t *text_lens, int B, int T_max, int L_max,
                        double blank_logprob, const double *alpha, const double *nll, const double *grad_out,
                        void *grad, fs2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FS2HIP_ALIGN_H */
