/*
 * fs2hip_f0_track.h — an F0 path through the whole utterance, chosen over the normalised difference
 * table that fs2_f0_yin writes (include/fs2hip_f0.h, its cmnd output): probabilistic YIN in the
 * manner of Mauch & Dixon (2014). Every trough of a frame's dp row is a candidate, a prior over
 * thresholds weights the candidates, and a hidden Markov model over pitch bin and voicing picks one
 * path by Viterbi. This is pYIN-style tracking over this project's own table; its values are neither
 * librosa.pyin's nor WORLD's. The definitions below are the whole specification.
 *
 * Design rule: the device only compares, adds and looks up. Every logarithm, power and division of
 * the model is taken on the host, into small float64 tables passed to the launch (Python builds
 * them from exact rationals and correctly rounded logarithms). The one exception is the refinement
 * of a candidate, which is the uncontracted parabola of fs2hip_f0.h. Given the dp table, everything
 * below is therefore determined bit for bit in any evaluation order, and the dp table itself is for
 * int16 input under that header's condition W * tau_max < 2^21.
 *
 * Utterance b has F_b = min(max(lens[b], 0) / hop + 1, F_max) frames (lens in samples, as fs2_f0_yin
 * takes them; NULL: F_max frames each). Nothing of a row k >= F_b is read.
 *
 * Candidates of frame k, from its row dp(0 .. tau_max), in lag order:
 *   every t in [tau_min, tau_max - 1] with dp(t) < dp(t - 1) && dp(t) <= dp(t + 1)   (a NaN: false)
 *   a = dp(t - 1), b = dp(t), c = dp(t + 1);  den = (a - 2 * b) + c
 *   delta = den > 0 ? (0.5 * (a - c)) / den : 0;  p = (double)t + delta;  f = sr / p
 *   kept when f0_floor <= f && f <= f0_ceil.
 *
 * Threshold prior. thr[0 .. 100], thr[i] the double nearest i / 100 (thr[0] is not a threshold).
 *   a(c) = the smallest i in 1 .. 100 with dp_c < thr[i], 101 when there is none.
 *   The weights w_i, i = 1 .. 100, are Beta(2, 18) at i / 100, w_i ~ s (1 - s)^17, normalised to sum
 *   1; C_j = w_1 + .. + w_j, C_0 = 0, C_100 = 1, kept exact on the host. For threshold i the chosen
 *   candidate is the first in lag order with dp < thr[i]. With m(c) = min(101, a(c') for kept c'
 *   before c), candidate c is chosen for i in [a(c), m(c) - 1]: mass C_{m(c)-1} - C_{a(c)-1} when
 *   a(c) < m(c), none otherwise. The thresholds below every a, i < a_min, give p_a = 1 / 100 of their
 *   mass C_{a_min - 1} to the candidate with the smallest dp (ties: the smaller lag), "the best".
 *   With u = a(c) - 1 and v = m(c) - 1, both in 0 .. 100 (v >= u for the best), the log-mass is
 *     lm0[u * 101 + v] = max(log(C_v - C_u), log_floor)            v > u, else -inf    (not the best)
 *     lm1[u * 101 + v] = max(log((C_v - C_u) + p_a C_u), log_floor)  mass > 0, else -inf   (the best)
 *   A candidate whose log-mass is -inf is dropped. The frame's unvoiced log-probability is
 *     lu[g] = log(max((1 - p_a) C_g / N, p_floor)),  g = a_min - 1;   lu[101] = log(1 / N): no kept candidate.
 *   log_floor = log(p_floor), p_floor = 1e-12.
 *
 * Pitch bins. R bins per semitone upward from f0_floor, N the smallest count whose top edge reaches
 *   f0_ceil (R = 5, 71 .. 800 Hz: 210). edges[0 .. N], edges[n] = the double nearest
 *   sr / (f0_floor * 2^(n / (12 R))): periods in samples, decreasing.
 *   bin(p) = the number of n in 1 .. N - 1 with p <= edges[n].
 *   Of two candidates in one bin the one with the larger log-mass stays; ties: the smaller lag.
 *   At most FS2_F0_TRACK_CAP_MAX = 101 candidates of a frame survive (a strictly falls along the
 *   ones with mass, plus the best), and never more than there can be troughs:
 *   cap = min((tau_max - tau_min + 1) / 2, 101).
 *
 * States. 2 N: s = n is "bin n, voiced", s = N + n "bin n, unvoiced".
 *   obs_k(n) = the log-mass of the frame's candidate in bin n, log_floor where it has none
 *   obs_k(N + n) = lu[g_k]
 *   trans(s', s) for |n - n'| <= K: trans_same[|n - n'|] when the voicing stays, trans_switch[|n - n'|]
 *   when it changes: log(tri(d) * (1 - switch_prob)) and log(tri(d) * switch_prob) with
 *   tri(d) = (K + 1 - d) / (K + 1)^2, one table entry each (not renormalised at the edges).
 *
 * Viterbi.
 *   delta_0(s) = obs_0(s) + log_init,  log_init = log(1 / (2 N))
 *   delta_k(s) = obs_k(s) + max over predecessors s' of (delta_{k-1}(s') + trans(s', s))
 *   Each + is one float64 add. The max is taken by > over the predecessors in this order, so the
 *   first of equals wins: bins n' = n - K .. n + K ascending (inside 0 .. N - 1), and for each bin
 *   the state of the same voicing before the one of the other.
 *   The final state is the largest delta_{F_b - 1}, the lowest s among equals; the path follows the
 *   stored predecessors back to frame 0.
 *
 * Output per frame k < F_b on the path's state s: a voiced state (s < N) whose bin holds a candidate
 * of frame k gives f0 = that candidate's f and state = s; an unvoiced state, and a voiced state
 * without a candidate in the frame (the path may bridge a frame that way), give f0 = 0 and
 * state = -1. Frames k >= F_b: 0 and -1. score[b] = the final state's delta.
 *
 * Layout: two launches on one stream. The observation stage runs one wave per (utterance, frame): it
 * scans the row with ballots, runs the running minimum of a as a wave scan and writes the frame's
 * sparse candidate list (bin, log-mass, f) and lu index to the workspace. The recursion runs one
 * workgroup of 256 threads per utterance, lane n holding bin n in both voicings, delta
 * double-buffered in LDS, one barrier per frame, one byte of predecessor per state and frame in
 * the workspace; the back-trace stages FS2_F0_TRACK_TB frames of those bytes in LDS at a time and
 * is walked by one lane. No atomics: an utterance's result does not depend on B, on its place in
 * the batch, on F_max or on what the rows past F_b hold.
 */
#ifndef FS2HIP_F0_TRACK_H
#define FS2HIP_F0_TRACK_H

#include "fs2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS2_F0_TRACK_THR 100       /* thresholds; thr, lu, lm0 and lm1 are sized by it             */
#define FS2_F0_TRACK_CAP_MAX 101   /* candidates of one frame that can survive                     */
#define FS2_F0_TRACK_BINS_MAX 256  /* N: one lane of the recursion's workgroup per bin             */
#define FS2_F0_TRACK_STEP_MAX 63   /* K: (2 K + 1) * 2 predecessors fit one byte                   */
#define FS2_F0_TRACK_TB 64         /* frames of predecessor bytes staged in LDS by the back-trace  */
#define FS2_F0_TRACK_LDS_BYTES 65536 /* the recursion's LDS: 8 * (4 * (N + 2 K) + 2 * N) + TB * 2 N + 8 */

/* bytes of LDS of the recursion (0 for a size < 1; INT64_MAX beyond 2^24) */
int64_t fs2_f0_track_lds_bytes(int n_bins, int max_step);

/*
 * bytes of workspace of one call (0 for a size < 1; INT64_MAX where it does not fit 63 bits), with
 * cap as above and every part rounded up to 8 bytes:
 *   8 * B * F_max (lu index and count) + 20 * B * F_max * cap (log-mass, f, bin) + B * F_max * 2 * N
 */
int64_t fs2_f0_track_workspace_bytes(int B, int F_max, int tau_min, int tau_max, int n_bins);

/*
 * cmnd f64 [B, F_max, tau_max + 1] contiguous, as fs2_f0_yin writes it; lens int64 [B] in samples or
 * NULL. Tables, all f64 device memory: thr [101], lm0 and lm1 [101 * 101], lu [102], edges
 * [n_bins + 1], trans_same and trans_switch [max_step + 1]. workspace: ws_bytes >=
 * fs2_f0_track_workspace_bytes, 8-byte aligned. f0 f64 [B, F_max], state int32 [B, F_max], score f64
 * [B] or NULL. All device memory. Two launches.
 * FS2_EINVAL: a NULL pointer other than lens / score, B / F_max / hop / n_bins < 1, max_step < 0,
 * tau_min < 2, tau_min >= tau_max, ws_bytes below the need, sr not above 0.
 * FS2_EUNSUPPORTED: B > 65535, n_bins > FS2_F0_TRACK_BINS_MAX, max_step > FS2_F0_TRACK_STEP_MAX,
 * fs2_f0_track_lds_bytes above FS2_F0_TRACK_LDS_BYTES, B * F_max * max(tau_max + 1, 2 * n_bins, cap)
 * beyond 2^40.
 */
int fs2_f0_track(const double *cmnd, const int64_t *lens, int B, int F_max, int hop, double sr, int tau_min,
                 int tau_max, double f0_floor, double f0_ceil, const double *thr, const double *lm0, const double *lm1,
                 const double *lu, const double *edges, int n_bins, const double *trans_same,
                 const double *trans_switch, int max_step, double log_floor, double log_init, void *workspace,
                 int64_t ws_bytes, double *f0, int32_t *state, double *score, fs2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FS2HIP_F0_TRACK_H */
