// The workspace layout and the LDS need of fs2_f0_track (include/fs2hip_f0_track.h) in one place: the
// entry point validates and sizes its launches with it, both kernels place their arrays with it, and
// fs2_f0_track_workspace_bytes / fs2_f0_track_lds_bytes report it. Plain C++, in 64 bits throughout
// and saturating at INT64_MAX, so that it also compiles for the host alone.
#pragma once
#include <stdint.h>

#include "fs2hip_f0_track.h"

#ifdef __HIPCC__
#define FS2_FT_HD __host__ __device__
#else
#define FS2_FT_HD
#endif

#define FS2_FT_SIZE_CAP (1 << 24)  // n_bins or max_step beyond it is far past any LDS: bytes saturates

FS2_FT_HD static inline int64_t ft_sat_mul(int64_t a, int64_t b) {  // a, b >= 0
  return b != 0 && a > INT64_MAX / b ? INT64_MAX : a * b;
}
FS2_FT_HD static inline int64_t ft_sat_add(int64_t a, int64_t b) {  // a, b >= 0
  return a > INT64_MAX - b ? INT64_MAX : a + b;
}
FS2_FT_HD static inline int64_t ft_round8(int64_t a) {  // a >= 0
  return a > INT64_MAX - 7 ? INT64_MAX : (a + 7) / 8 * 8;
}

// candidates of one frame that can survive: troughs lie at least two lags apart
FS2_FT_HD static inline int64_t ft_cap(int64_t tau_min, int64_t tau_max) {
  const int64_t troughs = (tau_max - tau_min + 1) / 2;
  return troughs < FS2_F0_TRACK_CAP_MAX ? troughs : FS2_F0_TRACK_CAP_MAX;
}

struct F0TrackSizes {
  int64_t cap;    // list entries per frame
  int64_t head;   // byte offset of the frame heads: int32 (lu index, count) per frame
  int64_t lm;     // of the log-masses, f64 [B * F_max * cap]
  int64_t fq;     // of the frequencies, f64 likewise
  int64_t bin;    // of the bins, int32 likewise
  int64_t bp;     // of the predecessor bytes [B * F_max * 2 N]
  int64_t bytes;  // of it all
};

// B, F_max, n_bins >= 1, 2 <= tau_min < tau_max. Every offset is a multiple of 8.
FS2_FT_HD static inline F0TrackSizes f0_track_sizes(int64_t B, int64_t F_max, int64_t tau_min, int64_t tau_max,
                                                    int64_t n_bins) {
  F0TrackSizes s;
  s.cap = ft_cap(tau_min, tau_max);
  const int64_t frames = ft_sat_mul(B, F_max), ents = ft_sat_mul(frames, s.cap);
  s.head = 0;
  s.lm = ft_round8(ft_sat_mul(frames, 8));
  s.fq = ft_sat_add(s.lm, ft_sat_mul(ents, 8));
  s.bin = ft_sat_add(s.fq, ft_sat_mul(ents, 8));
  s.bp = ft_sat_add(s.bin, ft_round8(ft_sat_mul(ents, 4)));
  s.bytes = ft_sat_add(s.bp, ft_round8(ft_sat_mul(frames, ft_sat_mul(n_bins, 2))));
  return s;
}

// f64 slots of one delta row: K slots of -inf on either side of the N bins
FS2_FT_HD static inline int64_t ft_row(int64_t n_bins, int64_t max_step) { return n_bins + 2 * max_step; }

// bytes of LDS of the recursion: two buffers of a voiced and an unvoiced row, two rows of voiced
// observations, then the back-trace's stage (and 8 bytes so that it can keep the source's alignment)
FS2_FT_HD static inline int64_t f0_track_lds_bytes(int64_t n_bins, int64_t max_step) {
  if (n_bins > FS2_FT_SIZE_CAP || max_step > FS2_FT_SIZE_CAP) return INT64_MAX;
  return 8 * (4 * ft_row(n_bins, max_step) + 2 * n_bins) + FS2_F0_TRACK_TB * 2 * n_bins + 8;
}
