// The host-side arithmetic of include/fs2hip_pvoc.h in one place: the count of output frames (the kernel
// computes it with the same function) and the validation of a descriptor's sizes. Plain C++, in 64 bits
// and float64, so that it also compiles for the host alone (tools/pvoc_sizes_check.cpp runs it under
// the sanitizers).
#pragma once
#include <math.h>
#include <stdint.h>

#include "fs2hip_pvoc.h"

#ifdef __HIPCC__
#define FS2_PVOC_HD __host__ __device__
#else
#define FS2_PVOC_HD
#endif

// J of the header's rule 1: the number of j >= 0 with fl((double)j * rate) < T, saturated at
// FS2_PVOC_J_CAP. fl(j * rate) does not decrease with j for rate > 0, so J is the least j that fails the
// test: ceil(T / rate), put right by the test itself (one step either way at most, the quotient and
// the product being within a rounding of each other). A quotient that is infinite or past the cap
// saturates. No sum follows a product here, so nothing can be contracted.
FS2_PVOC_HD static inline int64_t pvoc_frames(int64_t T, double rate) {
  if (T < 1 || !(rate > 0.0) || !(rate - rate == 0.0)) return 0;  // NaN, +-inf, <= 0
  const double t = T < FS2_PVOC_J_CAP ? (double)T : (double)FS2_PVOC_J_CAP;
  const double q = ceil(t / rate);
  if (!(q < 2147483650.0)) return FS2_PVOC_J_CAP;
  int64_t j = (int64_t)q;
  while (j > 0 && !((double)(j - 1) * rate < t)) --j;
  while ((double)j * rate < t) ++j;
  return j < FS2_PVOC_J_CAP ? j : FS2_PVOC_J_CAP;
}

FS2_PVOC_HD static inline int64_t pvoc_clamp_frames(int64_t f, int64_t T_max) {
  return f < 0 ? 0 : (f > T_max ? T_max : f);
}

// FS2_OK, or why fs2_phase_vocoder refuses these sizes (the codes of include/fs2hip.h)
FS2_PVOC_HD static inline int pvoc_check(int64_t B, int64_t NB, int64_t T_max, int64_t J_max, int64_t spec_row_stride,
                                         int64_t recomb_row_stride) {
  if (B < 1 || NB < 1 || T_max < 1 || J_max < 1) return FS2_EINVAL;
  if (spec_row_stride < T_max || recomb_row_stride < J_max) return FS2_EINVAL;
  if (B > FS2_PVOC_B_MAX) return FS2_EUNSUPPORTED;
  return FS2_OK;
}

// FS2_EINVAL where a row's count, as far as the host can see it, exceeds J_max: rates_host is needed, and
// frames_host unless every row has T_max frames (frames_given == 0).
static inline int pvoc_check_counts(const int64_t *frames_host, int frames_given, const double *rates_host, int64_t B,
                                    int64_t T_max, int64_t J_max) {
  if (rates_host == nullptr || (frames_given && frames_host == nullptr)) return FS2_OK;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t T = frames_given ? pvoc_clamp_frames(frames_host[b], T_max) : T_max;
    if (pvoc_frames(T, rates_host[b]) > J_max) return FS2_EINVAL;
  }
  return FS2_OK;
}
