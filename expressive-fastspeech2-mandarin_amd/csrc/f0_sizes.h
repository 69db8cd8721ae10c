// The LDS layout of fs2_f0_yin (include/fs2hip_f0.h) in one place: the entry point sizes the launch
// with it, the kernel places its two regions with it, fs2_f0_lds_bytes reports it. Plain C++, in 64
// bits throughout (hop, W and tau_max are the caller's), so that it also compiles for the host alone.
#pragma once
#include <stdint.h>

#include "fs2hip_f0.h"

#ifdef __HIPCC__
#define FS2_F0_HD __host__ __device__
#else
#define FS2_F0_HD
#endif

#define FS2_F0_LAGS 8  // consecutive lags per thread

struct F0Sizes {
  int64_t tau_pad;  // tau_max rounded up to a multiple of FS2_F0_LAGS
  int64_t ts;       // table stride: tau_pad + 1 entries (lag 0 included)
  int64_t segs;     // block sums kept per group: shared hop blocks, then one tail per frame
  int64_t first;    // f64 elements of the first region: the padded span, later the group's tables
  int64_t bytes;    // both regions
};

#define FS2_F0_SIZE_CAP (1 << 24)  // a size beyond it is far past any LDS: bytes saturates, no product overflows

// hop, W, tau_max >= 1. Below the cap every product stays under 2^52.
FS2_F0_HD static inline F0Sizes f0_sizes(int64_t hop, int64_t W, int64_t tau_max) {
  F0Sizes s;
  if (hop > FS2_F0_SIZE_CAP || W > FS2_F0_SIZE_CAP || tau_max > FS2_F0_SIZE_CAP) {
    s.tau_pad = s.ts = s.segs = s.first = 0;
    s.bytes = INT64_MAX;
    return s;
  }
  s.tau_pad = (tau_max + FS2_F0_LAGS - 1) / FS2_F0_LAGS * FS2_F0_LAGS;
  s.ts = s.tau_pad + 1;
  const int64_t q = W / hop, r = W % hop;
  s.segs = (q > 0 ? FS2_F0_GROUP + q - 1 : 0) + (r > 0 ? FS2_F0_GROUP : 0);
  const int64_t span = (FS2_F0_GROUP - 1) * hop + W + s.tau_pad;
  const int64_t x = span + span / 8 + 1, tab = FS2_F0_GROUP * s.ts;
  s.first = x > tab ? x : tab;
  s.bytes = 8 * (s.first + s.segs * s.ts);
  return s;
}
