// The size arithmetic of fs2_resample (include/fs2hip_resample.h) in one place: the entry point
// validates and sizes the launch with it, the kernel finds each output's input range with it, and
// fs2_resample_out_len / fs2_resample_lds_bytes report it. Plain C++, in 64 bits throughout, so that
// it also compiles for the host alone. For n <= INT32_MAX and up, down <= INT32_MAX every product
// below stays under 2^63: n * up + down - 1 < 2^62 + 2^31, and m * down <= n * up + down for m < M.
#pragma once
#include <stdint.h>

#include "fs2hip_resample.h"

#ifdef __HIPCC__
#define FS2_RS_HD __host__ __device__
#else
#define FS2_RS_HD
#endif

#define FS2_RS_SIZE_CAP (1 << 24)  // a ratio term beyond it is far past any LDS: bytes saturates
#define FS2_RS_PAD_SHIFT 5         // one f64 of padding after every 32 taps

// 10 * max(up, down): the taps on either side of the centre
FS2_RS_HD static inline int64_t rs_half(int64_t up, int64_t down) { return 10 * (up > down ? up : down); }

// ceil(n * up / down); 0 for n < 1. up, down >= 1.
FS2_RS_HD static inline int64_t rs_out_len(int64_t n, int64_t up, int64_t down) {
  return n < 1 ? 0 : (n * up + down - 1) / down;
}

// where tap k lives in LDS
FS2_RS_HD static inline int64_t rs_slot(int64_t k) { return k + (k >> FS2_RS_PAD_SHIFT); }

// bytes of LDS for the padded table of N = 2 * half + 1 taps. up, down >= 1.
FS2_RS_HD static inline int64_t rs_lds_bytes(int64_t up, int64_t down) {
  if (up > FS2_RS_SIZE_CAP || down > FS2_RS_SIZE_CAP) return INT64_MAX;
  const int64_t N = 2 * rs_half(up, down) + 1;
  return 8 * (rs_slot(N) + 1);
}

struct RsRange {
  int64_t c;   // m * down + half: tap index of input sample 0 (h[c - i * up] pairs with x[i])
  int64_t lo;  // first input sample of output m
  int64_t hi;  // last one; hi < lo: no sample
};

// 0 <= m < rs_out_len(n, up, down), n >= 1
FS2_RS_HD static inline RsRange rs_range(int64_t m, int64_t n, int64_t up, int64_t down, int64_t half) {
  RsRange r;
  r.c = m * down + half;
  const int64_t a = r.c - 2 * half;  // the smallest i * up whose tap index is <= 2 * half
  r.lo = a <= 0 ? 0 : (a + up - 1) / up;
  const int64_t h = r.c / up;
  r.hi = h < n - 1 ? h : n - 1;
  return r;
}

// An upper bound on the input samples that `tile` consecutive outputs read, first sample of the first
// to last sample of the last: hi(m + tile - 1) - lo(m) + 1 <= ((tile - 1) * down + 2 * half) / up + 1.
// up, down >= 1 and within FS2_RS_SIZE_CAP, tile <= 2^20.
FS2_RS_HD static inline int64_t rs_span(int64_t tile, int64_t up, int64_t down) {
  return ((tile - 1) * down + 2 * rs_half(up, down)) / up + 2;
}

// FS2_OK, or why fs2_resample refuses these sizes (the codes of include/fs2hip.h)
FS2_RS_HD static inline int rs_check(int64_t n_max, int64_t up, int64_t down, int64_t n_taps) {
  if (n_max < 1 || up < 1 || down < 1) return FS2_EINVAL;
  if (up == 1 && down == 1) return FS2_OK;  // no FIR, no table
  if (rs_lds_bytes(up, down) > FS2_RESAMPLE_LDS_BYTES) {
    // the tap count is checked only where it cannot overflow
    return up <= FS2_RS_SIZE_CAP && down <= FS2_RS_SIZE_CAP && n_taps != 2 * rs_half(up, down) + 1 ? FS2_EINVAL
                                                                                                  : FS2_EUNSUPPORTED;
  }
  if (n_taps != 2 * rs_half(up, down) + 1) return FS2_EINVAL;
  if (rs_out_len(n_max, up, down) > INT32_MAX) return FS2_EUNSUPPORTED;
  return FS2_OK;
}
