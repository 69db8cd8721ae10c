// The size arithmetic of include/fs2hip_iir.h in one place: the entry points validate and size their
// launches with it, and fs2_iir_blocks / fs2_iir_chunks / fs2_loudness_blocks /
// fs2_loudness_workspace_bytes report it. Plain C++, in 64 bits throughout and saturating, so that it
// also compiles for the host alone (tools/iir_sizes_check.cpp runs it under the sanitizers).
#pragma once
#include <stdint.h>

#include "fs2hip_iir.h"

#ifdef __HIPCC__
#define FS2_IIR_HD __host__ __device__
#else
#define FS2_IIR_HD
#endif

#define FS2_IIR_PAD 65                                        // doubles between two blocks in LDS
#define FS2_IIR_CHUNK_BLOCKS (FS2_IIR_CHUNK / FS2_IIR_BLOCK)  // 256: one block per thread
#define FS2_LOUD_LEAVES_MAX (FS2_LOUD_H_MAX / 8)              // leaves of one sub-block, at most

// blocks of a row of n samples: 0 for n < 1, else ceil(n / 64)
FS2_IIR_HD static inline int64_t iir_blocks(int64_t n) {
  return n < 1 ? 0 : (n - 1) / FS2_IIR_BLOCK + 1;
}

// chunks of a row of n samples: 0 for n < 1, else ceil(n / 16384)
FS2_IIR_HD static inline int64_t iir_chunks(int64_t n) {
  return n < 1 ? 0 : (n - 1) / FS2_IIR_CHUNK + 1;
}

// gating blocks of a row of n samples at hop H >= 1: 0 for n < 4 H, else (n - 4 H) / H + 1
FS2_IIR_HD static inline int64_t loud_blocks(int64_t n, int64_t H) {
  if (n < 1 || H > INT64_MAX / 4 || n < 4 * H) return 0;
  return (n - 4 * H) / H + 1;
}

// doubles of one row of the gate's workspace: J + 3 sub-block sums and the two tree buffers;
// INT64_MAX where that does not fit
FS2_IIR_HD static inline int64_t loud_row_doubles(int64_t J) {
  if (J < 1) return 0;
  return J > INT64_MAX / 4 ? INT64_MAX : (J + 3) + J + (J + 1) / 2;
}

// bytes of the gate's workspace; 0 for a size below 1 or J == 0; INT64_MAX where it does not fit
FS2_IIR_HD static inline int64_t loud_workspace_bytes(int64_t B, int64_t n_max, int64_t H) {
  if (B < 1 || n_max < 1 || H < 1) return 0;
  const int64_t rw = loud_row_doubles(loud_blocks(n_max, H));
  if (rw < 1) return 0;
  if (rw == INT64_MAX) return INT64_MAX;
  return B > INT64_MAX / 8 / rw ? INT64_MAX : 8 * B * rw;
}

// FS2_OK, or why fs2_sosfilt refuses these sizes (the codes of include/fs2hip.h)
FS2_IIR_HD static inline int iir_check(int64_t B, int64_t n_max, int64_t S, int64_t row_stride) {
  if (B < 1 || n_max < 1 || S < 1 || row_stride < n_max) return FS2_EINVAL;
  if (S > FS2_IIR_S_MAX || B > FS2_IIR_B_MAX) return FS2_EUNSUPPORTED;
  return FS2_OK;
}

// the same for fs2_loudness_gate
FS2_IIR_HD static inline int loud_check(int64_t B, int64_t n_max, int64_t H) {
  if (B < 1 || n_max < 1 || H < 1) return FS2_EINVAL;
  if (H > FS2_LOUD_H_MAX || B > FS2_IIR_B_MAX) return FS2_EUNSUPPORTED;
  if (loud_workspace_bytes(B, n_max, H) == INT64_MAX) return FS2_EUNSUPPORTED;
  return FS2_OK;
}

// the same for fs2_gain_int16
FS2_IIR_HD static inline int gain_check(int64_t B, int64_t n_max, int64_t row_stride) {
  if (B < 1 || n_max < 1 || row_stride < n_max) return FS2_EINVAL;
  if (B > FS2_IIR_B_MAX) return FS2_EUNSUPPORTED;
  return FS2_OK;
}
