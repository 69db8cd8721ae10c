// The size arithmetic of fs2_mas and fs2_forward_sum (include/fs2hip_align.h) in one place: the entry
// points validate and size their launches with it, the kernels lay out their LDS with it, and
// fs2_mas_lds_bytes / fs2_mas_ws_bytes / fs2_forward_sum_lds_bytes report it. Plain C++, in 64 bits
// throughout, so that it also compiles for the host alone. With T, L <= FS2_AL_SIZE_CAP = 2^24 a
// bitmap has fewer than 2^24 * 2^18 = 2^42 words; the product with B is checked before it is formed.
#pragma once
#include <stdint.h>

#include "fs2hip_align.h"

#ifdef __HIPCC__
#define FS2_AL_HD __host__ __device__
#else
#define FS2_AL_HD
#endif

#define FS2_AL_SIZE_CAP (1 << 24)  // a size beyond it is far past any LDS: bytes saturates

// 64-bit words of one bitmap row: ceil(L / 64)
FS2_AL_HD static inline int64_t al_words(int64_t L) { return (L + 63) >> 6; }

// f64 slots of one v row: slot 0 is v[-1] = -inf, slot 1 + j is v[j]
FS2_AL_HD static inline int64_t al_mas_row(int64_t L) { return L + 1; }

// bytes of LDS of fs2_mas: the two rows, then the bitmap when it lives there. T, L >= 1.
FS2_AL_HD static inline int64_t al_mas_lds_bytes(int64_t T, int64_t L, int in_lds) {
  if (T > FS2_AL_SIZE_CAP || L > FS2_AL_SIZE_CAP) return INT64_MAX;
  return 8 * (2 * al_mas_row(L) + (in_lds ? T * al_words(L) : 0));
}

// bytes of the global bitmap; INT64_MAX beyond the cap. B, T, L >= 1.
FS2_AL_HD static inline int64_t al_mas_ws_bytes(int64_t B, int64_t T, int64_t L) {
  if (B > FS2_AL_SIZE_CAP || T > FS2_AL_SIZE_CAP || L > FS2_AL_SIZE_CAP) return INT64_MAX;
  const int64_t per = T * al_words(L);  // < 2^42
  return per > (INT64_MAX >> 3) / B ? INT64_MAX : 8 * per * B;
}

// f64 slots of one state row of the forward sum: two -inf slots on either side of the 2 L + 1 states
FS2_AL_HD static inline int64_t al_fs_row(int64_t L) { return 2 * L + 5; }

// bytes of LDS of fs2_forward_sum(_bwd): the two state rows, then max and log-sum per frame
FS2_AL_HD static inline int64_t al_fs_lds_bytes(int64_t T, int64_t L) {
  if (T > FS2_AL_SIZE_CAP || L > FS2_AL_SIZE_CAP) return INT64_MAX;
  return 8 * (2 * al_fs_row(L) + 2 * T);
}

// The form fs2_mas takes: FS2_MAS_LDS or FS2_MAS_GLOBAL in *form and FS2_OK, or why it refuses.
FS2_AL_HD static inline int al_mas_form(int64_t T, int64_t L, int bitmap, int *form) {
  if (T < 1 || L < 1) return FS2_EINVAL;
  if (bitmap != FS2_MAS_AUTO && bitmap != FS2_MAS_LDS && bitmap != FS2_MAS_GLOBAL) return FS2_EINVAL;
  if (al_mas_lds_bytes(T, L, 0) > FS2_MAS_LDS_BYTES) return FS2_EUNSUPPORTED;
  const bool fits = al_mas_lds_bytes(T, L, 1) <= FS2_MAS_LDS_BYTES;
  if (bitmap == FS2_MAS_LDS && !fits) return FS2_EUNSUPPORTED;
  *form = bitmap == FS2_MAS_GLOBAL || !fits ? FS2_MAS_GLOBAL : FS2_MAS_LDS;
  return FS2_OK;
}
