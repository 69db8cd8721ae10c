// The size arithmetic of fs2_dtw (include/fs2hip_eval.h) in one place: the entry point validates and
// sizes its launch with it, the kernel lays out its LDS with it, and fs2_dtw_lds_bytes /
// fs2_dtw_ws_bytes report it. Plain C++, in 64 bits throughout, so that it also compiles for the host
// alone. With Tx, Ty <= FS2_EV_SIZE_CAP = 2^24 a bitmap has fewer than 2^25 * 2 * 2^18 = 2^44 words;
// the product with B is checked before it is formed.
#pragma once
#include <stdint.h>

#include "fs2hip_eval.h"

#ifdef __HIPCC__
#define FS2_EV_HD __host__ __device__
#else
#define FS2_EV_HD
#endif

#define FS2_EV_SIZE_CAP (1 << 24)  // a size beyond it is far past any LDS: bytes saturates

// 64-bit words of one bit plane of one anti-diagonal, indexed by i >> 6: ceil(Tx / 64)
FS2_EV_HD static inline int64_t ev_words(int64_t Tx) { return (Tx + 63) >> 6; }

// f64 slots of one anti-diagonal: slot 1 + i is cell i; slot 0 and the slot past the last cell are +inf
FS2_EV_HD static inline int64_t ev_dtw_row(int64_t Tx) { return Tx + 3; }

// anti-diagonals of a Tx x Ty matrix, which is also the longest path
FS2_EV_HD static inline int64_t ev_dtw_diags(int64_t Tx, int64_t Ty) { return Tx + Ty - 1; }

// 64-bit words of one utterance's step bitmap: two planes per anti-diagonal
FS2_EV_HD static inline int64_t ev_dtw_bitmap_words(int64_t Tx, int64_t Ty) {
  return ev_dtw_diags(Tx, Ty) * 2 * ev_words(Tx);
}

// bytes of LDS of fs2_dtw: the three rows, then the bitmap when it lives there. Tx, Ty >= 1.
FS2_EV_HD static inline int64_t ev_dtw_lds_bytes(int64_t Tx, int64_t Ty, int in_lds) {
  if (Tx > FS2_EV_SIZE_CAP || Ty > FS2_EV_SIZE_CAP) return INT64_MAX;
  return 8 * (3 * ev_dtw_row(Tx) + (in_lds ? ev_dtw_bitmap_words(Tx, Ty) : 0));
}

// bytes of the global bitmap; INT64_MAX beyond the cap. B, Tx, Ty >= 1.
FS2_EV_HD static inline int64_t ev_dtw_ws_bytes(int64_t B, int64_t Tx, int64_t Ty) {
  if (B > FS2_EV_SIZE_CAP || Tx > FS2_EV_SIZE_CAP || Ty > FS2_EV_SIZE_CAP) return INT64_MAX;
  const int64_t per = ev_dtw_bitmap_words(Tx, Ty);  // < 2^44
  return per > (INT64_MAX >> 3) / B ? INT64_MAX : 8 * per * B;
}

// The form fs2_dtw takes: FS2_DTW_LDS or FS2_DTW_GLOBAL in *form and FS2_OK, or why it refuses.
FS2_EV_HD static inline int ev_dtw_form(int64_t Tx, int64_t Ty, int bitmap, int *form) {
  if (Tx < 1 || Ty < 1) return FS2_EINVAL;
  if (bitmap != FS2_DTW_AUTO && bitmap != FS2_DTW_LDS && bitmap != FS2_DTW_GLOBAL) return FS2_EINVAL;
  if (ev_dtw_lds_bytes(Tx, Ty, 0) > FS2_DTW_LDS_BYTES) return FS2_EUNSUPPORTED;
  const bool fits = ev_dtw_lds_bytes(Tx, Ty, 1) <= FS2_DTW_LDS_BYTES;
  if (bitmap == FS2_DTW_LDS && !fits) return FS2_EUNSUPPORTED;
  *form = bitmap == FS2_DTW_GLOBAL || !fits ? FS2_DTW_GLOBAL : FS2_DTW_LDS;
  return FS2_OK;
}
