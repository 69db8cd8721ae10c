// Stand-alone host program over csrc/eval_sizes.h: prints, for a grid of (B, Tx, Ty) that walks the
// LDS limits of fs2_dtw and runs up to INT32_MAX, what the helpers give, one line per point, for
// tools/eval_sizes_check.py to compare with the Python mirror in fs2amd/_lib.py. Built with the
// address and undefined-behaviour sanitizers, so that an overflow in the helpers is reported here,
// on the CPU.
//
//   M Tx Ty          -> rows_bytes lds_bytes bitmap_words words
//   F Tx Ty bitmap   -> status form
//   W B Tx Ty        -> ws_bytes
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "eval_sizes.h"

int main() {
  const int64_t big = INT32_MAX;
  // 529 x 520 is the last Tx in LDS at Ty = 520; 6823 the last Tx whose three rows fit at all
  const int64_t Txs[] = {1,    2,    63,   64,        65,          130,     300,    512, 520, 524, 529, 530, 576, 577,
                         860,  1362, 1363, 2000,      6822,        6823,    6824,   65536,
                         (1 << 24), (1 << 24) + 1, big - 1, big};
  const int64_t Tys[] = {1, 2, 9, 64, 65, 130, 270, 512, 519, 520, 521, 524, 700, 860, 9000, 10176, 10177, 65536,
                         (1 << 24), (1 << 24) + 1, big - 1, big};
  const int64_t Bs[] = {1, 2, 64, 65535, (1 << 24), (1 << 24) + 1, big};
  for (int64_t Tx : Txs)
    for (int64_t Ty : Tys) {
      const bool capped = Tx > FS2_EV_SIZE_CAP || Ty > FS2_EV_SIZE_CAP;
      printf("M %lld %lld -> %lld %lld %lld %lld\n", (long long)Tx, (long long)Ty,
             (long long)ev_dtw_lds_bytes(Tx, Ty, 0), (long long)ev_dtw_lds_bytes(Tx, Ty, 1),
             (long long)(capped ? -1 : ev_dtw_bitmap_words(Tx, Ty)), (long long)ev_words(Tx));
      for (int bitmap : {FS2_DTW_AUTO, FS2_DTW_LDS, FS2_DTW_GLOBAL, 3, -1}) {
        int form = -1;
        const int rc = ev_dtw_form(Tx, Ty, bitmap, &form);
        printf("F %lld %lld %d -> %d %d\n", (long long)Tx, (long long)Ty, bitmap, rc, rc == FS2_OK ? form : -1);
      }
      for (int64_t B : Bs)
        printf("W %lld %lld %lld -> %lld\n", (long long)B, (long long)Tx, (long long)Ty,
               (long long)ev_dtw_ws_bytes(B, Tx, Ty));
    }
  // the refusals of sizes below 1
  for (int64_t T : {(int64_t)0, (int64_t)-1})
    for (int bitmap : {FS2_DTW_AUTO, FS2_DTW_GLOBAL}) {
      int form = -1;
      printf("F %lld %lld %d -> %d %d\n", (long long)T, 5LL, bitmap, ev_dtw_form(T, 5, bitmap, &form), -1);
      printf("F %lld %lld %d -> %d %d\n", 5LL, (long long)T, bitmap, ev_dtw_form(5, T, bitmap, &form), -1);
    }
  return 0;
}
