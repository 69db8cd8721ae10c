// Stand-alone host program over csrc/align_sizes.h: prints, for a grid of (B, T, L) that walks the
// LDS limits of fs2_mas and fs2_forward_sum and runs up to INT32_MAX, what the helpers give, one line
// per point, for tools/align_sizes_check.py to compare with the Python mirror in fs2amd/_lib.py.
// Built with the address and undefined-behaviour sanitizers, so that an overflow in the helpers is
// reported here, on the CPU.
//
//   M T L          -> rows_bytes lds_bytes fs_bytes words
//   F T L bitmap   -> status form
//   W B T L        -> ws_bytes
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "align_sizes.h"

int main() {
  const int64_t big = INT32_MAX;
  const int64_t Ts[] = {1, 2, 63, 64, 65, 136, 860, 1000, 1279, 1280, 1281, 4071, 4072, 4096, 10237, 10238, 10239, 65536,
                        (1 << 24), (1 << 24) + 1, big - 1, big};
  const int64_t Ls[] = {1, 2, 63, 64, 65, 70, 128, 129, 150, 1000, 2045, 2046, 2047, 10238, 10239, 10240, 65536,
                        (1 << 24), (1 << 24) + 1, big - 1, big};
  const int64_t Bs[] = {1, 2, 64, 65535, (1 << 24), (1 << 24) + 1, big};
  for (int64_t T : Ts)
    for (int64_t L : Ls) {
      printf("M %lld %lld -> %lld %lld %lld %lld\n", (long long)T, (long long)L, (long long)al_mas_lds_bytes(T, L, 0),
             (long long)al_mas_lds_bytes(T, L, 1), (long long)al_fs_lds_bytes(T, L), (long long)al_words(L));
      for (int bitmap : {FS2_MAS_AUTO, FS2_MAS_LDS, FS2_MAS_GLOBAL, 3, -1}) {
        int form = -1;
        const int rc = al_mas_form(T, L, bitmap, &form);
        printf("F %lld %lld %d -> %d %d\n", (long long)T, (long long)L, bitmap, rc, rc == FS2_OK ? form : -1);
      }
      for (int64_t B : Bs)
        printf("W %lld %lld %lld -> %lld\n", (long long)B, (long long)T, (long long)L,
               (long long)al_mas_ws_bytes(B, T, L));
    }
  // the refusals of sizes below 1
  for (int64_t T : {(int64_t)0, (int64_t)-1})
    for (int bitmap : {FS2_MAS_AUTO, FS2_MAS_GLOBAL}) {
      int form = -1;
      printf("F %lld %lld %d -> %d %d\n", (long long)T, 5LL, bitmap, al_mas_form(T, 5, bitmap, &form), -1);
      printf("F %lld %lld %d -> %d %d\n", 5LL, (long long)T, bitmap, al_mas_form(5, T, bitmap, &form), -1);
    }
  return 0;
}
