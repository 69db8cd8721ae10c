// Stand-alone host program over csrc/resample_sizes.h: prints, for a grid of (n, up, down) up to
// INT32_MAX, what the helpers give, one line per point, for tools/resample_sizes_check.py to compare
// with Python's integers. Built with the address and undefined-behaviour sanitizers, so that an
// overflow or an out-of-range shift in the helpers is reported here, on the CPU.
//
//   S n up down n_taps -> out_len lds_bytes status
//   R n up down m      -> c lo hi
//   P tile up down     -> span
#include <stdint.h>
#include <stdio.h>

#include "resample_sizes.h"

int main() {
  const int64_t big = INT32_MAX;
  const int64_t terms[] = {1, 2, 3, 147, 160, 319, 320, 321, 441, 496, 497, 4096, 65536, (1 << 24), (1 << 24) + 1,
                           big - 1, big};
  const int64_t lens[] = {-1, 0, 1, 2, 319, 320, 321, 1000, 3001, 5200000, big - 1, big};
  for (int64_t up : terms)
    for (int64_t down : terms) {
      const int64_t half = rs_half(up, down);
      for (int64_t n : lens) {
        const int64_t taps[] = {2 * half + 1, 2 * half, 1};
        for (int64_t nt : taps)
          printf("S %lld %lld %lld %lld -> %lld %lld %d\n", (long long)n, (long long)up, (long long)down, (long long)nt,
                 (long long)rs_out_len(n, up, down), (long long)rs_lds_bytes(up, down), rs_check(n, up, down, nt));
        if (n < 1) continue;
        const int64_t M = rs_out_len(n, up, down);
        const int64_t ms[] = {0, 1, M / 3, M / 2, M - 2, M - 1};
        for (int64_t m : ms) {
          if (m < 0 || m >= M) continue;
          const RsRange r = rs_range(m, n, up, down, half);
          printf("R %lld %lld %lld %lld -> %lld %lld %lld\n", (long long)n, (long long)up, (long long)down, (long long)m,
                 (long long)r.c, (long long)r.lo, (long long)r.hi);
        }
      }
    }
  for (int64_t up : terms)
    for (int64_t down : terms)
      if (up <= FS2_RS_SIZE_CAP && down <= FS2_RS_SIZE_CAP)
        for (int64_t tile : {(int64_t)1, (int64_t)2048, (int64_t)(1 << 20)})
          printf("P %lld %lld %lld -> %lld\n", (long long)tile, (long long)up, (long long)down,
                 (long long)rs_span(tile, up, down));
  for (int64_t k : {(int64_t)0, (int64_t)31, (int64_t)32, (int64_t)8820, (int64_t)9920})
    printf("K %lld -> %lld\n", (long long)k, (long long)rs_slot(k));
  return 0;
}
