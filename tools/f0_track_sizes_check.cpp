// Stand-alone host program over csrc/f0_track_sizes.h: for a grid of (B, F_max, tau_min, tau_max,
// n_bins) and (n_bins, max_step) that runs up to INT32_MAX it compares what the header gives with
// the same formula restated here in 128-bit arithmetic (exit status 1 on a difference), and prints
// one line per point for tools/f0_track_sizes_check.py to compare with the Python mirror in
// fs2amd/_lib.py. Built with the address and undefined-behaviour sanitizers, so that an overflow in
// the header is reported here, on the CPU.
//
//   W B F_max tau_min tau_max n_bins -> cap bytes
//   L n_bins max_step                -> lds_bytes
#include <stdint.h>
#include <stdio.h>

#include "f0_track_sizes.h"

typedef unsigned __int128 u128;

static u128 r8(u128 a) { return (a + 7) / 8 * 8; }
static int64_t sat(u128 a) { return a > (u128)INT64_MAX ? INT64_MAX : (int64_t)a; }

int main() {
  const int64_t big = INT32_MAX;
  const int64_t Bs[] = {1, 2, 20, 64, 65535, 65536, (1 << 24) + 1, big};
  const int64_t Fs[] = {1, 2, 36, 860, 65536, (1 << 24), (1 << 24) + 1, big - 1, big};
  const int64_t lags[][2] = {{2, 3},  {2, 4},   {4, 20},      {27, 311},  {27, 228},     {27, 229},
                             {27, 230}, {2, 65536}, {2, big}, {big - 1, big}, {big - 3, big}};
  const int64_t Ns[] = {1, 2, 28, 210, 256, 257, 65536, (1 << 24), (1 << 24) + 1, big};
  const int64_t Ks[] = {0, 1, 3, 12, 63, 64, 3000, (1 << 24), (1 << 24) + 1, big};
  int bad = 0;
  for (int64_t B : Bs)
    for (int64_t F : Fs)
      for (const auto &lg : lags)
        for (int64_t N : Ns) {
          const F0TrackSizes s = f0_track_sizes(B, F, lg[0], lg[1], N);
          const u128 troughs = (u128)(lg[1] - lg[0] + 1) / 2;
          const u128 cap = troughs < FS2_F0_TRACK_CAP_MAX ? troughs : FS2_F0_TRACK_CAP_MAX;
          const u128 frames = (u128)B * (u128)F, ents = frames * cap;
          const u128 lm = r8(frames * 8), fq = lm + ents * 8, bin = fq + ents * 8, bp = bin + r8(ents * 4);
          const u128 bytes = bp + r8(frames * 2 * (u128)N);
          if ((u128)s.cap != cap || s.head != 0 || s.lm != sat(lm) || s.fq != sat(fq) || s.bin != sat(bin) ||
              s.bp != sat(bp) || s.bytes != sat(bytes)) {
            fprintf(stderr, "mismatch at %lld %lld %lld %lld %lld\n", (long long)B, (long long)F, (long long)lg[0],
                    (long long)lg[1], (long long)N);
            bad = 1;
          }
          printf("W %lld %lld %lld %lld %lld -> %lld %lld\n", (long long)B, (long long)F, (long long)lg[0],
                 (long long)lg[1], (long long)N, (long long)s.cap, (long long)s.bytes);
        }
  for (int64_t N : Ns)
    for (int64_t K : Ks) {
      const int64_t got = f0_track_lds_bytes(N, K);
      const bool capped = N > FS2_FT_SIZE_CAP || K > FS2_FT_SIZE_CAP;
      const u128 want = 8 * (4 * ((u128)N + 2 * (u128)K) + 2 * (u128)N) + (u128)FS2_F0_TRACK_TB * 2 * (u128)N + 8;
      if (got != (capped ? INT64_MAX : sat(want))) {
        fprintf(stderr, "mismatch at N %lld K %lld\n", (long long)N, (long long)K);
        bad = 1;
      }
      printf("L %lld %lld -> %lld\n", (long long)N, (long long)K, (long long)got);
    }
  return bad;
}
