// Stand-alone host program over csrc/vad_sizes.h: for a grid of sizes up to INT32_MAX it compares what
// the helpers give with a 128-bit restatement of the same formulas (exit status 1 and a line on stderr
// on a difference) and prints one line per point for tools/vad_sizes_check.py to compare with the
// Python mirror in fs2amd/_lib.py. Built with the address and undefined-behaviour sanitizers, so that
// an overflow or an out-of-range shift in the helpers is reported here, on the CPU.
//
//   F n hop               -> frames
//   G frame_length hop    -> g tile_frames tile_blocks lds_bytes fits
//   W B F_max frame_length hop -> workspace_bytes
//   C B n_max frame_length hop -> status
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "vad_sizes.h"

typedef __int128 i128;

static i128 gcd128(i128 a, i128 b) {
  while (b != 0) {
    const i128 t = a % b;
    a = b;
    b = t;
  }
  return a;
}

static int fail(const char *what, long long a, long long b, long long c, long long d) {
  fprintf(stderr, "%s differs from the 128-bit restatement at %lld %lld %lld %lld\n", what, a, b, c, d);
  return 1;
}

int main() {
  const int64_t big = INT32_MAX;
  const int64_t hops[] = {1, 2, 3, 255, 256, 257, 300, 333, 512, 640, 1000, 1024, 4096, 8191, 8192, 8193, 65536,
                          big - 1, big};
  const int64_t lens[] = {-1, 0, 1, 2, 255, 256, 257, 511, 512, 513, 1024, 3001, 220500, big - 1, big};
  const int64_t rows[] = {-1, 0, 1, 2, 7, 64, 65535, 65536, big};
  for (int64_t hop : hops)
    for (int64_t n : lens) {
      const int64_t F = vad_frames(n, hop);
      if ((i128)F != (n < 1 ? (i128)0 : 1 + (i128)n / hop)) return fail("vad_frames", n, hop, 0, 0);
      printf("F %lld %lld -> %lld\n", (long long)n, (long long)hop, (long long)F);
    }
  for (int64_t L : hops)
    for (int64_t hop : hops) {
      if (hop <= L) {
        const i128 g = gcd128(L, hop), q = L / g, h = hop / g;
        i128 G = q > FS2_VAD_SUMS_MAX ? 0 : (FS2_VAD_SUMS_MAX - q) / h + 1;
        G = G < FS2_VAD_TILE_FRAMES ? G : FS2_VAD_TILE_FRAMES;
        const int64_t Gh = vad_tile_frames(L, hop);
        const int64_t nb = Gh >= 1 ? vad_tile_blocks(L, hop, Gh) : 0;
        if ((i128)vad_gcd(L, hop) != g || (i128)Gh != G || (Gh >= 1 && (i128)nb != (G - 1) * h + q) ||
            nb > FS2_VAD_SUMS_MAX)
          return fail("the tile", L, hop, 0, 0);
        const i128 gs4 = g | 1;
        const i128 gs2 = g + ((2 - g % 4) + 4) % 4;
        if ((i128)vad_row_stride((int64_t)g, 4) != gs4 || (i128)vad_row_stride((int64_t)g, 2) != gs2 || gs2 % 4 != 2)
          return fail("vad_row_stride", L, hop, 0, 0);
        if ((i128)vad_lds_bytes(L, hop) != 8 * q + 4 * gs4 ||
            vad_fits(L, hop) != (8 * q <= FS2_VAD_SUMS_BYTES && 4 * gs4 <= FS2_VAD_AREA_BYTES))
          return fail("vad_lds_bytes", L, hop, 0, 0);
        printf("G %lld %lld -> %lld %lld %lld %lld %d\n", (long long)L, (long long)hop, (long long)vad_gcd(L, hop),
               (long long)Gh, (long long)nb, (long long)vad_lds_bytes(L, hop), vad_fits(L, hop));
      }
      for (int64_t B : rows) {
        for (int64_t F : lens) {
          const int64_t ws = vad_workspace_bytes(B, F, L, hop);
          i128 want = 0;
          if (B >= 1 && F >= 1 && hop <= L && vad_tile_frames(L, hop) >= 1) {
            const i128 G = vad_tile_frames(L, hop);
            want = 8 * (i128)B * (((i128)F + G - 1) / G);
            if (want > INT64_MAX) want = INT64_MAX;
          }
          if ((i128)ws != want) return fail("vad_workspace_bytes", B, F, L, hop);
          printf("W %lld %lld %lld %lld -> %lld\n", (long long)B, (long long)F, (long long)L, (long long)hop,
                 (long long)ws);
        }
        for (int64_t n : lens) {
          const int rc = vad_check(B, n, L, hop);
          int want = FS2_OK;
          if (B < 1 || n < 1 || hop > L) {
            want = FS2_EINVAL;
          } else {
            const i128 F = 1 + (i128)n / hop;
            if (B > FS2_VAD_B_MAX || !vad_fits(L, hop) || F > INT32_MAX || 8 * (i128)B * F > INT32_MAX - 7)
              want = FS2_EUNSUPPORTED;
          }
          if (rc != want) return fail("vad_check", B, n, L, hop);
          printf("C %lld %lld %lld %lld -> %d\n", (long long)B, (long long)n, (long long)L, (long long)hop, rc);
        }
      }
    }
  // sizes below 1
  for (int64_t L : {(int64_t)-1, (int64_t)0, (int64_t)1024})
    for (int64_t hop : {(int64_t)-1, (int64_t)0, (int64_t)256, (int64_t)2048}) {
      printf("W %d %d %lld %lld -> %lld\n", 4, 100, (long long)L, (long long)hop,
             (long long)vad_workspace_bytes(4, 100, L, hop));
      printf("C %d %d %lld %lld -> %d\n", 4, 100, (long long)L, (long long)hop, vad_check(4, 100, L, hop));
      printf("L %lld %lld -> %lld\n", (long long)L, (long long)hop, (long long)vad_lds_bytes(L, hop));
    }
  return 0;
}
