// Stand-alone host program over csrc/iir_sizes.h: it compares the block, chunk and gating-block counts
// with their definitions (counted one by one where that is small enough), the workspace size with its
// restatement in unsigned 128-bit arithmetic and the three status functions with the tables of
// include/fs2hip_iir.h, exits with status 1 and a line on stderr on a difference, and prints one line per
// point for tools/iir_sizes_check.py to compare with the Python mirror in fs2amd/_lib.py. Built with the
// address and undefined-behaviour sanitizers, so that an overflow in the helpers is reported here, on
// the CPU.
//
//   K n               -> blocks chunks
//   J n H             -> gating blocks
//   W B n_max H       -> workspace bytes
//   S B n_max S rs    -> status of iir_check
//   L B n_max H       -> status of loud_check
//   G B n_max rs      -> status of gain_check
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "iir_sizes.h"

static int fail(const char *what, long long a, long long b) {
  fprintf(stderr, "%s differs from its restatement at %lld %lld\n", what, a, b);
  return 1;
}

int main() {
  const int64_t big = INT32_MAX, huge = INT64_MAX;
  const int64_t ns[] = {-7, 0, 1, 2, 63, 64, 65, 127, 128, 4095, 4096, 4097, 8819, 8820, 8821, 11024, 11025, 16383, 16384,
                        16385, 220500, big - 1, big, big + 1, (int64_t)1 << 40, huge - 1, huge};
  for (int64_t n : ns) {
    const int64_t kb = iir_blocks(n), kc = iir_chunks(n);
    if (n >= 1 && n < 300000) {
      int64_t b = 0, c = 0;
      for (int64_t t = 0; t < n; t += FS2_IIR_BLOCK) ++b;
      for (int64_t t = 0; t < n; t += FS2_IIR_CHUNK) ++c;
      if (b != kb || c != kc) return fail("iir_blocks / iir_chunks", n, kb);
    }
    if (n < 1 && (kb != 0 || kc != 0)) return fail("iir_blocks (empty)", n, kb);
    if (n >= 1 && ((kb - 1) * FS2_IIR_BLOCK >= n || (kb > huge / FS2_IIR_BLOCK ? false : kb * FS2_IIR_BLOCK < n)))
      return fail("iir_blocks (bounds)", n, kb);
    printf("K %lld -> %lld %lld\n", (long long)n, (long long)kb, (long long)kc);
  }
  const int64_t Hs[] = {1, 2, 7, 1600, 2205, 4800, 32768, 32769, big, huge / 4, huge / 4 + 1, huge};
  for (int64_t n : ns)
    for (int64_t H : Hs) {
      const int64_t J = loud_blocks(n, H);
      if (n >= 1 && n < 300000 && H < 300000) {
        int64_t c = 0;
        for (int64_t j = 0; j * H + 4 * H <= n && c < 400000; ++j) ++c;
        if (c != J) return fail("loud_blocks", n, H);
      }
      if (J < 0) return fail("loud_blocks (sign)", n, H);
      printf("J %lld %lld -> %lld\n", (long long)n, (long long)H, (long long)J);
    }
  const int64_t Bs[] = {-1, 0, 1, 7, 64, 65535, 65536, big, huge};
  for (int64_t B : Bs)
    for (int64_t n : ns)
      for (int64_t H : {(int64_t)0, (int64_t)1, (int64_t)2205, (int64_t)32768, (int64_t)32769, big}) {
        const int64_t w = loud_workspace_bytes(B, n, H);
        int64_t want = 0;
        if (B >= 1 && n >= 1 && H >= 1) {
          const int64_t J = loud_blocks(n, H);
          if (J >= 1) {
            const unsigned __int128 v = (unsigned __int128)8 * (unsigned __int128)B *
                                        ((unsigned __int128)(J + 3) + (unsigned __int128)J + (unsigned __int128)((J + 1) / 2));
            want = v > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)v;
          }
        }
        if (w != want) return fail("loud_workspace_bytes", B, n);
        printf("W %lld %lld %lld -> %lld\n", (long long)B, (long long)n, (long long)H, (long long)w);
        const int rc = loud_check(B, n, H);
        int wrc = FS2_OK;
        if (B < 1 || n < 1 || H < 1)
          wrc = FS2_EINVAL;
        else if (H > FS2_LOUD_H_MAX || B > FS2_IIR_B_MAX || want == INT64_MAX)
          wrc = FS2_EUNSUPPORTED;
        if (rc != wrc) return fail("loud_check", B, n);
        printf("L %lld %lld %lld -> %d\n", (long long)B, (long long)n, (long long)H, rc);
      }
  for (int64_t B : Bs)
    for (int64_t n : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)220500, big})
      for (int64_t d : {(int64_t)-1, (int64_t)0, (int64_t)9}) {
        const int64_t rs = n + d;
        for (int64_t S : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)2, (int64_t)8, (int64_t)9, big}) {
          const int rc = iir_check(B, n, S, rs);
          int want = FS2_OK;
          if (B < 1 || n < 1 || S < 1 || d < 0)
            want = FS2_EINVAL;
          else if (S > FS2_IIR_S_MAX || B > FS2_IIR_B_MAX)
            want = FS2_EUNSUPPORTED;
          if (rc != want) return fail("iir_check", B, S);
          printf("S %lld %lld %lld %lld -> %d\n", (long long)B, (long long)n, (long long)S, (long long)rs, rc);
        }
        const int rc = gain_check(B, n, rs);
        int want = FS2_OK;
        if (B < 1 || n < 1 || d < 0)
          want = FS2_EINVAL;
        else if (B > FS2_IIR_B_MAX)
          want = FS2_EUNSUPPORTED;
        if (rc != want) return fail("gain_check", B, n);
        printf("G %lld %lld %lld -> %d\n", (long long)B, (long long)n, (long long)rs, rc);
      }
  return 0;
}
