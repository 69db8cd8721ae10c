// Stand-alone host program over csrc/pvoc_sizes.h: it compares pvoc_frames with the definition (the
// least j whose fl(j * rate) is not below T, found by bisection over the monotone test, and for small
// counts by trying every j) and the size checks with their restatement, exits with status 1 and a line
// on stderr on a difference, and prints one line per point for tools/pvoc_sizes_check.py to compare
// with the Python mirror in fs2amd/_lib.py. Built with the address and undefined-behaviour sanitizers,
// so that an overflow or a conversion out of range in the helpers is reported here, on the CPU.
//
//   F T rate(hex float)                                   -> J
//   C B NB T_max J_max spec_row_stride recomb_row_stride   -> status
//   V J_max                                               -> status of pvoc_check_counts over a fixed batch
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "pvoc_sizes.h"

static int64_t by_bisection(int64_t T, double rate) {
  if (T < 1 || !(rate > 0.0) || isinf(rate) || isnan(rate)) return 0;
  const double t = T < FS2_PVOC_J_CAP ? (double)T : (double)FS2_PVOC_J_CAP;
  int64_t lo = 0, hi = FS2_PVOC_J_CAP;  // the test holds at lo = 0; the answer is the least j in (lo, hi] that
  if ((double)hi * rate < t) return hi;  // fails it, or the cap
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((double)mid * rate < t) lo = mid; else hi = mid;
  }
  return hi;
}

static int fail(const char *what, long long a, double r) {
  fprintf(stderr, "%s differs from its restatement at %lld %a\n", what, a, r);
  return 1;
}

int main() {
  const int64_t big = INT32_MAX;
  const int64_t Ts[] = {-5, 0, 1, 2, 3, 63, 64, 65, 130, 860, 4136, 100000, big - 1, big, big + 1, (int64_t)1 << 40};
  const double rates[] = {0.0, -1.0, NAN, INFINITY, -INFINITY, 5e-324, 1e-300, 1e-12, 1e-9, 1.0 / 3.0, 0.25, 0.5, 0.8,
                          0.9, 1.0, 1.0594630943592953, 1.25, 1.5, 2.0, 3.7, 1.0 / 0.3, 0.1, 0.7, 63.99999999999999,
                          64.0, 1e9, 4294967296.0, 1e300, 1.7976931348623157e308};
  for (int64_t T : Ts)
    for (double r : rates) {
      const int64_t J = pvoc_frames(T, r);
      if (J != by_bisection(T, r)) return fail("pvoc_frames", T, r);
      if (J > 0 && J < 100000) {  // and every j on its own
        int64_t n = 0;
        const double t = T < FS2_PVOC_J_CAP ? (double)T : (double)FS2_PVOC_J_CAP;  // a T past the cap counts as the cap
        for (int64_t j = 0; j < 100001; ++j) n += (double)j * r < t ? 1 : 0;
        if (n != J) return fail("pvoc_frames (counted)", T, r);
      }
      printf("F %lld %a -> %lld\n", (long long)T, r, (long long)J);
    }
  // a sweep of awkward quotients: T / rate lands on or next to an integer
  for (int64_t T = 1; T < 150; ++T)
    for (int64_t m = 1; m < 3 * T + 3; ++m) {
      const double r = (double)T / (double)m;  // T / r is m but for the two roundings
      const int64_t J = pvoc_frames(T, r);
      if (J != by_bisection(T, r)) return fail("pvoc_frames (sweep)", T, r);
      printf("F %lld %a -> %lld\n", (long long)T, r, (long long)J);
    }
  const int64_t sizes[] = {-1, 0, 1, 5, 513, 65535, 65536, big};
  for (int64_t B : sizes)
    for (int64_t NB : {(int64_t)0, (int64_t)1, (int64_t)513})
      for (int64_t T_max : {(int64_t)0, (int64_t)1, (int64_t)860, big})
        for (int64_t J_max : {(int64_t)0, (int64_t)1, (int64_t)1075, big})
          for (int64_t ds : {(int64_t)-1, (int64_t)0, (int64_t)7})
            for (int64_t dr : {(int64_t)-1, (int64_t)0, (int64_t)7}) {
              const int64_t ss = T_max + ds, rs = J_max + dr;
              const int rc = pvoc_check(B, NB, T_max, J_max, ss, rs);
              int want = FS2_OK;
              if (B < 1 || NB < 1 || T_max < 1 || J_max < 1 || ds < 0 || dr < 0)
                want = FS2_EINVAL;
              else if (B > FS2_PVOC_B_MAX)
                want = FS2_EUNSUPPORTED;
              if (rc != want) return fail("pvoc_check", B, (double)NB);
              printf("C %lld %lld %lld %lld %lld %lld -> %d\n", (long long)B, (long long)NB, (long long)T_max,
                     (long long)J_max, (long long)ss, (long long)rs, rc);
            }
  // the counts the host can see: rows of 10, 100 (clamped to 64), -3 (clamped to 0) frames; counts 20, 128, 0
  const int64_t frames[3] = {10, 100, -3};
  const double rs3[3] = {0.5, 0.5, 0.5};
  for (int64_t J_max : {(int64_t)1, (int64_t)19, (int64_t)20, (int64_t)127, (int64_t)128, (int64_t)129}) {
    const int rc = pvoc_check_counts(frames, 1, rs3, 3, 64, J_max);
    if (rc != (J_max >= 128 ? FS2_OK : FS2_EINVAL)) return fail("pvoc_check_counts", J_max, 0.5);
    printf("V %lld -> %d\n", (long long)J_max, rc);
  }
  if (pvoc_check_counts(nullptr, 1, rs3, 3, 64, 1) != FS2_OK || pvoc_check_counts(frames, 1, nullptr, 3, 64, 1) != FS2_OK ||
      pvoc_check_counts(nullptr, 0, rs3, 3, 64, 127) != FS2_EINVAL || pvoc_check_counts(nullptr, 0, rs3, 3, 64, 128) != FS2_OK)
    return fail("pvoc_check_counts (what the host cannot see)", 0, 0.0);
  return 0;
}
