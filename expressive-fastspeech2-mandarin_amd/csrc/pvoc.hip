// The phase vocoder (include/fs2hip_pvoc.h): a spectrum resampled along time with a running phase per
// bin, the phase kept as a running product of unit rotors in float64. A wave owns one (row, bin) and
// walks the output in blocks of 64 frames, a lane per frame: the two input frames of a lane are read
// straight from the bin's row (neighbouring lanes read neighbouring or equal columns), the prefix
// product inside a block is six rounds of shuffles, the carry into the next block is lane 63.
#include "fs2_common.h"
#include "pvoc_sizes.h"

// No a * b + c may become an FMA anywhere in this file (csrc/prep.hip explains why the helpers are
// defined under the pragma).
#pragma clang fp contract(off)

namespace {

constexpr int kWaves = 4;  // bins per workgroup
constexpr int kNT = kWaves * FS2_WAVE;
static_assert(FS2_PVOC_BLOCK == FS2_WAVE, "a block of the scan is one wave");

__device__ __forceinline__ double add_rn(double a, double b) { return a + b; }
__device__ __forceinline__ double sub_rn(double a, double b) { return a - b; }
__device__ __forceinline__ double mul_rn(double a, double b) { return a * b; }
__device__ __forceinline__ double div_rn(double a, double b) { return a / b; }

struct Cx {
  double x, y;
};

// (x, y) (*) (u, v) = (x u - y v, x v + y u), each product and sum rounded on its own
__device__ __forceinline__ Cx cmul(Cx a, Cx b) {
  return {sub_rn(mul_rn(a.x, b.x), mul_rn(a.y, b.y)), add_rn(mul_rn(a.x, b.y), mul_rn(a.y, b.x))};
}

// m and e of the header's rule 2 for one input frame; i == T is the zero pad
__device__ __forceinline__ void unit(const float *__restrict__ re_row, const float *__restrict__ im_row, int i, int T,
                                     double &m, Cx &e) {
  m = 0.0;
  e = {1.0, 0.0};
  if (i < T) {
    const double re = (double)re_row[i], im = (double)im_row[i];
    m = sqrt(add_rn(mul_rn(re, re), mul_rn(im, im)));
    if (m != 0.0) e = {div_rn(re, m), div_rn(im, m)};
  }
}

struct PvocArgs {
  const float *spec;
  int64_t spec_rs;
  const int64_t *frames;
  const double *rates;
  int NB, T_max, J_max;
  float *recomb;
  int64_t recomb_rs;
  int64_t *frames_out;
};

__global__ __launch_bounds__(kNT) void pvoc_kernel(PvocArgs A) {
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int k = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (k >= A.NB) return;  // whole waves; no barrier below
  const int T = (int)pvoc_clamp_frames(A.frames != nullptr ? A.frames[b] : A.T_max, A.T_max);
  const double rate = A.rates[b];
  const int64_t J = pvoc_frames(T, rate);
  if (k == 0 && lane == 0 && A.frames_out != nullptr) A.frames_out[b] = J;
  const int Jw = J < A.J_max ? (int)J : A.J_max;  // the columns that hold a value
  const float *re_row = A.spec + ((int64_t)b * 2 * A.NB + k) * A.spec_rs;
  const float *im_row = re_row + (int64_t)A.NB * A.spec_rs;
  float *out_re = A.recomb + ((int64_t)b * 2 * A.NB + k) * A.recomb_rs;
  float *out_im = out_re + (int64_t)A.NB * A.recomb_rs;

  Cx carry = {1.0, 0.0}, prev_rotor = {1.0, 0.0};  // P and the rotor of the frame before this block
  for (int64_t j0 = 0; j0 < A.J_max; j0 += FS2_PVOC_BLOCK) {  // 64 bits: J_max may be close to 2^31
    const int64_t j = j0 + lane;
    if (j0 >= Jw) {  // uniform: the zero tail
      if (j < A.J_max) {
        out_re[j] = 0.0f;
        out_im[j] = 0.0f;
      }
      continue;
    }
    // lanes at or past Jw take part in the shuffles with a harmless value: a lane's prefix only
    // depends on the lanes below it
    double mag = 0.0;
    Cx rotor = {1.0, 0.0};
    if (j < Jw) {
      const double p = mul_rn((double)j, rate);
      const int i = (int)p;  // 0 <= p < T: truncation is floor
      const double alpha = sub_rn(p, (double)i);
      double m0, m1;
      Cx e0, e1;
      unit(re_row, im_row, i, T, m0, e0);
      unit(re_row, im_row, i + 1, T, m1, e1);
      mag = add_rn(mul_rn(sub_rn(1.0, alpha), m0), mul_rn(alpha, m1));
      rotor = {add_rn(mul_rn(e1.x, e0.x), mul_rn(e1.y, e0.y)), sub_rn(mul_rn(e1.y, e0.x), mul_rn(e1.x, e0.y))};
      if (j == 0) prev_rotor = e0;  // s_0 = e[0]
    }
    // s_j = rotor_{j - 1}: one lane up; lane 0 takes the last rotor of the block before (e[0] at j = 0)
    Cx s = {__shfl_up(rotor.x, 1, 64), __shfl_up(rotor.y, 1, 64)};
    if (lane == 0) s = prev_rotor;
    prev_rotor = {__shfl(rotor.x, 63, 64), __shfl(rotor.y, 63, 64)};
#pragma unroll
    for (int d = 1; d < FS2_PVOC_BLOCK; d <<= 1) {
      const Cx lo = {__shfl_up(s.x, d, 64), __shfl_up(s.y, d, 64)};
      if (lane >= d) s = cmul(lo, s);
    }
    if (j0 > 0) s = cmul(carry, s);
    carry = {__shfl(s.x, 63, 64), __shfl(s.y, 63, 64)};
    if (j < A.J_max) {
      const bool live = j < Jw;
      out_re[j] = live ? (float)mul_rn(mag, s.x) : 0.0f;
      out_im[j] = live ? (float)mul_rn(mag, s.y) : 0.0f;
    }
  }
}

}  // namespace

extern "C" int64_t fs2_pvoc_frames(int64_t T, double rate) { return pvoc_frames(T, rate); }

extern "C" int fs2_phase_vocoder(const fs2_pvoc_desc *d, fs2_stream_t stream) {
  if (d == nullptr || d->spec == nullptr || d->rates == nullptr || d->recomb == nullptr) return FS2_EINVAL;
  int rc = pvoc_check(d->B, d->NB, d->T_max, d->J_max, d->spec_row_stride, d->recomb_row_stride);
  if (rc != FS2_OK) return rc;
  rc = pvoc_check_counts(d->frames_host, d->frames != nullptr, d->rates_host, d->B, d->T_max, d->J_max);
  if (rc != FS2_OK) return rc;
  PvocArgs a;
  a.spec = d->spec;
  a.spec_rs = d->spec_row_stride;
  a.frames = d->frames;
  a.rates = d->rates;
  a.NB = d->NB;
  a.T_max = d->T_max;
  a.J_max = d->J_max;
  a.recomb = d->recomb;
  a.recomb_rs = d->recomb_row_stride;
  a.frames_out = d->frames_out;
  const dim3 grid((unsigned)((d->NB + kWaves - 1) / kWaves), (unsigned)d->B);
  hipLaunchKernelGGL(pvoc_kernel, grid, dim3(kNT), 0, as_stream(stream), a);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}
