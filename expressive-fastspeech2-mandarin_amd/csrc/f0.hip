// F0 contours from waveforms (include/fs2hip_f0.h): YIN in float64. One workgroup per utterance
// and group of FS2_F0_GROUP frames: the group's samples staged once in LDS, the squared differences
// summed per hop-sized block (shared by the frames over it) with 8 lags per thread in registers,
// then per frame the table d -> cum -> dp in LDS and the pick by one wave. No atomics.
#include "f0_sizes.h"
#include "fs2_common.h"
#include "fs2hip_audio.h"
#include "fs2hip_f0.h"

// Nothing here may be contracted: the one fused operation the header allows, the square inside the
// accumulation of d, is written as an explicit fma.
#pragma clang fp contract(off)

namespace {

constexpr int kNT = 256;  // threads per workgroup: 4 waves
constexpr int kG = FS2_F0_GROUP;
constexpr int kLags = FS2_F0_LAGS;  // consecutive lags per thread

struct F0Args {
  int64_t stride;
  const int64_t *lens;
  int n_max, hop, W, tau_min, tau_max, F_max;
  double sr, thr, f0_floor, f0_ceil;
  double *f0;
  int *tau;
  double *cmnd;
};

// Index of sample p inside the staged span: one f64 of padding after every 8, so that the lanes of
// a wave, whose lag windows start 8 samples apart, read 16 distinct bank pairs, not 4.
__device__ __forceinline__ int sw(int p) { return p + (p >> 3); }

template <typename T>
__global__ __launch_bounds__(kNT) void f0_yin_kernel(const T *__restrict__ wav, F0Args A) {
  extern __shared__ __align__(16) double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, k0 = blockIdx.x * kG;
  const int hop = A.hop, W = A.W, tau_max = A.tau_max;
  const int n_oct = (tau_max + kLags - 1) / kLags, tau_pad = n_oct * kLags, ts = tau_pad + 1;
  double *X = lds;                             // the span; after the block sums, the tables [kG][ts]
  double *P = lds + (int)f0_sizes(hop, W, tau_max).first;  // block sums [segs][ts]; later cum [kG][ts]

  long long nl = A.lens != nullptr ? A.lens[b] : A.n_max;
  const int n = (int)(nl < 0 ? 0 : (nl > A.n_max ? A.n_max : nl));
  const int F_b = n / hop + 1;
  const int ng = min(kG, A.F_max - k0);               // frames this group writes
  const int nv = max(0, min(ng, F_b - k0));           // of them, frames of the utterance
  const int64_t row = (int64_t)b * A.F_max + k0;
  double *f0o = A.f0 + row;
  int *tauo = A.tau != nullptr ? A.tau + row : nullptr;
  double *cm = A.cmnd != nullptr ? A.cmnd + row * (tau_max + 1) : nullptr;

  // frames past F_b: zeros
  for (int i = nv + tid; i < ng; i += kNT) {
    f0o[i] = 0.0;
    if (tauo != nullptr) tauo[i] = 0;
  }
  if (cm != nullptr)
    for (int e = nv * (tau_max + 1) + tid; e < ng * (tau_max + 1); e += kNT) cm[e] = 0.0;
  if (nv == 0) return;  // uniform

  // stage the span: sample s0 + p at X[sw(p)], 0 outside [0, n)
  const int q = W / hop, r = W - q * hop;
  const int span = (nv - 1) * hop + W + tau_pad;
  const long long s0 = (long long)k0 * hop - (W + tau_max) / 2;
  const T *x = wav + (int64_t)b * A.stride;
  for (int p = tid; p < span; p += kNT) {
    const long long g = s0 + p;
    X[sw(p)] = g >= 0 && g < n ? (double)x[g] : 0.0;
  }
  __syncthreads();

  // block sums: segment seg < n_blk is the hop block [seg * hop, (seg + 1) * hop) of the span,
  // shared by the frames seg - q + 1 .. seg; segment n_blk + i is frame i's own tail
  // [(i + q) * hop, i * hop + W) when hop does not divide W
  const int n_blk = q > 0 ? nv + q - 1 : 0;
  const int n_seg = n_blk + (r > 0 ? nv : 0);
  const int n_items = n_seg * n_oct;
  for (int it = tid; it < n_items; it += kNT) {
    const int seg = it / n_oct, o = it - seg * n_oct;
    const int a = seg < n_blk ? seg * hop : (seg - n_blk + q) * hop;
    const int len = seg < n_blk ? hop : r;
    const int y0 = a + 1 + kLags * o;  // the sample lag tau0 = 1 + 8 o pairs with sample a
    double acc[kLags], ring[kLags];
#pragma unroll
    for (int i = 0; i < kLags; ++i) acc[i] = 0.0;
#pragma unroll
    for (int i = 0; i < kLags - 1; ++i) ring[i] = X[sw(y0 + i)];
    int s = 0;
    // step s pairs sample a + s with the samples y0 + s + i, kept at ring[(s + i) % 8]: one new
    // sample and one (broadcast) x per 8 terms
    for (; s + kLags <= len; s += kLags) {
#pragma unroll
      for (int u = 0; u < kLags; ++u) {
        ring[(u + kLags - 1) & (kLags - 1)] = X[sw(y0 + s + u + kLags - 1)];
        const double xv = X[sw(a + s + u)];
#pragma unroll
        for (int i = 0; i < kLags; ++i) {
          const double dd = xv - ring[(u + i) & (kLags - 1)];
          acc[i] = __builtin_fma(dd, dd, acc[i]);
        }
      }
    }
    for (; s < len; ++s) {
      const double xv = X[sw(a + s)];
#pragma unroll
      for (int i = 0; i < kLags; ++i) {
        const double dd = xv - X[sw(y0 + s + i)];
        acc[i] = __builtin_fma(dd, dd, acc[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < kLags; ++i) P[seg * ts + 1 + kLags * o + i] = acc[i];
  }
  __syncthreads();  // the span is dead: its LDS now holds the tables

  // d of frame i: its q blocks in order, then its tail
  double *D = X;
  for (int e = tid; e < nv * ts; e += kNT) {
    const int i = e / ts, t = e - i * ts;
    double d = 0.0;
    if (t >= 1) {
      for (int m = 0; m < q; ++m) d = d + P[(i + m) * ts + t];
      if (r > 0) d = d + P[(n_blk + i) * ts + t];
    }
    D[e] = d;
  }
  __syncthreads();  // the block sums are dead: their LDS now holds cum

  // cum, left to right: one thread per frame, two frames per wave
  double *C = P;
  if ((tid & 31) == 0 && (tid >> 5) < nv) {
    const int i = tid >> 5;
    double c = 0.0;
#pragma unroll 8
    for (int t = 1; t <= tau_max; ++t) {
      c = c + D[i * ts + t];
      C[i * ts + t] = c;
    }
  }
  __syncthreads();

  for (int e = tid; e < nv * (tau_max + 1); e += kNT) {
    const int i = e / (tau_max + 1), t = e - i * (tau_max + 1);
    double dp = 1.0;
    if (t >= 1) {
      const double c = C[i * ts + t];
      if (!(c == 0.0)) dp = (D[i * ts + t] * (double)t) / c;
    }
    D[i * ts + t] = dp;
    if (cm != nullptr) cm[e] = dp;
  }
  __syncthreads();

  // the pick: wave w takes frames w, w + 4
  for (int i = wave; i < nv; i += kNT / FS2_WAVE) {
    const double *dp = D + i * ts;
    int first = -1;
    for (int base = A.tau_min; base < tau_max; base += FS2_WAVE) {
      const int t = base + lane;
      const unsigned long long m = __ballot(t < tau_max && dp[t] < A.thr);
      if (m) {
        first = base + __ffsll(m) - 1;
        break;
      }
    }
    int tau = 0;
    double f0 = 0.0;
    if (first >= 0) {  // uniform
      for (int base = first;; base += FS2_WAVE) {  // t = tau_max - 1 always stops
        const int t = base + lane;
        const bool stop = t < tau_max && !(t + 1 < tau_max && dp[t + 1] < dp[t]);
        const unsigned long long m = __ballot(stop);
        if (m) {
          tau = base + __ffsll(m) - 1;
          break;
        }
      }
      const double a = dp[tau - 1], bb = dp[tau], c = dp[tau + 1];
      const double den = (a - 2.0 * bb) + c;
      const double delta = den > 0.0 ? (0.5 * (a - c)) / den : 0.0;
      const double f = A.sr / ((double)tau + delta);
      if (A.f0_floor <= f && f <= A.f0_ceil)
        f0 = f;
      else
        tau = 0;
    }
    if (lane == 0) {
      f0o[i] = f0;
      if (tauo != nullptr) tauo[i] = tau;
    }
  }
}

}  // namespace

extern "C" int64_t fs2_f0_lds_bytes(int hop, int W, int tau_max) {
  return hop < 1 || W < 1 || tau_max < 1 ? 0 : f0_sizes(hop, W, tau_max).bytes;
}

extern "C" int fs2_f0_yin(const void *wav, int dtype, int64_t row_stride, const int64_t *lens, int B, int n_max,
                          double sr, int hop, int W, int tau_min, int tau_max, double thr, double f0_floor,
                          double f0_ceil, double *f0, int32_t *tau, double *cmnd, fs2_stream_t stream) {
  if (wav == nullptr || f0 == nullptr) return FS2_EINVAL;
  if (B < 1 || n_max < 1 || hop < 1 || W < 1 || row_stride < n_max) return FS2_EINVAL;
  if (tau_min < 2 || tau_min >= tau_max) return FS2_EINVAL;
  if (dtype != FS2_I16 && dtype != FS2_F32) return FS2_EUNSUPPORTED;
  if (B > 65535) return FS2_EUNSUPPORTED;
  const int64_t lds = f0_sizes(hop, W, tau_max).bytes;  // the LDS the launch needs, as the header states it
  if (lds > FS2_F0_LDS_BYTES) return FS2_EUNSUPPORTED;
  F0Args a;
  a.stride = row_stride;
  a.lens = lens;
  a.n_max = n_max;
  a.hop = hop;
  a.W = W;
  a.tau_min = tau_min;
  a.tau_max = tau_max;
  a.F_max = n_max / hop + 1;
  a.sr = sr;
  a.thr = thr;
  a.f0_floor = f0_floor;
  a.f0_ceil = f0_ceil;
  a.f0 = f0;
  a.tau = tau;
  a.cmnd = cmnd;
  const dim3 grid((a.F_max + kG - 1) / kG, B);
  if (dtype == FS2_I16)
    hipLaunchKernelGGL(f0_yin_kernel<int16_t>, grid, dim3(kNT), (size_t)lds, as_stream(stream),
                       static_cast<const int16_t *>(wav), a);
  else
    hipLaunchKernelGGL(f0_yin_kernel<float>, grid, dim3(kNT), (size_t)lds, as_stream(stream),
                       static_cast<const float *>(wav), a);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}
