// Corpus preprocessing after feature extraction (include/fs2hip_prep.h): phoneme-level pitch
// targets, the outlier fence with per-utterance moments, the running merge of those moments, and
// the normalisation pass with its minimum and maximum. Everything here is exact arithmetic on a
// few thousand numbers per utterance: one workgroup per utterance, no atomics, no contraction.
#include <float.h>

#include "fs2_common.h"
#include "fs2hip_prep.h"

// No a * b + c may become an FMA anywhere in this file. The operations the header names are
// written through the helpers below, defined HERE, under the pragma: HIP's __fmul_rn / __dadd_rn
// are inline functions of a header compiled with contraction allowed, and the compiler does fuse
// them (seen in the ISA as v_pk_fma_f32).
#pragma clang fp contract(off)

namespace {

constexpr int kNT = 256;  // threads per workgroup: 4 waves, one pass covers 256 frames
constexpr int kWaves = kNT / FS2_WAVE;
constexpr int kBig = 0x7fffffff;
constexpr int kPassMax = FS2_PITCH_T_MAX / kNT;

template <typename E> __device__ __forceinline__ E add_rn(E a, E b) { return a + b; }
template <typename E> __device__ __forceinline__ E sub_rn(E a, E b) { return a - b; }
template <typename E> __device__ __forceinline__ E mul_rn(E a, E b) { return a * b; }
__device__ __forceinline__ double div_rn(double a, double b) { return a / b; }  // IEEE: no fast-math here

struct OpSum {
  template <typename V> __device__ V operator()(V a, V b) const { return a + b; }
};
struct OpMin {
  __device__ int operator()(int a, int b) const { return a < b ? a : b; }
  __device__ double operator()(double a, double b) const { return fmin(a, b); }
};
struct OpMax {
  __device__ double operator()(double a, double b) const { return fmax(a, b); }
};

// Reduction over the workgroup, the result in every thread. scratch: kWaves values in LDS.
template <typename V, typename Op>
__device__ __forceinline__ V block_reduce(V v, V *scratch, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  V r = scratch[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) r = op(r, scratch[w]);
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kNT) void pitch_targets_kernel(const double *__restrict__ f0, int64_t f0_stride,
                                                            const int64_t *__restrict__ frames,
                                                            const int64_t *__restrict__ dur, int T, int L,
                                                            double *__restrict__ out, double *filled,
                                                            int *__restrict__ voiced_out) {
  // per (pass, wave): before the carry scan, the first / last voiced frame of that wave's 64
  // frames; after it, the first voiced frame of any LATER wave (nextS) and the last voiced frame
  // of any EARLIER wave (prevS)
  __shared__ int nextS[kPassMax * kWaves];
  __shared__ int prevS[kPassMax * kWaves];
  __shared__ double stageS[FS2_PITCH_T_MAX_NOFILL];  // the filled contour when it is not kept
  __shared__ long long red64S[kWaves];
  __shared__ int redS[kWaves];
  __shared__ int edgeS[2];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double *x = f0 + (int64_t)b * f0_stride;
  const int64_t *d = dur + (int64_t)b * L;
  double *fo = filled != nullptr ? filled + (int64_t)b * T : nullptr;
  double *ob = out + (int64_t)b * L;

  long long dsum = 0;
  for (int i = tid; i < L; i += kNT) dsum += d[i] > 0 ? d[i] : 0;
  dsum = block_reduce(dsum, red64S, OpSum());
  long long fr = frames != nullptr ? frames[b] : T;
  fr = fr < 0 ? 0 : (fr > T ? T : fr);
  const int n = (int)(fr < dsum ? fr : dsum);
  const int n_pass = (n + kNT - 1) / kNT;

  // wave totals of both scans, and the voiced count
  int cnt = 0;
  for (int c = 0; c < n_pass; ++c) {
    const int t = c * kNT + tid;
    const bool v = t < n && x[t] != 0.0;
    const unsigned long long m = __ballot(v);
    if (lane == 0) {
      const int base = c * kNT + wave * 64;
      nextS[c * kWaves + wave] = m ? base + __ffsll(m) - 1 : kBig;
      prevS[c * kWaves + wave] = m ? base + 63 - __clzll(m) : -1;
    }
    cnt += v ? 1 : 0;
  }
  cnt = block_reduce(cnt, redS, OpSum());  // its barriers also publish nextS / prevS
  if (tid == 0) voiced_out[b] = cnt;
  if (cnt <= 1) {  // dropped utterance (uniform branch)
    for (int i = tid; i < L; i += kNT) ob[i] = 0.0;
    if (fo != nullptr)
      for (int t = tid; t < T; t += kNT) fo[t] = 0.0;
    return;
  }
  // carries across waves and passes: exclusive min scan backward, exclusive max scan forward
  if (tid == 0) {
    int run = kBig;
    for (int k = n_pass * kWaves - 1; k >= 0; --k) {
      const int v = nextS[k];
      nextS[k] = run;
      run = v < run ? v : run;
    }
    edgeS[0] = run;
  } else if (tid == 64) {
    int run = -1;
    for (int k = 0; k < n_pass * kWaves; ++k) {
      const int v = prevS[k];
      prevS[k] = run;
      run = v > run ? v : run;
    }
    edgeS[1] = run;
  }
  __syncthreads();
  const int first = edgeS[0], last = edgeS[1];  // first < last: two voiced frames at least
  int second = kBig;
  for (int t = first + 1 + tid; t <= last; t += kNT)
    if (x[t] != 0.0) {
      second = t;
      break;
    }
  second = block_reduce(second, redS, OpMin());
  const double y_first = x[first], y_last = x[last];

  const int t_pass = fo != nullptr ? (T + kNT - 1) / kNT : n_pass;
  for (int c = 0; c < t_pass; ++c) {
    const int t = c * kNT + tid;
    double y = 0.0;
    if (c < n_pass) {  // uniform: the ballot below needs the whole wave
      const bool v = t < n && x[t] != 0.0;
      const unsigned long long m = __ballot(v);
      if (t < n) {
        if (t < first) {
          y = y_first;
        } else if (t > last) {
          y = y_last;
        } else {
          const unsigned long long below = m & ((1ull << lane) - 1ull);
          const unsigned long long above = m >> lane;
          const int base = c * kNT + wave * 64;
          const int pe = below ? base + 63 - __clzll(below) : prevS[c * kWaves + wave];  // last voiced < t
          const int nx = above ? t + __ffsll(above) - 1 : nextS[c * kWaves + wave];      // first voiced >= t
          const int hi = t == first ? second : nx;
          const int lo = t == first ? first : pe;
          const double y_lo = x[lo];
          const double slope = div_rn(sub_rn(x[hi], y_lo), (double)(hi - lo));
          y = add_rn(mul_rn(slope, (double)(t - lo)), y_lo);
        }
      }
    }
    if (fo != nullptr) {
      if (t < T) fo[t] = y;
    } else if (t < n) {
      stageS[t] = y;
    }
  }
  __syncthreads();  // the contour is read below by other threads than wrote it

  // phoneme means: each thread a contiguous run of phonemes, exclusive scan of the durations
  const double *src = fo != nullptr ? fo : stageS;
  const int per = (L + kNT - 1) / kNT;
  const int i0 = min(tid * per, L), i1 = min(i0 + per, L);
  long long local = 0;
  for (int i = i0; i < i1; ++i) local += d[i] > 0 ? d[i] : 0;
  long long incl = local;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) red64S[wave] = incl;
  __syncthreads();
  long long run = incl - local;
  for (int w = 0; w < wave; ++w) run += red64S[w];
  for (int i = i0; i < i1; ++i) {
    const long long di = d[i] > 0 ? d[i] : 0;
    const long long s0 = run < n ? run : n, s1 = run + di < n ? run + di : n;
    double s = 0.0;
    for (long long t = s0; t < s1; ++t) s = add_rn(s, src[t]);
    ob[i] = s1 > s0 ? div_rn(s, (double)(s1 - s0)) : 0.0;
    run += di;
  }
}

template <typename E>
__device__ __forceinline__ E quantile_linear(const E *sorted, int n, E q) {
  const E vi = mul_rn(q, (E)(n - 1));
  const E fl = floor(vi);
  const E g = sub_rn(vi, fl);
  int lo = (int)fl, hi = lo + 1;
  if (lo >= n - 1) lo = hi = n - 1;
  const E a = sorted[lo], bb = sorted[hi];
  const E diff = sub_rn(bb, a);
  return g >= (E)0.5 ? sub_rn(bb, mul_rn(diff, sub_rn((E)1, g))) : add_rn(a, mul_rn(diff, g));
}

template <typename E>
__global__ __launch_bounds__(kNT) void outlier_moments_kernel(const E *__restrict__ values, int64_t stride,
                                                              const int64_t *__restrict__ lens, int n_max,
                                                              E *__restrict__ quart, uint8_t *__restrict__ inlier,
                                                              int64_t *__restrict__ count, double *__restrict__ mean,
                                                              double *__restrict__ m2) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  E *s = reinterpret_cast<E *>(lds_raw);
  const int b = blockIdx.x, tid = threadIdx.x;
  const E *v = values + (int64_t)b * stride;
  uint8_t *io = inlier + (int64_t)b * n_max;
  long long nl = lens != nullptr ? lens[b] : n_max;
  const int n = (int)(nl < 0 ? 0 : (nl > n_max ? n_max : nl));
  for (int i = n + tid; i < n_max; i += kNT) io[i] = 0;
  const E nan = (E)NAN;
  if (n == 0) {
    if (tid == 0) {
      quart[2 * b] = nan;
      quart[2 * b + 1] = nan;
      count[b] = 0;
      mean[b] = 0.0;
      m2[b] = 0.0;
    }
    return;
  }
  int n_pad = 1;
  while (n_pad < n) n_pad <<= 1;
  for (int i = tid; i < n_pad; i += kNT) s[i] = i < n ? v[i] : (E)INFINITY;
  __syncthreads();
  // NaN orders after +inf, so a NaN among the values ends up in the last slot (numpy looks there too)
  for (int k = 2; k <= n_pad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n_pad; i += kNT) {
        const int p = i ^ j;
        if (p > i) {
          const E a = s[i], c = s[p];
          const bool gt = a > c || (a != a && c == c);
          if (gt == ((i & k) == 0)) {
            s[i] = c;
            s[p] = a;
          }
        }
      }
      __syncthreads();
    }
  const bool has_nan = s[n_pad - 1] != s[n_pad - 1];
  E p25 = quantile_linear(s, n, (E)0.25), p75 = quantile_linear(s, n, (E)0.75);
  if (has_nan) p25 = p75 = nan;
  __syncthreads();  // the sorted copy is not read again: its LDS now holds the partial sums
  const E w = mul_rn((E)1.5, sub_rn(p75, p25));
  const E lower = sub_rn(p25, w), upper = add_rn(p75, w);
  double *sumS = reinterpret_cast<double *>(lds_raw);
  int *cntS = reinterpret_cast<int *>(lds_raw + kNT * sizeof(double));
  const int per = (n + kNT - 1) / kNT;
  const int i0 = min(tid * per, n), i1 = min(i0 + per, n);
  double sum = 0.0;
  int c = 0;
  for (int i = i0; i < i1; ++i) {
    const E e = v[i];
    const bool in = e > lower && e < upper;
    io[i] = in ? 1 : 0;
    if (in) {
      sum = add_rn(sum, (double)e);
      ++c;
    }
  }
  sumS[tid] = sum;
  cntS[tid] = c;
  __syncthreads();
  double tot = 0.0;
  int ctot = 0;
  for (int k = 0; k < kNT; ++k) {  // every thread the same order: the same mean in all of them
    tot = add_rn(tot, sumS[k]);
    ctot += cntS[k];
  }
  const double mu = ctot > 0 ? div_rn(tot, (double)ctot) : 0.0;
  __syncthreads();
  double acc = 0.0;
  for (int i = i0; i < i1; ++i) {
    const E e = v[i];
    if (e > lower && e < upper) {
      const double dv = sub_rn((double)e, mu);
      acc = add_rn(acc, mul_rn(dv, dv));
    }
  }
  sumS[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    double t2 = 0.0;
    for (int k = 0; k < kNT; ++k) t2 = add_rn(t2, sumS[k]);
    quart[2 * b] = p25;
    quart[2 * b + 1] = p75;
    count[b] = ctot;
    mean[b] = mu;
    m2[b] = ctot > 0 ? t2 : 0.0;
  }
}

// One wave: 64 partials at a time into LDS, lane 0 folds them in index order.
__global__ __launch_bounds__(64) void moments_merge_kernel(const int64_t *__restrict__ count,
                                                           const double *__restrict__ mean,
                                                           const double *__restrict__ m2, int B,
                                                           double *__restrict__ state) {
  __shared__ double cS[64], meanS[64], m2S[64];
  const int lane = threadIdx.x;
  double na = 0.0, ma = 0.0, qa = 0.0;
  if (lane == 0) {
    na = state[0];
    ma = state[1];
    qa = state[2];
  }
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int b = b0 + lane;
    cS[lane] = b < B ? (double)count[b] : 0.0;
    meanS[lane] = b < B ? mean[b] : 0.0;
    m2S[lane] = b < B ? m2[b] : 0.0;
    __syncthreads();
    if (lane == 0) {
      const int m = min(64, B - b0);
      for (int k = 0; k < m; ++k) {
        const double nb = cS[k];
        if (!(nb > 0.0)) continue;
        if (!(na > 0.0)) {
          na = nb;
          ma = meanS[k];
          qa = m2S[k];
          continue;
        }
        const double nn = add_rn(na, nb);
        const double delta = sub_rn(meanS[k], ma);
        ma = add_rn(ma, mul_rn(delta, div_rn(nb, nn)));
        qa = add_rn(add_rn(qa, m2S[k]), mul_rn(mul_rn(delta, delta), div_rn(mul_rn(na, nb), nn)));
        na = nn;
      }
    }
    __syncthreads();
  }
  if (lane == 0) {
    state[0] = na;
    state[1] = ma;
    state[2] = qa;
  }
}

template <typename E>
__global__ __launch_bounds__(kNT) void normalize_kernel(const E *__restrict__ values, int64_t stride,
                                                        const int64_t *__restrict__ lens, int n_max, double mean,
                                                        double std, double *__restrict__ out,
                                                        double *__restrict__ part) {
  __shared__ double redS[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const E *v = values + (int64_t)b * stride;
  double *o = out + (int64_t)b * n_max;
  long long nl = lens != nullptr ? lens[b] : n_max;
  const int n = (int)(nl < 0 ? 0 : (nl > n_max ? n_max : nl));
  double mn = DBL_MAX, mx = -DBL_MAX;
  for (int i = tid; i < n_max; i += kNT) {
    double y = 0.0;
    if (i < n) {
      y = div_rn(sub_rn((double)v[i], mean), std);
      mn = fmin(mn, y);
      mx = fmax(mx, y);
    }
    o[i] = y;
  }
  mn = block_reduce(mn, redS, OpMin());
  mx = block_reduce(mx, redS, OpMax());
  if (tid == 0) {
    part[2 * b] = mn;
    part[2 * b + 1] = mx;
  }
}

__global__ __launch_bounds__(kNT) void minmax_finish_kernel(const double *__restrict__ part, int B,
                                                            double *__restrict__ minmax) {
  __shared__ double redS[kWaves];
  double mn = DBL_MAX, mx = -DBL_MAX;
  for (int b = threadIdx.x; b < B; b += kNT) {
    mn = fmin(mn, part[2 * b]);
    mx = fmax(mx, part[2 * b + 1]);
  }
  mn = block_reduce(mn, redS, OpMin());
  mx = block_reduce(mx, redS, OpMax());
  if (threadIdx.x == 0) {
    minmax[0] = mn;
    minmax[1] = mx;
  }
}

}  // namespace

extern "C" int fs2_pitch_targets(const double *f0, int64_t f0_row_stride, const int64_t *frames, const int64_t *dur,
                                 int B, int T, int L, double *out, double *filled, int32_t *voiced,
                                 fs2_stream_t stream) {
  if (f0 == nullptr || dur == nullptr || out == nullptr || voiced == nullptr) return FS2_EINVAL;
  if (B < 1 || T < 1 || L < 1 || f0_row_stride < T) return FS2_EINVAL;
  if (T > FS2_PITCH_T_MAX || (filled == nullptr && T > FS2_PITCH_T_MAX_NOFILL) || B > 65535) return FS2_EUNSUPPORTED;
  hipLaunchKernelGGL(pitch_targets_kernel, dim3(B), dim3(kNT), 0, as_stream(stream), f0, f0_row_stride, frames, dur, T,
                     L, out, filled, voiced);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_outlier_moments(const void *values, int dtype, int64_t row_stride, const int64_t *lens, int B,
                                   int n_max, void *quartiles, uint8_t *inlier, int64_t *count, double *mean,
                                   double *m2, fs2_stream_t stream) {
  if (values == nullptr || quartiles == nullptr || inlier == nullptr || count == nullptr || mean == nullptr ||
      m2 == nullptr)
    return FS2_EINVAL;
  if (B < 1 || n_max < 1 || row_stride < n_max) return FS2_EINVAL;
  if (dtype != FS2_F32 && dtype != FS2_F64) return FS2_EUNSUPPORTED;
  const int64_t esize = dtype == FS2_F64 ? 8 : 4;
  if ((int64_t)n_max * esize > FS2_OUTLIER_LDS_BYTES || B > 65535) return FS2_EUNSUPPORTED;
  int n_pad = 1;
  while (n_pad < n_max) n_pad <<= 1;
  // the sort buffer, and at least the 256 partial sums and counts that follow it in the same LDS
  size_t lds = (size_t)n_pad * esize;
  if (lds < kNT * (sizeof(double) + sizeof(int))) lds = kNT * (sizeof(double) + sizeof(int));
  if (dtype == FS2_F64)
    hipLaunchKernelGGL(outlier_moments_kernel<double>, dim3(B), dim3(kNT), lds, as_stream(stream),
                       static_cast<const double *>(values), row_stride, lens, n_max, static_cast<double *>(quartiles),
                       inlier, count, mean, m2);
  else
    hipLaunchKernelGGL(outlier_moments_kernel<float>, dim3(B), dim3(kNT), lds, as_stream(stream),
                       static_cast<const float *>(values), row_stride, lens, n_max, static_cast<float *>(quartiles),
                       inlier, count, mean, m2);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_moments_merge(const int64_t *count, const double *mean, const double *m2, int B, double *state,
                                 fs2_stream_t stream) {
  if (count == nullptr || mean == nullptr || m2 == nullptr || state == nullptr || B < 1) return FS2_EINVAL;
  hipLaunchKernelGGL(moments_merge_kernel, dim3(1), dim3(64), 0, as_stream(stream), count, mean, m2, B, state);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int64_t fs2_normalize_minmax_ws_bytes(int B) { return B < 1 ? 0 : (int64_t)B * 2 * sizeof(double); }

extern "C" int fs2_normalize_minmax(const void *values, int dtype, int64_t row_stride, const int64_t *lens, int B,
                                    int n_max, double mean, double std, double *out, double *minmax, void *ws,
                                    int64_t ws_bytes, fs2_stream_t stream) {
  if (values == nullptr || out == nullptr || minmax == nullptr || ws == nullptr) return FS2_EINVAL;
  if (B < 1 || n_max < 1 || row_stride < n_max || ws_bytes < fs2_normalize_minmax_ws_bytes(B)) return FS2_EINVAL;
  if (dtype != FS2_F32 && dtype != FS2_F64) return FS2_EUNSUPPORTED;
  if (B > 65535) return FS2_EUNSUPPORTED;
  double *part = static_cast<double *>(ws);
  hipStream_t s = as_stream(stream);
  if (dtype == FS2_F64)
    hipLaunchKernelGGL(normalize_kernel<double>, dim3(B), dim3(kNT), 0, s, static_cast<const double *>(values),
                       row_stride, lens, n_max, mean, std, out, part);
  else
    hipLaunchKernelGGL(normalize_kernel<float>, dim3(B), dim3(kNT), 0, s, static_cast<const float *>(values),
                       row_stride, lens, n_max, mean, std, out, part);
  FS2_CHECK_LAUNCH();
  hipLaunchKernelGGL(minmax_finish_kernel, dim3(1), dim3(kNT), 0, s, part, B, minmax);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}
