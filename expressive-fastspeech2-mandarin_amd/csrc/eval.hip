// Objective evaluation (include/fs2hip_eval.h): mel cepstra, pairwise distances, dynamic time warping
// and statistics along the warping path, float64. The DTW is sequential over anti-diagonals and
// parallel within one: one workgroup per utterance at a time (persistent workgroups walk the batch),
// three anti-diagonals rotating in LDS, one barrier per anti-diagonal, the next one's costs computed
// before that barrier. The costs are computed where they are used, never materialised.
#include "eval_sizes.h"
#include "fs2_common.h"
#include "fs2hip_prep.h"

// Nothing here may be contracted: every operation the header names is one IEEE operation.
#pragma clang fp contract(off)

namespace {

constexpr int kNT = 256;  // threads per workgroup: 4 waves
constexpr int kPF = 2;    // chunks of kNT cells whose costs are computed an anti-diagonal ahead

__device__ __forceinline__ double pos_inf() { return __builtin_inf(); }

__device__ __forceinline__ int clamp_len(const int64_t *lens, int b, int n_max) {
  const int64_t nl = lens != nullptr ? lens[b] : n_max;
  return (int)(nl < 0 ? 0 : (nl > n_max ? n_max : nl));
}

// The cost of fs2_pair_dist and of fs2_dtw: the one place where it is computed.
// N terms of the sum, in index order, their 2 N loads issued together: a loop of one term at a time
// waits for one load round trip per term (13 in a row at D = 13), and the DTW pays that on every
// anti-diagonal.
template <typename T, int N>
__device__ __forceinline__ double ev_sq_terms(const T *__restrict__ xi, const T *__restrict__ yj, double s) {
  T xv[N], yv[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    xv[k] = xi[k];
    yv[k] = yj[k];
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double e = (double)xv[k] - (double)yv[k];
    s = s + e * e;
  }
  return s;
}

template <typename T>
__device__ __forceinline__ double ev_sq_dist(const T *__restrict__ xi, const T *__restrict__ yj, int D) {
  double s = 0.0;
  int d = 0;
  for (; d + 8 <= D; d += 8) s = ev_sq_terms<T, 8>(xi + d, yj + d, s);
  if (d + 4 <= D) {
    s = ev_sq_terms<T, 4>(xi + d, yj + d, s);
    d += 4;
  }
  for (; d < D; ++d) s = ev_sq_terms<T, 1>(xi + d, yj + d, s);
  return s;
}
template <typename T>
__device__ __forceinline__ double ev_pair_cost(const T *__restrict__ xi, const T *__restrict__ yj, int D) {
  return sqrt(ev_sq_dist<T>(xi, yj, D));
}

// ------------------------------------------------------------------------------------------------
// mel cepstrum: one thread per output

template <typename T>
__global__ __launch_bounds__(kNT) void mel_cepstrum_kernel(const T *__restrict__ mel, int64_t bs, int64_t rs,
                                                           const int64_t *__restrict__ lens,
                                                           const double *__restrict__ basis, int B, int T_max, int M,
                                                           int C, double *__restrict__ out) {
  const int64_t n = (int64_t)B * T_max * C;
  for (int64_t o = (int64_t)blockIdx.x * kNT + threadIdx.x; o < n; o += (int64_t)gridDim.x * kNT) {
    const int q = (int)(o % C);
    const int64_t bt = o / C;
    const int t = (int)(bt % T_max), b = (int)(bt / T_max);
    double s = 0.0;
    if (t < clamp_len(lens, b, T_max)) {
      const T *row = mel + (int64_t)b * bs + (int64_t)t * rs;
      const double *w = basis + (int64_t)q * M;
      for (int m = 0; m < M; ++m) s = s + (double)row[m] * w[m];
    }
    out[o] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// pairwise distances: one thread per output, j fastest

struct PairArgs {
  int64_t xbs, xrs, ybs, yrs;
  const int64_t *x_lens, *y_lens;
  int B, Tx_max, Ty_max, D, squared;
};

template <typename T>
__global__ __launch_bounds__(kNT) void pair_dist_kernel(const T *__restrict__ x, const T *__restrict__ y, PairArgs A,
                                                        double *__restrict__ out) {
  const int64_t n = (int64_t)A.B * A.Tx_max * A.Ty_max;
  for (int64_t o = (int64_t)blockIdx.x * kNT + threadIdx.x; o < n; o += (int64_t)gridDim.x * kNT) {
    const int j = (int)(o % A.Ty_max);
    const int64_t bi = o / A.Ty_max;
    const int i = (int)(bi % A.Tx_max), b = (int)(bi / A.Tx_max);
    double c = 0.0;
    if (i < clamp_len(A.x_lens, b, A.Tx_max) && j < clamp_len(A.y_lens, b, A.Ty_max)) {
      const T *xi = x + (int64_t)b * A.xbs + (int64_t)i * A.xrs, *yj = y + (int64_t)b * A.ybs + (int64_t)j * A.yrs;
      c = A.squared ? ev_sq_dist<T>(xi, yj, A.D) : ev_pair_cost<T>(xi, yj, A.D);
    }
    out[o] = c;
  }
}

// ------------------------------------------------------------------------------------------------
// dynamic time warping

struct DtwArgs {
  int64_t xbs, xrs, ybs, yrs;
  const int64_t *x_lens, *y_lens;
  int B, Tx_max, Ty_max, D, in_lds;
  unsigned long long *ws;
  double *total;
  int *K, *path_i, *path_j;
};

// first and last i of anti-diagonal e, and the first i of the 64-cell word that holds the first
__device__ __forceinline__ void dtw_span(int e, int Tx, int Ty, int &lo, int &hi, int &i0) {
  lo = e - (Ty - 1) > 0 ? e - (Ty - 1) : 0;
  hi = e < Tx - 1 ? e : Tx - 1;
  i0 = lo & ~(FS2_WAVE - 1);
}

// the cost of cell i = i0 + c * kNT + tid of anti-diagonal e (0 for an idle thread)
template <typename T>
__device__ __forceinline__ double dtw_cost(const T *x, const T *y, const DtwArgs &A, int e, int c, int Tx, int Ty) {
  int lo, hi, i0;
  dtw_span(e, Tx, Ty, lo, hi, i0);
  const int i = i0 + c * kNT + (int)threadIdx.x;
  if (i < lo || i > hi) return 0.0;
  return ev_pair_cost<T>(x + (int64_t)i * A.xrs, y + (int64_t)(e - i) * A.yrs, A.D);
}

// One cell of anti-diagonal e. Every lane of the wave calls it: the steps of 64 neighbouring cells
// leave as two ballot words. p1: anti-diagonal e - 1, p2: e - 2; slot 1 + i holds cell (i, . - i).
__device__ __forceinline__ void dtw_cell(double cost, int i, int lo, int hi, const double *p2, const double *p1,
                                         double *cur, unsigned long long *bits_row) {
  const bool in = i >= lo && i <= hi;
  const double p = in ? p2[i] : 0.0, u = in ? p1[i] : 0.0, l = in ? p1[i + 1] : 0.0;
  const int step = (p <= u && p <= l) ? 0 : (u <= l ? 1 : 2);
  if (in) {
    cur[1 + i] = cost + (step == 0 ? p : (step == 1 ? u : l));
    if (i == hi) cur[2 + i] = pos_inf();  // the missing neighbour of the next two anti-diagonals
  }
  const unsigned long long m1 = __ballot(in && step == 1), m2 = __ballot(in && step == 2);
  const int iw = i & ~(FS2_WAVE - 1);  // the wave's first cell: i0 and kNT are multiples of 64
  if ((threadIdx.x & (FS2_WAVE - 1)) == 0 && iw <= hi) {
    bits_row[(iw >> 6) * 2] = m1;
    bits_row[(iw >> 6) * 2 + 1] = m2;
  }
}

template <typename T, int kBytes>
__global__ __launch_bounds__(kNT) void dtw_kernel(const T *__restrict__ xall, const T *__restrict__ yall, DtwArgs A) {
  __shared__ __align__(16) double lds[kBytes / 8];
  const int tid = threadIdx.x;
  const int rsz = (int)ev_dtw_row(A.Tx_max), W = (int)ev_words(A.Tx_max);
  const int P = A.Tx_max + A.Ty_max - 1;
  const int64_t bwords = ev_dtw_bitmap_words(A.Tx_max, A.Ty_max);
  unsigned long long *lbits = reinterpret_cast<unsigned long long *>(lds + 3 * rsz);
  for (int b = blockIdx.x; b < A.B; b += gridDim.x) {  // uniform
    const int Tx = clamp_len(A.x_lens, b, A.Tx_max), Ty = clamp_len(A.y_lens, b, A.Ty_max);
    int *pi = A.path_i + (int64_t)b * P, *pj = A.path_j + (int64_t)b * P;
    if (Tx == 0 || Ty == 0) {  // uniform
      for (int k = tid; k < P; k += kNT) pi[k] = pj[k] = -1;
      if (tid == 0) {
        A.total[b] = pos_inf();
        A.K[b] = 0;
      }
      continue;
    }
    unsigned long long *bits = A.in_lds ? lbits : A.ws + (int64_t)b * bwords;
    const T *x = xall + (int64_t)b * A.xbs, *y = yall + (int64_t)b * A.ybs;
    const int E = Tx + Ty - 1;  // anti-diagonals
    double cn[kPF];
#pragma unroll
    for (int k = 0; k < kPF; ++k) cn[k] = E > 1 ? dtw_cost<T>(x, y, A, 1, k, Tx, Ty) : 0.0;
    __syncthreads();  // the previous utterance's backtrack is done with the rows and the bitmap
    if (tid == 0) {   // anti-diagonal 0 in row 0; what anti-diagonals 1 and 2 find beside and before it
      lds[0] = lds[rsz] = lds[2 * rsz] = pos_inf();
      lds[1] = ev_pair_cost<T>(x, y, A.D);
      lds[2] = pos_inf();
      lds[2 * rsz + 1] = pos_inf();
    }
    int m = 1;  // e % 3
    for (int e = 1; e < E; ++e) {
      double cc[kPF];
#pragma unroll
      for (int k = 0; k < kPF; ++k) {
        cc[k] = cn[k];
        cn[k] = e + 1 < E ? dtw_cost<T>(x, y, A, e + 1, k, Tx, Ty) : 0.0;
      }
      __syncthreads();
      int lo, hi, i0;
      dtw_span(e, Tx, Ty, lo, hi, i0);
      const int nch = (hi - i0) / kNT + 1;
      double *cur = lds + m * rsz;
      const double *p1 = lds + (m == 0 ? 2 : m - 1) * rsz, *p2 = lds + (m == 2 ? 0 : m + 1) * rsz;
      unsigned long long *brow = bits + (int64_t)e * 2 * W;
#pragma unroll
      for (int k = 0; k < kPF; ++k)
        if (k < nch) dtw_cell(cc[k], i0 + k * kNT + tid, lo, hi, p2, p1, cur, brow);
      for (int c = kPF; c < nch; ++c)
        dtw_cell(dtw_cost<T>(x, y, A, e, c, Tx, Ty), i0 + c * kNT + tid, lo, hi, p2, p1, cur, brow);
      m = m == 2 ? 0 : m + 1;
    }
    if (!A.in_lds) __threadfence();  // the bitmap words, before thread 0 reads them back
    __syncthreads();
    // Thread 0 walks back, writing the path in reverse at the end of its rows; then every thread
    // moves it to the front. The path length goes through slot 0 of row 0.
    if (tid == 0) {
      A.total[b] = lds[((E - 1) % 3) * rsz + Tx];
      int i = Tx - 1, j = Ty - 1, k = 0;
      for (;;) {
        pi[P - 1 - k] = i;
        pj[P - 1 - k] = j;
        ++k;
        if (i == 0 && j == 0) break;
        const unsigned long long *wd = bits + ((int64_t)(i + j) * W + (i >> 6)) * 2;
        int step = (int)((wd[0] >> (i & 63)) & 1ull) + 2 * (int)((wd[1] >> (i & 63)) & 1ull);
        if (i == 0) step = 2;  // the only neighbour there is, whatever non-finite costs stored
        if (j == 0) step = 1;
        if (step != 2) --i;
        if (step != 1) --j;
      }
      A.K[b] = k;
      lds[0] = (double)k;
      __threadfence();  // the reversed path, before the other threads read it
    }
    __syncthreads();
    const int Kb = (int)lds[0], shift = P - Kb;
    for (int base = 0; base < Kb; base += kNT) {  // uniform; destinations lie below every unread source
      const int k = base + tid;
      int vi = 0, vj = 0;
      if (k < Kb) {
        vi = pi[shift + k];
        vj = pj[shift + k];
      }
      __syncthreads();
      if (k < Kb) {
        pi[k] = vi;
        pj[k] = vj;
      }
    }
    __syncthreads();
    for (int k = Kb + tid; k < P; k += kNT) pi[k] = pj[k] = -1;
  }
}

// ------------------------------------------------------------------------------------------------
// statistics along the path: one thread per (utterance, channel)

__global__ __launch_bounds__(kNT) void path_stats_kernel(const double *__restrict__ a, const double *__restrict__ bt,
                                                         const int *__restrict__ path_i, const int *__restrict__ path_j,
                                                         const int *__restrict__ K, int B, int Tx_max, int Ty_max,
                                                         int Ch, int64_t *__restrict__ counts,
                                                         double *__restrict__ sums) {
  const int64_t o = (int64_t)blockIdx.x * kNT + threadIdx.x;
  if (o >= (int64_t)B * Ch) return;
  const int ch = (int)(o % Ch), b = (int)(o / Ch);
  const int P = Tx_max + Ty_max - 1;
  const int Kb = K[b] < 0 ? 0 : (K[b] > P ? P : K[b]);
  const int *pi = path_i + (int64_t)b * P, *pj = path_j + (int64_t)b * P;
  const double *ar = a + (int64_t)b * Tx_max * Ch + ch, *br = bt + (int64_t)b * Ty_max * Ch + ch;
  int64_t n_both = 0, n_a = 0, n_b = 0, n_none = 0;
  double s = 0.0, s2 = 0.0;
  for (int k = 0; k < Kb; ++k) {
    const int i = pi[k], j = pj[k];
    if (i < 0 || i >= Tx_max || j < 0 || j >= Ty_max) break;
    const double va = ar[(int64_t)i * Ch], vb = br[(int64_t)j * Ch];
    const bool ha = va == va, hb = vb == vb;
    if (ha && hb) {
      const double d = va - vb;
      s = s + d;
      s2 = s2 + d * d;
      ++n_both;
    } else if (ha) {
      ++n_a;
    } else if (hb) {
      ++n_b;
    } else {
      ++n_none;
    }
  }
  counts[o * 4] = n_both;
  counts[o * 4 + 1] = n_a;
  counts[o * 4 + 2] = n_b;
  counts[o * 4 + 3] = n_none;
  sums[o * 2] = s;
  sums[o * 2 + 1] = s2;
}

// Compute units of the current device (cached per device id).
int ev_num_cus() {
  static int cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (cache[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    cache[dev] = n;
  }
  return cache[dev];
}

unsigned ev_grid(int64_t blocks, int per_cu) {
  const int cus = ev_num_cus();
  const int64_t slots = (int64_t)(cus > 0 ? cus : 256) * per_cu;
  return (unsigned)(blocks < slots ? blocks : slots);
}

// x [B, T_max, D] with unit stride along D: the strides cover the rows
int ev_check_rows(const void *p, int64_t bs, int64_t rs, int B, int T_max, int D) {
  if (p == nullptr || B < 1 || T_max < 1 || D < 1) return FS2_EINVAL;
  if (rs < D || (B > 1 && bs < (int64_t)(T_max - 1) * rs + D)) return FS2_EINVAL;
  return FS2_OK;
}

}  // namespace

extern "C" int64_t fs2_dtw_lds_bytes(int Tx_max, int Ty_max, int in_lds) {
  return Tx_max < 1 || Ty_max < 1 ? 0 : ev_dtw_lds_bytes(Tx_max, Ty_max, in_lds);
}

extern "C" int64_t fs2_dtw_ws_bytes(int B, int Tx_max, int Ty_max) {
  return B < 1 || Tx_max < 1 || Ty_max < 1 ? 0 : ev_dtw_ws_bytes(B, Tx_max, Ty_max);
}

extern "C" int fs2_mel_cepstrum(const void *mel, int dtype, int64_t batch_stride, int64_t row_stride,
                                const int64_t *lens, const double *basis, int B, int T_max, int M, int C, double *out,
                                fs2_stream_t stream) {
  const int rc = ev_check_rows(mel, batch_stride, row_stride, B, T_max, M);
  if (rc != FS2_OK) return rc;
  if (basis == nullptr || out == nullptr || C < 1) return FS2_EINVAL;
  const int64_t n = (int64_t)B * T_max * C;
  if (n > INT32_MAX) return FS2_EINVAL;
  if (dtype != FS2_F32 && dtype != FS2_F64) return FS2_EUNSUPPORTED;
  const dim3 grid(ev_grid((n + kNT - 1) / kNT, 8));
  const hipStream_t s = as_stream(stream);
  if (dtype == FS2_F32)
    hipLaunchKernelGGL(mel_cepstrum_kernel<float>, grid, dim3(kNT), 0, s, static_cast<const float *>(mel), batch_stride,
                       row_stride, lens, basis, B, T_max, M, C, out);
  else
    hipLaunchKernelGGL(mel_cepstrum_kernel<double>, grid, dim3(kNT), 0, s, static_cast<const double *>(mel),
                       batch_stride, row_stride, lens, basis, B, T_max, M, C, out);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_pair_dist(const void *x, const void *y, int dtype, int64_t x_batch_stride, int64_t x_row_stride,
                             int64_t y_batch_stride, int64_t y_row_stride, const int64_t *x_lens,
                             const int64_t *y_lens, int B, int Tx_max, int Ty_max, int D, int squared,
                             double *out, fs2_stream_t stream) {
  int rc = ev_check_rows(x, x_batch_stride, x_row_stride, B, Tx_max, D);
  if (rc != FS2_OK) return rc;
  rc = ev_check_rows(y, y_batch_stride, y_row_stride, B, Ty_max, D);
  if (rc != FS2_OK) return rc;
  if (out == nullptr) return FS2_EINVAL;
  if ((int64_t)B * Tx_max > INT32_MAX / (int64_t)Ty_max) return FS2_EINVAL;
  if (dtype != FS2_F32 && dtype != FS2_F64) return FS2_EUNSUPPORTED;
  PairArgs a;
  a.xbs = x_batch_stride;
  a.xrs = x_row_stride;
  a.ybs = y_batch_stride;
  a.yrs = y_row_stride;
  a.x_lens = x_lens;
  a.y_lens = y_lens;
  a.B = B;
  a.Tx_max = Tx_max;
  a.Ty_max = Ty_max;
  a.D = D;
  a.squared = squared != 0;
  const int64_t n = (int64_t)B * Tx_max * Ty_max;
  const dim3 grid(ev_grid((n + kNT - 1) / kNT, 8));
  const hipStream_t s = as_stream(stream);
  if (dtype == FS2_F32)
    hipLaunchKernelGGL(pair_dist_kernel<float>, grid, dim3(kNT), 0, s, static_cast<const float *>(x),
                       static_cast<const float *>(y), a, out);
  else
    hipLaunchKernelGGL(pair_dist_kernel<double>, grid, dim3(kNT), 0, s, static_cast<const double *>(x),
                       static_cast<const double *>(y), a, out);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_dtw(const void *x, const void *y, int dtype, int64_t x_batch_stride, int64_t x_row_stride,
                       int64_t y_batch_stride, int64_t y_row_stride, const int64_t *x_lens, const int64_t *y_lens,
                       int B, int Tx_max, int Ty_max, int D, int bitmap, void *ws, int64_t ws_bytes, double *total,
                       int32_t *K, int32_t *path_i, int32_t *path_j, fs2_stream_t stream) {
  int rc = ev_check_rows(x, x_batch_stride, x_row_stride, B, Tx_max, D);
  if (rc != FS2_OK) return rc;
  rc = ev_check_rows(y, y_batch_stride, y_row_stride, B, Ty_max, D);
  if (rc != FS2_OK) return rc;
  if (total == nullptr || K == nullptr || path_i == nullptr || path_j == nullptr) return FS2_EINVAL;
  if (dtype != FS2_F32 && dtype != FS2_F64) return FS2_EUNSUPPORTED;
  int form = FS2_DTW_LDS;
  rc = ev_dtw_form(Tx_max, Ty_max, bitmap, &form);
  if (rc != FS2_OK) return rc;
  if (form == FS2_DTW_GLOBAL && (ws == nullptr || ws_bytes < ev_dtw_ws_bytes(B, Tx_max, Ty_max))) return FS2_EINVAL;
  DtwArgs a;
  a.xbs = x_batch_stride;
  a.xrs = x_row_stride;
  a.ybs = y_batch_stride;
  a.yrs = y_row_stride;
  a.x_lens = x_lens;
  a.y_lens = y_lens;
  a.B = B;
  a.Tx_max = Tx_max;
  a.Ty_max = Ty_max;
  a.D = D;
  a.in_lds = form == FS2_DTW_LDS ? 1 : 0;
  a.ws = static_cast<unsigned long long *>(ws);
  a.total = total;
  a.K = K;
  a.path_i = path_i;
  a.path_j = path_j;
  const bool small = ev_dtw_lds_bytes(Tx_max, Ty_max, a.in_lds) <= FS2_DTW_LDS_SMALL;
  const dim3 grid(ev_grid(B, small ? 4 : 1));
  const hipStream_t s = as_stream(stream);
  if (dtype == FS2_F32) {
    const float *xf = static_cast<const float *>(x), *yf = static_cast<const float *>(y);
    if (small)
      hipLaunchKernelGGL((dtw_kernel<float, FS2_DTW_LDS_SMALL>), grid, dim3(kNT), 0, s, xf, yf, a);
    else
      hipLaunchKernelGGL((dtw_kernel<float, FS2_DTW_LDS_BYTES>), grid, dim3(kNT), 0, s, xf, yf, a);
  } else {
    const double *xd = static_cast<const double *>(x), *yd = static_cast<const double *>(y);
    if (small)
      hipLaunchKernelGGL((dtw_kernel<double, FS2_DTW_LDS_SMALL>), grid, dim3(kNT), 0, s, xd, yd, a);
    else
      hipLaunchKernelGGL((dtw_kernel<double, FS2_DTW_LDS_BYTES>), grid, dim3(kNT), 0, s, xd, yd, a);
  }
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_path_stats(const double *a, const double *b, const int32_t *path_i, const int32_t *path_j,
                              const int32_t *K, int B, int Tx_max, int Ty_max, int Ch, int64_t *counts, double *sums,
                              fs2_stream_t stream) {
  if (a == nullptr || b == nullptr || path_i == nullptr || path_j == nullptr || K == nullptr || counts == nullptr ||
      sums == nullptr)
    return FS2_EINVAL;
  if (B < 1 || Tx_max < 1 || Ty_max < 1 || Ch < 1 || (int64_t)B * Ch > INT32_MAX) return FS2_EINVAL;
  const int64_t n = (int64_t)B * Ch;
  hipLaunchKernelGGL(path_stats_kernel, dim3((unsigned)((n + kNT - 1) / kNT)), dim3(kNT), 0, as_stream(stream), a, b,
                     path_i, path_j, K, B, Tx_max, Ty_max, Ch, counts, sums);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}
