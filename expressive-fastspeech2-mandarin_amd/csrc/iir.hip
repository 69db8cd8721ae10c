// Recursive filtering and BS.1770 loudness (include/fs2hip_iir.h): cascaded second-order sections over
// a ragged batch as blocks of 64 samples run from zero state plus a Kogge-Stone scan over the block end
// states, the gating of a K-weighted row, and the gain to int16 / f32. Everything in float64 in the
// header's fixed order.
#include "fs2_common.h"
#include "fs2hip_audio.h"
#include "fs2hip_prep.h"
#include "iir_sizes.h"

// No a * b + c may become an FMA anywhere in this file (csrc/prep.hip explains why the helpers are
// defined under the pragma).
#pragma clang fp contract(off)

namespace {

constexpr int kNT = 256;  // threads of every workgroup here; one block of a chunk per thread
static_assert(kNT == FS2_IIR_CHUNK_BLOCKS, "one block per thread");

// offsets into one section's table (rule 3 of the header)
constexpr int kP = 0, kQ = 64, kPow = 128, kQi = 152;
static_assert(kQi + 65 * 4 == FS2_IIR_TABLE_LEN, "table layout");

__device__ __forceinline__ double add_rn(double a, double b) { return a + b; }
__device__ __forceinline__ double sub_rn(double a, double b) { return a - b; }
__device__ __forceinline__ double mul_rn(double a, double b) { return a * b; }
__device__ __forceinline__ double div_rn(double a, double b) { return a / b; }

__device__ __forceinline__ int64_t clamp_len(const int64_t *lens, int b, int64_t n_max) {
  const int64_t nl = lens != nullptr ? lens[b] : n_max;
  return nl < 0 ? 0 : (nl > n_max ? n_max : nl);
}

// (A v) of the header: two products and one add per component; A row-major
__device__ __forceinline__ void matvec(const double *A, double v1, double v2, double &r1, double &r2) {
  r1 = add_rn(mul_rn(A[0], v1), mul_rn(A[1], v2));
  r2 = add_rn(mul_rn(A[2], v1), mul_rn(A[3], v2));
}

struct SosArgs {
  int64_t stride;
  const int64_t *lens;
  int n_max, S;
  const double *sos, *tables, *zi;
  double *y;
  float *y32;
  double *zf;
};

__device__ __forceinline__ int lds_at(int u) { return u + (u >> 6); }  // sample u of the chunk: blocks 65 apart

// One workgroup per row. Sample u of the chunk at c0 lies in block u / 64 = thread u / 64 of the chunk;
// c0 is a multiple of 16384, so the row's block 256 (c0 / 16384) + tid is lane tid % 64 of group
// 4 (c0 / 16384) + tid / 64: wave w of the workgroup scans one group of the header.
template <typename T>
__global__ __launch_bounds__(kNT) void sosfilt_kernel(const T *__restrict__ wav, SosArgs A) {
  __shared__ double D[FS2_IIR_CHUNK_BLOCKS * FS2_IIR_PAD];
  __shared__ double tab[FS2_IIR_TABLE_LEN];
  __shared__ double st[2 * kNT];  // the incoming state of every block of the chunk
  __shared__ double wv[2 * (kNT / 64)];
  __shared__ double carry[2 * FS2_IIR_S_MAX], first[2 * FS2_IIR_S_MAX], prevx[FS2_IIR_S_MAX], prevy[FS2_IIR_S_MAX];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, b = blockIdx.x, S = A.S;
  const int64_t n = clamp_len(A.lens, b, A.n_max);
  const T *x = wav + (int64_t)b * A.stride;
  double *yrow = A.y + (int64_t)b * A.n_max;
  float *y32row = A.y32 != nullptr ? A.y32 + (int64_t)b * A.n_max : nullptr;

  if (tid < 2 * S) {
    const double v = A.zi != nullptr ? A.zi[(int64_t)b * S * 2 + tid] : 0.0;
    carry[tid] = v;
    first[tid] = v;
  }
  if (tid < S) {
    prevx[tid] = 0.0;
    prevy[tid] = 0.0;
  }
  // The samples of the chunk to come wait in registers (sample tid + 256 k in pre[k]): their loads are
  // issued together, before the work on the chunk at hand, which hides their latency; one workgroup
  // per compute unit has no other wave to hide it behind. Not for f64 input: 64 doubles beside the rest
  // do not fit the registers of a lane, and that input is read as it is needed.
  constexpr bool kPrefetch = sizeof(T) <= 4;
  T pre[kPrefetch ? FS2_IIR_BLOCK : 1];
  auto fetch = [&](int64_t c0) {
    const int64_t left = n - c0;
#pragma unroll
    for (int k = 0; k < FS2_IIR_BLOCK; ++k) {
      const int u = tid + kNT * k;
      pre[kPrefetch ? k : 0] = u < left ? x[c0 + u] : (T)0;
    }
  };
  if (kPrefetch && n > 0) fetch(0);
  for (int64_t c0 = 0; c0 < n; c0 += FS2_IIR_CHUNK) {
    const int cn = (int)(n - c0 < FS2_IIR_CHUNK ? n - c0 : FS2_IIR_CHUNK);
    const bool last = c0 + cn == n;
    __syncthreads();  // the chunk before is written out
    if constexpr (kPrefetch) {
#pragma unroll
      for (int k = 0; k < FS2_IIR_BLOCK; ++k) {
        const int u = tid + kNT * k;
        if (u < cn) D[lds_at(u)] = (double)pre[k];
      }
      if (!last) fetch(c0 + FS2_IIR_CHUNK);
    } else {
      for (int u = tid; u < cn; u += kNT) D[lds_at(u)] = (double)x[c0 + u];
    }
    __syncthreads();
    for (int s = 0; s < S; ++s) {
      for (int k = tid; k < FS2_IIR_TABLE_LEN; k += kNT) tab[k] = A.tables[(int64_t)s * FS2_IIR_TABLE_LEN + k];
      const double *cf = A.sos + 6 * s;
      const double b0 = cf[0], b1 = cf[1], b2 = cf[2], a1 = cf[4], a2 = cf[5];
      double xa = 0.0, xb = 0.0;  // the section's last two inputs (thread 0; rule 6)
      if (tid == 0) {
        xa = D[lds_at(cn - 1)];
        xb = cn >= 2 ? D[lds_at(cn - 2)] : prevx[s];
      }
      __syncthreads();
      // rule 2: this thread's block from zero state, in place
      int len = cn - 64 * tid;
      len = len < 0 ? 0 : (len > 64 ? 64 : len);
      double *blk = D + FS2_IIR_PAD * tid;
      double z1 = 0.0, z2 = 0.0;
      for (int i = 0; i < len; ++i) {
        const double xv = blk[i];
        const double yv = add_rn(mul_rn(b0, xv), z1);
        z1 = add_rn(sub_rn(mul_rn(b1, xv), mul_rn(a1, yv)), z2);
        z2 = sub_rn(mul_rn(b2, xv), mul_rn(a2, yv));
        blk[i] = yv;
      }
      // rule 4: the scan of this wave's group
      double v1 = z1, v2 = z2;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const int d = 1 << j;
        const double u1 = __shfl_up(v1, d, 64), u2 = __shfl_up(v2, d, 64);
        double r1, r2;
        matvec(tab + kPow + 4 * j, u1, u2, r1, r2);
        if (lane >= d) {
          v1 = add_rn(r1, v1);
          v2 = add_rn(r2, v2);
        }
      }
      if (lane == 63) {
        wv[2 * w] = v1;
        wv[2 * w + 1] = v2;
      }
      __syncthreads();
      double cg1 = carry[2 * s], cg2 = carry[2 * s + 1];  // the carry into this wave's group
      for (int g = 0; g < w; ++g) {
        double r1, r2;
        matvec(tab + kQi + 4 * 64, cg1, cg2, r1, r2);
        cg1 = add_rn(r1, wv[2 * g]);
        cg2 = add_rn(r2, wv[2 * g + 1]);
      }
      const double pv1 = __shfl_up(v1, 1, 64), pv2 = __shfl_up(v2, 1, 64);
      double s1 = cg1, s2 = cg2;
      if (lane > 0) {
        double r1, r2;
        matvec(tab + kQi + 4 * lane, cg1, cg2, r1, r2);
        s1 = add_rn(r1, pv1);
        s2 = add_rn(r2, pv2);
      }
      st[2 * tid] = s1;
      st[2 * tid + 1] = s2;
      __syncthreads();
      if (tid == kNT - 1 && cn == FS2_IIR_CHUNK) {  // the carry into the next chunk's first group
        double r1, r2;
        matvec(tab + kQi + 4 * 64, cg1, cg2, r1, r2);
        carry[2 * s] = add_rn(r1, v1);
        carry[2 * s + 1] = add_rn(r2, v2);
      }
      // rule 5
      const bool out = s == S - 1;
      for (int u = tid; u < cn; u += kNT) {
        const int k = u >> 6, i = u & 63, at = lds_at(u);
        const double yv = add_rn(add_rn(D[at], mul_rn(tab[kP + i], st[2 * k])), mul_rn(tab[kQ + i], st[2 * k + 1]));
        D[at] = yv;
        if (out) {
          yrow[c0 + u] = yv;
          if (y32row != nullptr) y32row[c0 + u] = (float)yv;
        }
      }
      __syncthreads();
      if (tid == 0) {  // rule 6
        const double ya = D[lds_at(cn - 1)];
        const double yb = cn >= 2 ? D[lds_at(cn - 2)] : prevy[s];
        if (last && A.zf != nullptr) {
          const double tail = n >= 2 ? sub_rn(mul_rn(b2, xb), mul_rn(a2, yb)) : first[2 * s + 1];
          double *zf = A.zf + ((int64_t)b * S + s) * 2;
          zf[0] = add_rn(sub_rn(mul_rn(b1, xa), mul_rn(a1, ya)), tail);
          zf[1] = sub_rn(mul_rn(b2, xa), mul_rn(a2, ya));
        }
        prevx[s] = xa;
        prevy[s] = ya;
      }
    }
  }
  if (n == 0 && A.zf != nullptr && tid < 2 * S) A.zf[(int64_t)b * S * 2 + tid] = first[tid];
  for (int64_t t = n + tid; t < A.n_max; t += kNT) {
    yrow[t] = 0.0;
    if (y32row != nullptr) y32row[t] = 0.0f;
  }
}

// ---- the gate --------------------------------------------------------------------------------------------

// The header's tree T over m values in cur (another buffer of at least (m + 1) / 2 behind nxt), by the
// whole workgroup, level by level. Returns the buffer whose element 0 is the value; a barrier has been
// passed since it was written.
__device__ __forceinline__ double *tree_levels(double *cur, double *nxt, int m) {
  while (m > 1) {
    __syncthreads();
    const int m2 = (m + 1) >> 1;
    for (int j = threadIdx.x; j < m2; j += kNT) nxt[j] = 2 * j + 1 < m ? add_rn(cur[2 * j], cur[2 * j + 1]) : cur[2 * j];
    double *t = cur;
    cur = nxt;
    nxt = t;
    m = m2;
  }
  __syncthreads();
  return cur;
}

// Sub-block blockIdx.x of row blockIdx.y: S_m into the row's part of the workspace.
__global__ __launch_bounds__(kNT) void loud_sums_kernel(const double *__restrict__ y, const int64_t *__restrict__ lens,
                                                        int n_max, int H, int64_t rw, double *__restrict__ ws) {
  __shared__ double La[FS2_LOUD_LEAVES_MAX], Lb[FS2_LOUD_LEAVES_MAX / 2];
  const int tid = threadIdx.x, b = blockIdx.y, m = blockIdx.x;
  const int64_t n = clamp_len(lens, b, n_max);
  const int64_t J = loud_blocks(n, H);
  if (J == 0 || m >= J + 3) return;  // uniform; (J + 3) H <= n, so every sub-block read is whole
  const double *src = y + (int64_t)b * n_max + (int64_t)m * H;
  const int nl = (H + 7) / 8;
  for (int j = tid; j < nl; j += kNT) {
    const int i0 = 8 * j, i1 = i0 + 8 < H ? i0 + 8 : H;
    double v = src[i0];
    v = mul_rn(v, v);
    for (int i = i0 + 1; i < i1; ++i) {
      const double t = src[i];
      v = add_rn(v, mul_rn(t, t));
    }
    La[j] = v;
  }
  const double *r = tree_levels(La, Lb, nl);
  if (tid == 0) ws[(int64_t)b * rw + m] = r[0];
}

// The gated tree of one stage: z_j where z_j > g1 and z_j > g2, +0.0 elsewhere; the count through cnt.
__device__ __forceinline__ double gated_tree(const double *S, int J, double Td, double g1, double g2, double *t0,
                                             double *t1, int *cnt, int &count) {
  if (threadIdx.x == 0) *cnt = 0;
  __syncthreads();
  int c = 0;
  for (int j = threadIdx.x; j < J; j += kNT) {
    const double z = div_rn(add_rn(add_rn(S[j], S[j + 1]), add_rn(S[j + 2], S[j + 3])), Td);
    const bool sel = z > g1 && z > g2;
    t0[j] = sel ? z : 0.0;
    c += sel ? 1 : 0;
  }
  if (c != 0) atomicAdd(cnt, c);
  const double *r = tree_levels(t0, t1, J);
  const double total = r[0];
  count = *cnt;
  __syncthreads();  // before the next stage resets the count and the buffers
  return total;
}

__global__ __launch_bounds__(kNT) void loud_gate_kernel(const int64_t *__restrict__ lens, int n_max, int H, int64_t J_max,
                                                        int64_t rw, double abs_gate, double rel_factor, double *ws,
                                                        double *__restrict__ zbar, int32_t *__restrict__ counts) {
  __shared__ int cnt;
  const int b = blockIdx.x;
  const int64_t n = clamp_len(lens, b, n_max);
  const int J = (int)loud_blocks(n, H);
  double zb = 0.0;
  int nA = 0, nR = 0;
  if (J > 0) {  // uniform
    double *S = ws + (int64_t)b * rw, *t0 = S + (J_max + 3), *t1 = t0 + J_max;
    const double Td = (double)(4 * (int64_t)H);
    const double sumA = gated_tree(S, J, Td, abs_gate, -1.0, t0, t1, &cnt, nA);
    if (nA > 0) {
      const double thr = mul_rn(rel_factor, div_rn(sumA, (double)nA));
      const double sumR = gated_tree(S, J, Td, abs_gate, thr, t0, t1, &cnt, nR);
      if (nR > 0) zb = div_rn(sumR, (double)nR);
    }
  }
  if (threadIdx.x == 0) {
    zbar[b] = zb;
    counts[3 * b] = J;
    counts[3 * b + 1] = nA;
    counts[3 * b + 2] = nR;
  }
}

// ---- the gain --------------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(kNT) void gain_peak_kernel(const T *__restrict__ wav, int64_t stride,
                                                        const int64_t *__restrict__ lens, int n_max,
                                                        unsigned long long *__restrict__ peak_bits) {
  const int b = blockIdx.y;
  const int64_t n = clamp_len(lens, b, n_max);
  const T *x = wav + (int64_t)b * stride;
  __shared__ double wmax[kNT / 64];
  double mx = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * kNT + threadIdx.x; t < n; t += (int64_t)gridDim.x * kNT) {
    const double v = (double)x[t];
    const double a = v < 0.0 ? -v : v;
    mx = a > mx ? a : mx;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_xor(mx, o, 64);
    mx = other > mx ? other : mx;
  }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {  // one atomic per workgroup: atomics on one address queue up behind each other
    for (int w = 1; w < kNT / 64; ++w) mx = wmax[w] > mx ? wmax[w] : mx;
    // non-negative doubles order as their bits do
    if (mx > 0.0) atomicMax(peak_bits + b, (unsigned long long)__double_as_longlong(mx));
  }
}

__device__ __forceinline__ double row_gain(double zb, double target_z, double peak_ceiling, const double *peak, int b) {
  if (!(zb > 0.0)) return 1.0;
  double g = sqrt(div_rn(target_z, zb));
  if (peak_ceiling > 0.0 && peak != nullptr && peak[b] > 0.0) {
    const double lim = div_rn(peak_ceiling, peak[b]);
    g = g > lim ? lim : g;
  }
  return g;
}

template <typename T>
__global__ __launch_bounds__(kNT) void gain_apply_kernel(const T *__restrict__ wav, int64_t stride,
                                                         const int64_t *__restrict__ lens, int n_max,
                                                         const double *__restrict__ zbar, double target_z,
                                                         double peak_ceiling, const double *__restrict__ peak,
                                                         T *__restrict__ q, double *__restrict__ gain,
                                                         int32_t *__restrict__ clipped, int32_t *__restrict__ unmeasured) {
  const int b = blockIdx.y;
  const int64_t n = clamp_len(lens, b, n_max);
  const T *x = wav + (int64_t)b * stride;
  T *o = q + (int64_t)b * n_max;
  const double zb = zbar[b];
  const double g = row_gain(zb, target_z, peak_ceiling, peak, b);  // the same bits in every thread
  int c = 0;
  for (int64_t t = (int64_t)blockIdx.x * kNT + threadIdx.x; t < n_max; t += (int64_t)gridDim.x * kNT) {
    if (t >= n) {
      o[t] = (T)0;
      continue;
    }
    const double v = mul_rn((double)x[t], g);
    if constexpr (sizeof(T) == 2) {
      double r = rint(v);  // to nearest, ties to even
      if (!(r <= 32767.0)) {
        r = 32767.0;
        ++c;
      } else if (r < -32768.0) {
        r = -32768.0;
        ++c;
      }
      o[t] = (T)(int)r;
    } else {
      o[t] = (T)v;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0 && c != 0) atomicAdd(clipped + b, c);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    gain[b] = g;
    if (unmeasured != nullptr) unmeasured[b] = zb > 0.0 ? 0 : 1;
  }
}

}  // namespace

extern "C" int64_t fs2_iir_blocks(int64_t n) { return iir_blocks(n); }

extern "C" int64_t fs2_iir_chunks(int64_t n) { return iir_chunks(n); }

extern "C" int64_t fs2_loudness_blocks(int64_t n, int64_t H) { return H < 1 ? -1 : loud_blocks(n, H); }

extern "C" int64_t fs2_loudness_workspace_bytes(int64_t B, int64_t n_max, int64_t H) {
  return loud_workspace_bytes(B, n_max, H);
}

extern "C" int fs2_sosfilt(const void *wav, int dtype, int64_t row_stride, const int64_t *lens, int B, int n_max,
                           const double *sos, const double *tables, int S, const double *zi, double *y, float *y32,
                           double *zf, fs2_stream_t stream) {
  if (wav == nullptr || sos == nullptr || tables == nullptr || y == nullptr) return FS2_EINVAL;
  const int rc = iir_check(B, n_max, S, row_stride);
  if (rc != FS2_OK) return rc;
  if (dtype != FS2_I16 && dtype != FS2_F32 && dtype != FS2_F64) return FS2_EUNSUPPORTED;
  SosArgs a;
  a.stride = row_stride;
  a.lens = lens;
  a.n_max = n_max;
  a.S = S;
  a.sos = sos;
  a.tables = tables;
  a.zi = zi;
  a.y = y;
  a.y32 = y32;
  a.zf = zf;
  const dim3 grid((unsigned)B);
  if (dtype == FS2_I16)
    hipLaunchKernelGGL(sosfilt_kernel<int16_t>, grid, dim3(kNT), 0, as_stream(stream), static_cast<const int16_t *>(wav),
                       a);
  else if (dtype == FS2_F32)
    hipLaunchKernelGGL(sosfilt_kernel<float>, grid, dim3(kNT), 0, as_stream(stream), static_cast<const float *>(wav), a);
  else
    hipLaunchKernelGGL(sosfilt_kernel<double>, grid, dim3(kNT), 0, as_stream(stream), static_cast<const double *>(wav),
                       a);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_loudness_gate(const double *y, const int64_t *lens, int B, int n_max, int H, double abs_gate,
                                 double rel_factor, double *zbar, int32_t *counts, void *workspace,
                                 int64_t workspace_bytes, fs2_stream_t stream) {
  if (y == nullptr || zbar == nullptr || counts == nullptr) return FS2_EINVAL;
  if (!(abs_gate >= 0.0) || !(rel_factor >= 0.0)) return FS2_EINVAL;
  const int rc = loud_check(B, n_max, H);
  if (rc != FS2_OK) return rc;
  const int64_t need = loud_workspace_bytes(B, n_max, H);
  if (need > 0 && (workspace == nullptr || workspace_bytes < need)) return FS2_EINVAL;
  const int64_t J_max = loud_blocks(n_max, H), rw = loud_row_doubles(J_max);
  double *ws = static_cast<double *>(workspace);
  if (J_max > 0) {
    if (J_max + 3 > INT32_MAX) return FS2_EUNSUPPORTED;
    hipLaunchKernelGGL(loud_sums_kernel, dim3((unsigned)(J_max + 3), (unsigned)B), dim3(kNT), 0, as_stream(stream), y, lens,
                       n_max, H, rw, ws);
    FS2_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(loud_gate_kernel, dim3((unsigned)B), dim3(kNT), 0, as_stream(stream), lens, n_max, H, J_max, rw,
                     abs_gate, rel_factor, ws, zbar, counts);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_gain_int16(const void *wav, int dtype, int64_t row_stride, const int64_t *lens, int B, int n_max,
                              const double *zbar, double target_z, double peak_ceiling, void *q, double *gain,
                              int32_t *clipped, int32_t *unmeasured, double *peak, fs2_stream_t stream) {
  if (wav == nullptr || zbar == nullptr || q == nullptr || gain == nullptr || clipped == nullptr) return FS2_EINVAL;
  const int rc = gain_check(B, n_max, row_stride);
  if (rc == FS2_EINVAL) return rc;
  if (!(target_z > 0.0) || !(target_z <= 1.7976931348623157e308) || !(peak_ceiling >= 0.0)) return FS2_EINVAL;
  if (peak == nullptr && peak_ceiling > 0.0) return FS2_EINVAL;
  if (rc != FS2_OK) return rc;
  if (dtype != FS2_I16 && dtype != FS2_F32) return FS2_EUNSUPPORTED;
  const hipStream_t s = as_stream(stream);
  const int64_t want = ((int64_t)n_max + kNT * 8 - 1) / (kNT * 8);  // about eight samples per thread
  const dim3 grid((unsigned)(want < 1024 ? want : 1024), (unsigned)B);
  if (hipMemsetAsync(clipped, 0, sizeof(int32_t) * (size_t)B, s) != hipSuccess) return FS2_ELAUNCH;
  if (peak != nullptr) {
    if (hipMemsetAsync(peak, 0, sizeof(double) * (size_t)B, s) != hipSuccess) return FS2_ELAUNCH;
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(peak);
    if (dtype == FS2_I16)
      hipLaunchKernelGGL(gain_peak_kernel<int16_t>, grid, dim3(kNT), 0, s, static_cast<const int16_t *>(wav), row_stride,
                         lens, n_max, bits);
    else
      hipLaunchKernelGGL(gain_peak_kernel<float>, grid, dim3(kNT), 0, s, static_cast<const float *>(wav), row_stride, lens,
                         n_max, bits);
    FS2_CHECK_LAUNCH();
  }
  if (dtype == FS2_I16)
    hipLaunchKernelGGL(gain_apply_kernel<int16_t>, grid, dim3(kNT), 0, s, static_cast<const int16_t *>(wav), row_stride,
                       lens, n_max, zbar, target_z, peak_ceiling, peak, static_cast<int16_t *>(q), gain, clipped,
                       unmeasured);
  else
    hipLaunchKernelGGL(gain_apply_kernel<float>, grid, dim3(kNT), 0, s, static_cast<const float *>(wav), row_stride, lens,
                       n_max, zbar, target_z, peak_ceiling, peak, static_cast<float *>(q), gain, clipped, unmeasured);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}
