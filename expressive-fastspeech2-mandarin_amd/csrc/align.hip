// Durations without a forced aligner (include/fs2hip_align.h): monotonic alignment search and the
// forward-sum (CTC) loss with its gradient, float64. Both are dynamic programmes sequential over mel
// frames and parallel over phonemes: one workgroup per utterance at a time (persistent workgroups walk
// the batch), the previous row ping-pong in LDS, one barrier per frame, the next frame's inputs
// fetched before that barrier.
#include "align_sizes.h"
#include "fs2_common.h"
#include "fs2hip_prep.h"

// Nothing here may be contracted: every operation the header names is one IEEE operation.
#pragma clang fp contract(off)

namespace {

constexpr int kNT = 256;  // threads per workgroup: 4 waves
constexpr int kNW = kNT / FS2_WAVE;
constexpr int kPF = 2;    // chunks of kNT cells whose next-frame inputs are fetched a frame ahead

__device__ __forceinline__ double neg_inf() { return -__builtin_inf(); }

__device__ __forceinline__ int clamp_len(const int64_t *lens, int b, int n_max) {
  const int64_t nl = lens != nullptr ? lens[b] : n_max;
  return (int)(nl < 0 ? 0 : (nl > n_max ? n_max : nl));
}

// ------------------------------------------------------------------------------------------------
// monotonic alignment search

struct MasArgs {
  int64_t bs, rs;
  const int64_t *mel_lens, *text_lens;
  int B, T_max, L_max, in_lds;
  unsigned long long *ws;
  int64_t *dur;
  double *score;
  int *path;
};

// One cell of frame t: phoneme j of chunk c (j < L or idle). Every lane of the wave calls it: the
// decisions of 64 neighbouring phonemes leave as one ballot word.
__device__ __forceinline__ void mas_cell(double xv, int c, int L, const double *prev, double *cur,
                                         unsigned long long *bits_row) {
  const int tid = threadIdx.x, j = c * kNT + tid;
  const bool in = j < L;
  const double vs = in ? prev[1 + j] : 0.0, vd = in ? prev[j] : 0.0;  // slot 0 is v[-1]
  const bool d = in && j >= 1 && vd >= vs;
  if (in) cur[1 + j] = xv + (d ? vd : vs);
  const unsigned long long m = __ballot(d);
  const int j0 = c * kNT + (tid & ~(FS2_WAVE - 1));  // the wave's first phoneme
  if ((tid & (FS2_WAVE - 1)) == 0 && j0 < L) bits_row[j0 >> 6] = m;
}

template <typename T, int kBytes>
__global__ __launch_bounds__(kNT) void mas_kernel(const T *__restrict__ logp, MasArgs A) {
  __shared__ __align__(16) double lds[kBytes / 8];
  const int tid = threadIdx.x;
  const int rsz = (int)al_mas_row(A.L_max), W = (int)al_words(A.L_max);
  unsigned long long *lbits = reinterpret_cast<unsigned long long *>(lds + 2 * rsz);
  for (int b = blockIdx.x; b < A.B; b += gridDim.x) {  // uniform
    const int Tb = clamp_len(A.mel_lens, b, A.T_max), L = clamp_len(A.text_lens, b, A.L_max);
    const bool skip = Tb == 0 || L == 0 || Tb < L;
    int64_t *dur = A.dur + (int64_t)b * A.L_max;
    int *path = A.path != nullptr ? A.path + (int64_t)b * A.T_max : nullptr;
    for (int j = tid; j < A.L_max; j += kNT) dur[j] = 0;
    if (path != nullptr)
      for (int t = (skip ? 0 : Tb) + tid; t < A.T_max; t += kNT) path[t] = -1;
    if (skip) {  // uniform
      if (tid == 0) A.score[b] = neg_inf();
      continue;
    }
    unsigned long long *bits = A.in_lds ? lbits : A.ws + (int64_t)b * A.T_max * W;
    const T *x = logp + (int64_t)b * A.bs;
    const int nch = (L + kNT - 1) / kNT;
    __syncthreads();  // the previous utterance's backtrack is done with the rows and the bitmap
    for (int j = tid; j < L; j += kNT) lds[1 + j] = j == 0 ? (double)x[0] : neg_inf();
    if (tid == 0) lds[0] = lds[rsz] = neg_inf();
    double xn[kPF];
#pragma unroll
    for (int k = 0; k < kPF; ++k) {
      const int j = k * kNT + tid;
      xn[k] = Tb > 1 && j < L ? (double)x[A.rs + j] : 0.0;
    }
    for (int t = 1; t < Tb; ++t) {
      const T *xrow = x + (int64_t)t * A.rs;
      double xc[kPF];
#pragma unroll
      for (int k = 0; k < kPF; ++k) {
        const int j = k * kNT + tid;
        xc[k] = xn[k];
        xn[k] = t + 1 < Tb && j < L ? (double)xrow[A.rs + j] : 0.0;
      }
      __syncthreads();
      const double *prev = lds + ((t - 1) & 1) * rsz;
      double *cur = lds + (t & 1) * rsz;
      unsigned long long *brow = bits + (int64_t)t * W;
#pragma unroll
      for (int k = 0; k < kPF; ++k)
        if (k < nch) mas_cell(xc[k], k, L, prev, cur, brow);
      for (int c = kPF; c < nch; ++c) {
        const int j = c * kNT + tid;
        mas_cell(j < L ? (double)xrow[j] : 0.0, c, L, prev, cur, brow);
      }
    }
    if (!A.in_lds) __threadfence();  // the bitmap words, before thread 0 reads them back
    __syncthreads();
    if (tid == 0) {
      A.score[b] = lds[((Tb - 1) & 1) * rsz + L];
      int j = L - 1;
      int64_t cnt = 0;
      for (int t = Tb - 1; t >= 0; --t) {
        ++cnt;
        if (path != nullptr) path[t] = j;
        if (t >= 1 && j >= 1 && ((bits[(int64_t)t * W + (j >> 6)] >> (j & 63)) & 1ull)) {
          dur[j] = cnt;
          cnt = 0;
          --j;
        }
      }
      dur[j] = cnt;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// forward sum

struct FsArgs {
  int64_t bs, rs;
  const int64_t *mel_lens, *text_lens;
  int B, T_max, L_max;
  double blank;
  double *alpha;        // forward: out; backward: in
  double *nll;          // forward: out; backward: in
  const double *gout;   // backward
};

// max and log-sum of every frame's L + 1 logits: one wave per frame, a fixed order for a given L
template <typename T>
__device__ __forceinline__ void fs_frame_lse(const T *x, int64_t rs, int Tb, int L, double blank, double *mx,
                                             double *ls) {
  const int lane = threadIdx.x & (FS2_WAVE - 1), wave = threadIdx.x / FS2_WAVE;
  for (int t = wave; t < Tb; t += kNW) {
    const T *row = x + (int64_t)t * rs;
    double m = blank;
    for (int j = lane; j < L; j += FS2_WAVE) m = fmax(m, (double)row[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, FS2_WAVE));
    double s = lane == 0 ? exp(blank - m) : 0.0;
    for (int j = lane; j < L; j += FS2_WAVE) s = s + exp((double)row[j] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, FS2_WAVE);
    if (lane == 0) {
      mx[t] = m;
      ls[t] = log(s);
    }
  }
}

// log(exp(a1) + exp(a2) + exp(a3)) in the operation order of the header
__device__ __forceinline__ double lse3(double a1, double a2, double a3) {
  double m = fmax(fmax(a1, a2), a3);
  if (m == neg_inf()) m = 0.0;
  return log((exp(a1 - m) + exp(a2 - m)) + exp(a3 - m)) + m;
}
__device__ __forceinline__ double lse2(double a1, double a2) {
  double m = fmax(a1, a2);
  if (m == neg_inf()) m = 0.0;
  return log(exp(a1 - m) + exp(a2 - m)) + m;
}

// Thread j (0 .. L) of frame t owns the blank state 2 j and, for j < L, the label state 2 j + 1.
// State s lives in slot 2 + s of a row; slots 0, 1 and 2 + S hold -inf.
__device__ __forceinline__ void fs_alpha_cell(double z, int j, int L, double lp_blank, double mxt, double lst,
                                              const double *prev, double *cur, double *arow) {
  if (j > L) return;
  const double a_e = lse2(prev[2 + 2 * j], prev[1 + 2 * j]) + lp_blank;
  cur[2 + 2 * j] = a_e;
  arow[2 * j] = a_e;
  if (j < L) {
    const double lp = (z - mxt) - lst;
    const double a_o = lse3(prev[3 + 2 * j], prev[2 + 2 * j], prev[1 + 2 * j]) + lp;
    cur[3 + 2 * j] = a_o;
    arow[2 * j + 1] = a_o;
  }
}

template <typename T>
__global__ __launch_bounds__(kNT) void forward_sum_kernel(const T *__restrict__ logp, FsArgs A) {
  extern __shared__ __align__(16) double lds[];
  const int tid = threadIdx.x;
  const int rsz = (int)al_fs_row(A.L_max), SM = 2 * A.L_max + 1;
  double *mx = lds + 2 * rsz, *ls = mx + A.T_max;
  for (int b = blockIdx.x; b < A.B; b += gridDim.x) {  // uniform
    const int Tb = clamp_len(A.mel_lens, b, A.T_max), L = clamp_len(A.text_lens, b, A.L_max);
    if (Tb == 0 || L == 0 || Tb < L) {  // uniform
      if (tid == 0) A.nll[b] = __builtin_inf();
      continue;
    }
    const T *x = logp + (int64_t)b * A.bs;
    double *alpha = A.alpha + (int64_t)b * A.T_max * SM;
    const int S = 2 * L + 1, nch = (L + 1 + kNT - 1) / kNT;
    __syncthreads();  // the previous utterance is done with the LDS
    fs_frame_lse(x, A.rs, Tb, L, A.blank, mx, ls);
    if (tid < 2) {
      lds[tid] = lds[rsz + tid] = neg_inf();
      lds[2 + S + tid] = lds[rsz + 2 + S + tid] = neg_inf();
    }
    __syncthreads();
    {  // frame 0: states 0 and 1 start
      const double lpb = (A.blank - mx[0]) - ls[0];
      for (int j = tid; j <= L; j += kNT) {
        const double a_e = j == 0 ? lpb : neg_inf();
        lds[2 + 2 * j] = a_e;
        alpha[2 * j] = a_e;
        if (j < L) {
          const double a_o = j == 0 ? ((double)x[0] - mx[0]) - ls[0] : neg_inf();
          lds[3 + 2 * j] = a_o;
          alpha[2 * j + 1] = a_o;
        }
      }
    }
    double zn[kPF];
#pragma unroll
    for (int k = 0; k < kPF; ++k) {
      const int j = k * kNT + tid;
      zn[k] = Tb > 1 && j < L ? (double)x[A.rs + j] : 0.0;
    }
    for (int t = 1; t < Tb; ++t) {
      const T *xrow = x + (int64_t)t * A.rs;
      double zc[kPF];
#pragma unroll
      for (int k = 0; k < kPF; ++k) {
        const int j = k * kNT + tid;
        zc[k] = zn[k];
        zn[k] = t + 1 < Tb && j < L ? (double)xrow[A.rs + j] : 0.0;
      }
      __syncthreads();
      const double *prev = lds + ((t - 1) & 1) * rsz;
      double *cur = lds + (t & 1) * rsz;
      double *arow = alpha + (int64_t)t * SM;
      const double mxt = mx[t], lst = ls[t], lpb = (A.blank - mxt) - lst;
#pragma unroll
      for (int k = 0; k < kPF; ++k)
        if (k < nch) fs_alpha_cell(zc[k], k * kNT + tid, L, lpb, mxt, lst, prev, cur, arow);
      for (int c = kPF; c < nch; ++c) {
        const int j = c * kNT + tid;
        fs_alpha_cell(j < L ? (double)xrow[j] : 0.0, j, L, lpb, mxt, lst, prev, cur, arow);
      }
    }
    __syncthreads();
    if (tid == 0) {
      const double *last = lds + ((Tb - 1) & 1) * rsz;
      A.nll[b] = -lse2(last[2 + S - 1], last[2 + S - 2]);
    }
  }
}

// loss = (sum of nll[b] / L_b over the finite ones, in index order) / B
__global__ void forward_sum_loss_kernel(const double *__restrict__ nll, const int64_t *__restrict__ text_lens, int B,
                                        int L_max, double *__restrict__ loss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double acc = 0.0;
  for (int b = 0; b < B; ++b) {
    const double v = nll[b];
    const int L = clamp_len(text_lens, b, L_max);
    if (L > 0 && v - v == 0.0) acc = acc + v / (double)L;  // finite
  }
  loss[0] = acc / (double)B;
}

template <typename T>
__device__ __forceinline__ void fs_beta_cell(double z, double a, int j, int L, double lp_blank, double mxt, double lst,
                                             const double *next, double *cur, double nllb, double scale, T *grow) {
  if (j > L) return;
  cur[2 + 2 * j] = lse2(next[2 + 2 * j], next[3 + 2 * j]) + lp_blank;
  if (j < L) {
    const double lp = (z - mxt) - lst;
    const double be = lse3(next[3 + 2 * j], next[4 + 2 * j], next[5 + 2 * j]) + lp;
    cur[3 + 2 * j] = be;
    grow[j] = (T)((exp(lp) - exp(((a + be) + nllb) - lp)) * scale);
  }
}

template <typename T>
__global__ __launch_bounds__(kNT) void forward_sum_bwd_kernel(const T *__restrict__ logp, FsArgs A,
                                                              T *__restrict__ grad) {
  extern __shared__ __align__(16) double lds[];
  const int tid = threadIdx.x;
  const int rsz = (int)al_fs_row(A.L_max), SM = 2 * A.L_max + 1;
  double *mx = lds + 2 * rsz, *ls = mx + A.T_max;
  for (int b = blockIdx.x; b < A.B; b += gridDim.x) {  // uniform
    const int Tb = clamp_len(A.mel_lens, b, A.T_max), L = clamp_len(A.text_lens, b, A.L_max);
    const double nllb = A.nll[b];
    const bool skip = Tb == 0 || L == 0 || Tb < L || !(nllb - nllb == 0.0);  // uniform
    T *g = grad + (int64_t)b * A.T_max * A.L_max;
    const int Tv = skip ? 0 : Tb;
    // exact zeros outside [T_b, L_b]: the tails of the valid rows, then the rows past them
    for (int t = 0; t < Tv; ++t)
      for (int j = L + tid; j < A.L_max; j += kNT) g[(int64_t)t * A.L_max + j] = (T)0;
    for (int64_t e = (int64_t)Tv * A.L_max + tid; e < (int64_t)A.T_max * A.L_max; e += kNT) g[e] = (T)0;
    if (skip) continue;
    const T *x = logp + (int64_t)b * A.bs;
    const double *alpha = A.alpha + (int64_t)b * A.T_max * SM;
    const int S = 2 * L + 1, nch = (L + 1 + kNT - 1) / kNT;
    const double scale = A.gout[0] / ((double)L * (double)A.B);
    __syncthreads();  // the previous utterance is done with the LDS
    fs_frame_lse(x, A.rs, Tb, L, A.blank, mx, ls);
    if (tid < 2) {
      lds[tid] = lds[rsz + tid] = neg_inf();
      lds[2 + S + tid] = lds[rsz + 2 + S + tid] = neg_inf();
    }
    __syncthreads();
    {  // the last frame: the last two states end
      const int t = Tb - 1;
      const double mxt = mx[t], lst = ls[t];
      double *cur = lds + (t & 1) * rsz;
      for (int j = tid; j <= L; j += kNT) {
        cur[2 + 2 * j] = j == L ? (A.blank - mxt) - lst : neg_inf();
        if (j < L) {
          const double lp = ((double)x[(int64_t)t * A.rs + j] - mxt) - lst;
          const double be = j == L - 1 ? lp : neg_inf();
          cur[3 + 2 * j] = be;
          const double a = alpha[(int64_t)t * SM + 2 * j + 1];
          g[(int64_t)t * A.L_max + j] = (T)((exp(lp) - exp(((a + be) + nllb) - lp)) * scale);
        }
      }
    }
    double zn[kPF], an[kPF];
#pragma unroll
    for (int k = 0; k < kPF; ++k) {
      const int j = k * kNT + tid;
      const bool in = Tb > 1 && j < L;
      zn[k] = in ? (double)x[(int64_t)(Tb - 2) * A.rs + j] : 0.0;
      an[k] = in ? alpha[(int64_t)(Tb - 2) * SM + 2 * j + 1] : 0.0;
    }
    for (int t = Tb - 2; t >= 0; --t) {
      const T *xrow = x + (int64_t)t * A.rs;
      const double *arow = alpha + (int64_t)t * SM;
      double zc[kPF], ac[kPF];
#pragma unroll
      for (int k = 0; k < kPF; ++k) {
        const int j = k * kNT + tid;
        const bool in = t >= 1 && j < L;
        zc[k] = zn[k];
        ac[k] = an[k];
        zn[k] = in ? (double)xrow[j - A.rs] : 0.0;
        an[k] = in ? arow[2 * j + 1 - SM] : 0.0;
      }
      __syncthreads();
      const double *next = lds + ((t + 1) & 1) * rsz;
      double *cur = lds + (t & 1) * rsz;
      T *grow = g + (int64_t)t * A.L_max;
      const double mxt = mx[t], lst = ls[t], lpb = (A.blank - mxt) - lst;
#pragma unroll
      for (int k = 0; k < kPF; ++k)
        if (k < nch) fs_beta_cell<T>(zc[k], ac[k], k * kNT + tid, L, lpb, mxt, lst, next, cur, nllb, scale, grow);
      for (int c = kPF; c < nch; ++c) {
        const int j = c * kNT + tid;
        const bool in = j < L;
        fs_beta_cell<T>(in ? (double)xrow[j] : 0.0, in ? arow[2 * j + 1] : 0.0, j, L, lpb, mxt, lst, next, cur, nllb,
                        scale, grow);
      }
    }
  }
}

// Compute units of the current device (cached per device id).
int al_num_cus() {
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

unsigned al_grid(int B, int per_cu) {
  const int cus = al_num_cus();
  const int64_t slots = (int64_t)(cus > 0 ? cus : 256) * per_cu;
  return (unsigned)(B < slots ? B : slots);
}

int fs_check(const void *logp, int dtype, int64_t bs, int64_t rs, int B, int T_max, int L_max) {
  if (logp == nullptr || B < 1 || T_max < 1 || L_max < 1) return FS2_EINVAL;
  if (rs < L_max || (B > 1 && bs < (int64_t)(T_max - 1) * rs + L_max)) return FS2_EINVAL;
  if (dtype != FS2_F32 && dtype != FS2_F64) return FS2_EUNSUPPORTED;
  return FS2_OK;
}

}  // namespace

extern "C" int64_t fs2_mas_lds_bytes(int T_max, int L_max, int in_lds) {
  return T_max < 1 || L_max < 1 ? 0 : al_mas_lds_bytes(T_max, L_max, in_lds);
}

extern "C" int64_t fs2_mas_ws_bytes(int B, int T_max, int L_max) {
  return B < 1 || T_max < 1 || L_max < 1 ? 0 : al_mas_ws_bytes(B, T_max, L_max);
}

extern "C" int64_t fs2_forward_sum_lds_bytes(int T_max, int L_max) {
  return T_max < 1 || L_max < 1 ? 0 : al_fs_lds_bytes(T_max, L_max);
}

extern "C" int fs2_mas(const void *logp, int dtype, int64_t batch_stride, int64_t row_stride, const int64_t *mel_lens,
                       const int64_t *text_lens, int B, int T_max, int L_max, int bitmap, void *ws, int64_t ws_bytes,
                       int64_t *durations, double *score, int32_t *path, fs2_stream_t stream) {
  int rc = fs_check(logp, dtype, batch_stride, row_stride, B, T_max, L_max);
  if (rc != FS2_OK) return rc;
  if (durations == nullptr || score == nullptr) return FS2_EINVAL;
  int form = FS2_MAS_LDS;
  rc = al_mas_form(T_max, L_max, bitmap, &form);
  if (rc != FS2_OK) return rc;
  if (form == FS2_MAS_GLOBAL && (ws == nullptr || ws_bytes < al_mas_ws_bytes(B, T_max, L_max))) return FS2_EINVAL;
  MasArgs a;
  a.bs = batch_stride;
  a.rs = row_stride;
  a.mel_lens = mel_lens;
  a.text_lens = text_lens;
  a.B = B;
  a.T_max = T_max;
  a.L_max = L_max;
  a.in_lds = form == FS2_MAS_LDS ? 1 : 0;
  a.ws = static_cast<unsigned long long *>(ws);
  a.dur = durations;
  a.score = score;
  a.path = path;
  const bool small = al_mas_lds_bytes(T_max, L_max, a.in_lds) <= FS2_MAS_LDS_SMALL;
  const dim3 grid(al_grid(B, small ? 4 : 1));
  const hipStream_t s = as_stream(stream);
  if (dtype == FS2_F32) {
    const float *x = static_cast<const float *>(logp);
    if (small)
      hipLaunchKernelGGL((mas_kernel<float, FS2_MAS_LDS_SMALL>), grid, dim3(kNT), 0, s, x, a);
    else
      hipLaunchKernelGGL((mas_kernel<float, FS2_MAS_LDS_BYTES>), grid, dim3(kNT), 0, s, x, a);
  } else {
    const double *x = static_cast<const double *>(logp);
    if (small)
      hipLaunchKernelGGL((mas_kernel<double, FS2_MAS_LDS_SMALL>), grid, dim3(kNT), 0, s, x, a);
    else
      hipLaunchKernelGGL((mas_kernel<double, FS2_MAS_LDS_BYTES>), grid, dim3(kNT), 0, s, x, a);
  }
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_forward_sum(const void *logp, int dtype, int64_t batch_stride, int64_t row_stride,
                               const int64_t *mel_lens, const int64_t *text_lens, int B, int T_max, int L_max,
                               double blank_logprob, double *alpha, double *nll, double *loss, fs2_stream_t stream) {
  const int rc = fs_check(logp, dtype, batch_stride, row_stride, B, T_max, L_max);
  if (rc != FS2_OK) return rc;
  if (alpha == nullptr || nll == nullptr || loss == nullptr || !(blank_logprob - blank_logprob == 0.0))
    return FS2_EINVAL;
  const int64_t lds = al_fs_lds_bytes(T_max, L_max);
  if (lds > FS2_FORWARD_SUM_LDS_BYTES) return FS2_EUNSUPPORTED;
  FsArgs a;
  a.bs = batch_stride;
  a.rs = row_stride;
  a.mel_lens = mel_lens;
  a.text_lens = text_lens;
  a.B = B;
  a.T_max = T_max;
  a.L_max = L_max;
  a.blank = blank_logprob;
  a.alpha = alpha;
  a.nll = nll;
  a.gout = nullptr;
  const dim3 grid(al_grid(B, 2));
  const hipStream_t s = as_stream(stream);
  if (dtype == FS2_F32)
    hipLaunchKernelGGL(forward_sum_kernel<float>, grid, dim3(kNT), (size_t)lds, s, static_cast<const float *>(logp), a);
  else
    hipLaunchKernelGGL(forward_sum_kernel<double>, grid, dim3(kNT), (size_t)lds, s, static_cast<const double *>(logp),
                       a);
  FS2_CHECK_LAUNCH();
  hipLaunchKernelGGL(forward_sum_loss_kernel, dim3(1), dim3(FS2_WAVE), 0, s, nll, text_lens, B, L_max, loss);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_forward_sum_bwd(const void *logp, int dtype, int64_t batch_stride, int64_t row_stride,
                                   const int64_t *mel_lens, const int64_t *text_lens, int B, int T_max, int L_max,
                                   double blank_logprob, const double *alpha, const double *nll,
                                   const double *grad_out, void *grad, fs2_stream_t stream) {
  const int rc = fs_check(logp, dtype, batch_stride, row_stride, B, T_max, L_max);
  if (rc != FS2_OK) return rc;
  if (alpha == nullptr || nll == nullptr || grad_out == nullptr || grad == nullptr ||
      !(blank_logprob - blank_logprob == 0.0))
    return FS2_EINVAL;
  const int64_t lds = al_fs_lds_bytes(T_max, L_max);
  if (lds > FS2_FORWARD_SUM_LDS_BYTES) return FS2_EUNSUPPORTED;
  FsArgs a;
  a.bs = batch_stride;
  a.rs = row_stride;
  a.mel_lens = mel_lens;
  a.text_lens = text_lens;
  a.B = B;
  a.T_max = T_max;
  a.L_max = L_max;
  a.blank = blank_logprob;
  a.alpha = const_cast<double *>(alpha);
  a.nll = const_cast<double *>(nll);
  a.gout = grad_out;
  const dim3 grid(al_grid(B, 2));
  const hipStream_t s = as_stream(stream);
  if (dtype == FS2_F32)
    hipLaunchKernelGGL(forward_sum_bwd_kernel<float>, grid, dim3(kNT), (size_t)lds, s,
                       static_cast<const float *>(logp), a, static_cast<float *>(grad));
  else
    hipLaunchKernelGGL(forward_sum_bwd_kernel<double>, grid, dim3(kNT), (size_t)lds, s,
                       static_cast<const double *>(logp), a, static_cast<double *>(grad));
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}
