// Silence trimming and splitting (include/fs2hip_vad.h): frame power in float64 in the header's fixed
// order, the activity mask with its short-silence fill, the intervals and the trim of every row, and
// the ragged cut. The power kernel stages each tile's samples in LDS once and sums every block of
// gcd(frame_length, hop) samples once; the interval kernel is one workgroup per row walking the frames
// in chunks.
#include "fs2_common.h"
#include "fs2hip_audio.h"
#include "vad_sizes.h"

// No a * b + c may become an FMA anywhere in this file (csrc/prep.hip explains why the helpers are
// defined under the pragma).
#pragma clang fp contract(off)

namespace {

constexpr int kNT = 256;  // threads of a power workgroup

__device__ __forceinline__ double add_rn(double a, double b) { return a + b; }
__device__ __forceinline__ double mul_rn(double a, double b) { return a * b; }
__device__ __forceinline__ double div_rn(double a, double b) { return a / b; }

__device__ __forceinline__ int64_t clamp_len(const int64_t *lens, int b, int64_t n_max) {
  const int64_t nl = lens != nullptr ? lens[b] : n_max;
  return nl < 0 ? 0 : (nl > n_max ? n_max : nl);
}

constexpr int kLev = 13;  // levels of the pairwise tree: up to 2^13 - 1 values (a block's leaves, a frame's blocks)
constexpr int kLeaf = 8;  // squares per leaf

// The header's tree T over values pushed in order, as a binary counter: level l holds the sum of an
// aligned group of 2^l values; a new value is added to the waiting group of its size, and so on up.
// total() adds what is left from the smallest group up, which is the carried last element of each
// level of the header's statement. nlev (uniform) >= the bit length of the number of values.
struct Tree {
  double st[kLev];
  unsigned cnt = 0;
  __device__ __forceinline__ void push(double v, int nlev) {
    unsigned c = cnt++;
    bool done = false;
#pragma unroll
    for (int l = 0; l < kLev; ++l) {
      if (!done && l < nlev) {
        if (c & 1u) {
          v = add_rn(st[l], v);
          c >>= 1;
        } else {
          st[l] = v;
          done = true;
        }
      }
    }
  }
  __device__ __forceinline__ double total(int nlev) const {
    double acc = 0.0;
    bool has = false;
#pragma unroll
    for (int l = 0; l < kLev; ++l) {
      if (l < nlev && ((cnt >> l) & 1u)) {
        acc = has ? add_rn(st[l], acc) : st[l];
        has = true;
      }
    }
    return acc;
  }
};

__host__ __device__ inline int bit_length(unsigned v) {
  int n = 0;
  for (; v != 0; v >>= 1) ++n;
  return n;
}

struct PowArgs {
  int64_t stride;
  const int64_t *lens;
  int n_max, F_max, L, hop;
  int g, q, h;  // block size; blocks per frame; blocks between neighbouring frames
  int G, nb;    // frames and blocks per tile
  int gs, pb;   // elements between neighbouring blocks in LDS; blocks per staging pass
  int lev_leaf, lev_q;
  int tiles;
  double *P;
  double *tmax;  // [B, tiles]
};

// Tile `blockIdx.x` of row `blockIdx.y`: frames f0 .. f0 + G. Block kb of the tile is samples
// [base + kb * g, base + (kb + 1) * g) of the row, base = f0 * hop - L / 2.
template <typename T>
__global__ __launch_bounds__(kNT) void vad_power_kernel(const T *__restrict__ wav, PowArgs A) {
  __shared__ double S[FS2_VAD_SUMS_MAX];
  __shared__ __align__(16) unsigned char area[FS2_VAD_AREA_BYTES];
  __shared__ double wmax[kNT / 64];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int f0 = blockIdx.x * A.G;
  const int64_t n = clamp_len(A.lens, b, A.n_max);
  const int F = (int)vad_frames(n, A.hop);
  T *X = reinterpret_cast<T *>(area);
  const T *x = wav + (int64_t)b * A.stride;
  const int64_t g = A.g, base = (int64_t)f0 * A.hop - A.L / 2;
  const int pad = A.gs - A.g;

  for (int k = tid; k < A.nb; k += kNT) S[k] = 0.0;
  if (f0 < F) {  // uniform
    // the tile's blocks that hold a sample of [0, n): the others are +0.0
    const int64_t t = -base - g;
    const int64_t lo64 = t < 0 ? 0 : t / g + 1;
    const int64_t hi64 = n - base > 0 ? (n - base + g - 1) / g : 0;
    const int kb_lo = (int)(lo64 < A.nb ? lo64 : A.nb), kb_hi = (int)(hi64 < A.nb ? hi64 : A.nb);
    for (int p0 = kb_lo; p0 < kb_hi; p0 += A.pb) {
      const int np = kb_hi - p0 < A.pb ? kb_hi - p0 : A.pb;  // blocks of this pass
      const int cn = np * A.g;                               // <= FS2_VAD_AREA_BYTES / sizeof(T)
      const int64_t s0 = base + (int64_t)p0 * g;             // the pass's first sample
      __syncthreads();                                        // the previous pass's readers are done
      for (int u = tid; u < cn; u += kNT) {
        const int64_t i = s0 + u;
        const T v = i >= 0 && i < n ? x[i] : (T)0;
        X[pad == 0 ? u : u + (int)((unsigned)u / (unsigned)A.g) * pad] = v;
      }
      __syncthreads();
      for (int j = tid; j < np; j += kNT) {
        const T *src = X + j * A.gs;
        Tree tr;
        for (int i0 = 0; i0 < A.g; i0 += kLeaf) {
          const int i1 = i0 + kLeaf < A.g ? i0 + kLeaf : A.g;
          double v = (double)src[i0];
          v = mul_rn(v, v);
          for (int i = i0 + 1; i < i1; ++i) {
            const double w = (double)src[i];
            v = add_rn(v, mul_rn(w, w));
          }
          tr.push(v, A.lev_leaf);
        }
        S[p0 + j] = tr.total(A.lev_leaf);
      }
    }
  }
  __syncthreads();
  double mx = 0.0;
  if (tid < A.G) {
    const int f = f0 + tid;
    if (f < A.F_max) {
      double p = 0.0;
      if (f < F) {
        Tree tr;
        for (int i = 0; i < A.q; ++i) tr.push(S[tid * A.h + i], A.lev_q);
        p = div_rn(tr.total(A.lev_q), (double)A.L);
      }
      A.P[(int64_t)b * A.F_max + f] = p;
      mx = p;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_xor(mx, o, 64);
    mx = other > mx ? other : mx;
  }
  if ((tid & 63) == 0) wmax[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kNT / 64; ++w) mx = wmax[w] > mx ? wmax[w] : mx;
    A.tmax[(int64_t)b * A.tiles + blockIdx.x] = mx;
  }
}

__global__ __launch_bounds__(64) void vad_rowmax_kernel(const double *__restrict__ tmax, int tiles,
                                                        double *__restrict__ Pmax) {
  const int b = blockIdx.x;
  double mx = 0.0;
  for (int t = threadIdx.x; t < tiles; t += 64) {
    const double v = tmax[(int64_t)b * tiles + t];
    mx = v > mx ? v : mx;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_xor(mx, o, 64);
    mx = other > mx ? other : mx;
  }
  if (threadIdx.x == 0) Pmax[b] = mx;
}

struct IvArgs {
  const double *P, *Pmax;
  const int64_t *lens;
  int n_max, F_max, hop, min_silence, max_intervals;
  int64_t margin;
  double threshold, floor;
  uint8_t *active;
  int32_t *count;
  int64_t *intervals, *trim;
};

constexpr int kNone = -1, kInf = INT32_MAX;

// One workgroup per row; blockDim.x frames per step. Carried from step to step: the last active frame
// so far (an open run, or an open silence behind it, hangs on it) and the number of runs begun. A run
// begins at an active frame whose previous active frame is missing or min_silence or more inactive
// frames back; the run before it then ends behind that previous active frame. The mask of the inactive
// frames behind the last active one is written once the next active frame (or the row's end) is known.
__global__ __launch_bounds__(256) void vad_intervals_kernel(IvArgs A) {
  __shared__ int wlast[4], wfirst[4], wstarts[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6, b = blockIdx.x;
  const int64_t n = clamp_len(A.lens, b, A.n_max), hop = A.hop;
  const int F = (int)vad_frames(n, hop);
  const double pm = A.Pmax[b];
  const double cut = mul_rn(A.threshold, pm > A.floor ? pm : A.floor);
  const double *P = A.P + (int64_t)b * A.F_max;
  uint8_t *act = A.active + (int64_t)b * A.F_max;
  int64_t *iv = A.intervals + (int64_t)b * A.max_intervals * 2;
  int last = kNone, first = kNone, runs = 0;  // uniform

  for (int c0 = 0; c0 < F; c0 += blockDim.x) {
    const int f = c0 + tid;
    bool a = false;
    if (f < F) {
      const double p = P[f];
      a = (p > A.floor ? p : A.floor) > cut;
    }
    const unsigned long long bal = __ballot(a);
    const unsigned long long below = bal & ((1ull << lane) - 1), above = bal & ~((2ull << lane) - 1);
    const int wb = c0 + w * 64;
    int prev = below ? wb + 63 - __clzll((long long)below) : kNone;
    int next = above ? wb + __ffsll((long long)above) - 1 : kInf;
    __syncthreads();  // the previous step's readers of the three arrays are done
    if (lane == 0) {
      wlast[w] = bal ? wb + 63 - __clzll((long long)bal) : kNone;
      wfirst[w] = bal ? wb + __ffsll((long long)bal) - 1 : kInf;
    }
    __syncthreads();
    for (int v = w - 1; v >= 0 && prev == kNone; --v) prev = wlast[v];
    if (prev == kNone) prev = last;
    for (int v = w + 1; v < nw && next == kInf; ++v) next = wfirst[v];
    int c_last = kNone, c_first = kInf;
    for (int v = 0; v < nw; ++v) {
      c_last = wlast[v] > c_last ? wlast[v] : c_last;
      c_first = wfirst[v] < c_first ? wfirst[v] : c_first;
    }
    const bool start = a && (prev == kNone || f - prev - 1 >= A.min_silence);
    const unsigned long long sbal = __ballot(start);
    if (lane == 0) wstarts[w] = __popcll(sbal);
    __syncthreads();
    int ord = runs + __popcll(sbal & ((1ull << lane) - 1)), total = 0;
    for (int v = 0; v < nw; ++v) {
      if (v < w) ord += wstarts[v];
      total += wstarts[v];
    }
    if (start) {
      if (ord < A.max_intervals) iv[2 * ord] = (int64_t)f * hop;
      if (ord > 0 && ord - 1 < A.max_intervals) {
        const int64_t e = (int64_t)(prev + 1) * hop;
        iv[2 * (ord - 1) + 1] = e < n ? e : n;
      }
    }
    // the mask: final for every frame that has an active frame at or behind it in this step
    if (f < F && (a || next != kInf))
      act[f] = a || (prev != kNone && next - prev - 1 < A.min_silence) ? 1 : 0;
    if (c_last != kNone) {  // uniform: the inactive frames left open by earlier steps, (last, c0)
      const uint8_t fill = last != kNone && c_first - last - 1 < A.min_silence ? 1 : 0;
      for (int g = last + 1 + tid; g < c0; g += blockDim.x) act[g] = fill;
      if (first == kNone) first = c_first;
      last = c_last;
    }
    runs += total;
  }
  // behind the last active frame, and the padding from F on
  for (int g = last + 1 + tid; g < A.F_max; g += blockDim.x) act[g] = 0;
  for (int i = (runs < A.max_intervals ? runs : A.max_intervals) * 2 + tid; i < A.max_intervals * 2; i += blockDim.x)
    iv[i] = 0;
  if (tid == 0) {
    A.count[b] = runs;
    int64_t s = 0, e = 0;
    if (last != kNone) {
      const int64_t end_run = (int64_t)(last + 1) * hop;
      if (runs - 1 < A.max_intervals) iv[2 * (runs - 1) + 1] = end_run < n ? end_run : n;
      s = (int64_t)first * hop - A.margin;
      s = s < 0 ? 0 : s;
      e = end_run + A.margin;
      e = e < n ? e : n;
    }
    A.trim[2 * b] = s;
    A.trim[2 * b + 1] = e;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void vad_cut_kernel(const T *__restrict__ wav, int64_t stride,
                                                      const int64_t *__restrict__ trim, int n_max, int M_max,
                                                      T *__restrict__ out, int64_t *__restrict__ out_lens) {
  const int b = blockIdx.y;
  int64_t s = trim[2 * b], e = trim[2 * b + 1];
  s = s < 0 ? 0 : (s > n_max ? n_max : s);
  e = e < s ? s : (e > n_max ? n_max : e);
  e = e - s > M_max ? s + M_max : e;
  const int64_t len = e - s;
  const T *x = wav + (int64_t)b * stride + s;
  T *o = out + (int64_t)b * M_max;
  for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M_max; m += (int64_t)gridDim.x * blockDim.x)
    o[m] = m < len ? x[m] : (T)0;
  if (out_lens != nullptr && blockIdx.x == 0 && threadIdx.x == 0) out_lens[b] = len;
}

}  // namespace

extern "C" int64_t fs2_vad_frames(int64_t n, int64_t hop) { return hop < 1 ? -1 : vad_frames(n, hop); }

extern "C" int64_t fs2_vad_workspace_bytes(int64_t B, int64_t F_max, int64_t frame_length, int64_t hop) {
  return vad_workspace_bytes(B, F_max, frame_length, hop);
}

extern "C" int64_t fs2_vad_lds_bytes(int64_t frame_length, int64_t hop) { return vad_lds_bytes(frame_length, hop); }

extern "C" int fs2_vad_power(const void *wav, int dtype, int64_t row_stride, const int64_t *lens, int B, int n_max,
                             int frame_length, int hop, double *P, double *Pmax, void *workspace,
                             int64_t workspace_bytes, fs2_stream_t stream) {
  if (wav == nullptr || P == nullptr || Pmax == nullptr || workspace == nullptr) return FS2_EINVAL;
  const int rc = vad_check(B, n_max, frame_length, hop);
  if (rc != FS2_OK) return rc;
  if (row_stride < n_max) return FS2_EINVAL;
  if (dtype != FS2_I16 && dtype != FS2_F32) return FS2_EUNSUPPORTED;
  PowArgs a;
  a.stride = row_stride;
  a.lens = lens;
  a.n_max = n_max;
  a.F_max = (int)vad_frames(n_max, hop);
  if (workspace_bytes < vad_workspace_bytes(B, a.F_max, frame_length, hop)) return FS2_EINVAL;
  const int64_t esize = dtype == FS2_I16 ? 2 : 4;
  a.L = frame_length;
  a.hop = hop;
  a.g = (int)vad_gcd(frame_length, hop);
  a.q = frame_length / a.g;
  a.h = hop / a.g;
  a.G = (int)vad_tile_frames(frame_length, hop);
  a.nb = (int)vad_tile_blocks(frame_length, hop, a.G);
  a.gs = (int)vad_row_stride(a.g, esize);
  a.pb = (int)(FS2_VAD_AREA_BYTES / esize / a.gs);  // >= 1: vad_check
  a.lev_leaf = bit_length((unsigned)((a.g + kLeaf - 1) / kLeaf));
  a.lev_q = bit_length((unsigned)a.q);
  if (a.G < 1 || a.nb > FS2_VAD_SUMS_MAX || a.pb < 1 || a.lev_leaf > kLev || a.lev_q > kLev) return FS2_EUNSUPPORTED;
  a.tiles = (int)vad_tiles(a.F_max, frame_length, hop);
  a.P = P;
  a.tmax = static_cast<double *>(workspace);
  const dim3 grid((unsigned)a.tiles, (unsigned)B);
  if (dtype == FS2_I16)
    hipLaunchKernelGGL(vad_power_kernel<int16_t>, grid, dim3(kNT), 0, as_stream(stream),
                       static_cast<const int16_t *>(wav), a);
  else
    hipLaunchKernelGGL(vad_power_kernel<float>, grid, dim3(kNT), 0, as_stream(stream), static_cast<const float *>(wav),
                       a);
  FS2_CHECK_LAUNCH();
  hipLaunchKernelGGL(vad_rowmax_kernel, dim3((unsigned)B), dim3(64), 0, as_stream(stream), a.tmax, a.tiles, Pmax);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_vad_intervals(const double *P, const double *Pmax, const int64_t *lens, int B, int n_max, int hop,
                                 double threshold, double floor, int min_silence, int64_t margin, int max_intervals,
                                 int chunk_frames, uint8_t *active, int32_t *count, int64_t *intervals, int64_t *trim,
                                 fs2_stream_t stream) {
  if (P == nullptr || Pmax == nullptr || active == nullptr || count == nullptr || trim == nullptr) return FS2_EINVAL;
  if (B < 1 || n_max < 1 || hop < 1 || min_silence < 1 || margin < 0 || max_intervals < 0) return FS2_EINVAL;
  if (intervals == nullptr && max_intervals > 0) return FS2_EINVAL;
  if (!(threshold >= 0.0) || !(floor >= 0.0)) return FS2_EINVAL;
  if (chunk_frames == 0) chunk_frames = FS2_VAD_CHUNK_FRAMES;
  if (chunk_frames != 64 && chunk_frames != 128 && chunk_frames != 256) return FS2_EINVAL;
  if (B > FS2_VAD_B_MAX) return FS2_EUNSUPPORTED;
  const int64_t F_max = vad_frames(n_max, hop);
  if (F_max > INT32_MAX || (int64_t)B * F_max > INT32_MAX / 8 || (int64_t)B * max_intervals > INT32_MAX / 16)
    return FS2_EUNSUPPORTED;
  IvArgs a;
  a.P = P;
  a.Pmax = Pmax;
  a.lens = lens;
  a.n_max = n_max;
  a.F_max = (int)F_max;
  a.hop = hop;
  a.min_silence = min_silence;
  a.max_intervals = max_intervals;
  a.margin = margin;
  a.threshold = threshold;
  a.floor = floor;
  a.active = active;
  a.count = count;
  a.intervals = intervals;
  a.trim = trim;
  hipLaunchKernelGGL(vad_intervals_kernel, dim3((unsigned)B), dim3((unsigned)chunk_frames), 0, as_stream(stream), a);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_vad_cut(const void *wav, int dtype, int64_t row_stride, const int64_t *trim, int B, int n_max,
                           int M_max, void *out, int64_t *out_lens, fs2_stream_t stream) {
  if (wav == nullptr || trim == nullptr || out == nullptr) return FS2_EINVAL;
  if (B < 1 || n_max < 1 || M_max < 1 || row_stride < n_max) return FS2_EINVAL;
  if (dtype != FS2_I16 && dtype != FS2_F32) return FS2_EUNSUPPORTED;
  if (B > FS2_VAD_B_MAX) return FS2_EUNSUPPORTED;
  const int64_t want = ((int64_t)M_max + 256 * 8 - 1) / (256 * 8);
  const dim3 grid((unsigned)(want < 1024 ? want : 1024), (unsigned)B);
  if (dtype == FS2_I16)
    hipLaunchKernelGGL(vad_cut_kernel<int16_t>, grid, dim3(256), 0, as_stream(stream),
                       static_cast<const int16_t *>(wav), row_stride, trim, n_max, M_max, static_cast<int16_t *>(out),
                       out_lens);
  else
    hipLaunchKernelGGL(vad_cut_kernel<float>, grid, dim3(256), 0, as_stream(stream), static_cast<const float *>(wav),
                       row_stride, trim, n_max, M_max, static_cast<float *>(out), out_lens);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}
