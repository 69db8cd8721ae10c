// Raw audio to corpus waveforms (include/fs2hip_resample.h): the rational polyphase FIR resampler in
// float64, bit for bit scipy.signal.resample_poly, with the peak of its f32 rounding, and the peak
// normalisation to int16. Persistent workgroups stage the whole tap table once in LDS and walk tiles
// of the ragged batch; an output is one thread's sequential multiply / add chain.
#include "fs2_common.h"
#include "fs2hip_audio.h"
#include "resample_sizes.h"

// No a * b + c may become an FMA anywhere in this file: the operations the header names go through
// the helpers below, defined HERE under the pragma (csrc/prep.hip explains why __dadd_rn is not enough).
#pragma clang fp contract(off)

namespace {

constexpr int kNT = 512;           // threads per workgroup: 8 waves; two workgroups per CU fit the LDS
constexpr int kPer = 4;            // outputs per thread and tile, kNT apart: a wave's stores stay contiguous
constexpr int kTile = kNT * kPer;  // outputs per tile
constexpr int kPerCU = 2;
constexpr int kAhead = 8;          // terms of an output fetched together

__device__ __forceinline__ double add_rn(double a, double b) { return a + b; }
__device__ __forceinline__ double mul_rn(double a, double b) { return a * b; }
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ double div_rn(double a, double b) { return a / b; }  // IEEE: no fast-math here

struct RsArgs {
  int64_t stride;
  const int64_t *lens;
  const double *taps;
  int B, n_max, up, down, n_taps, fir;
  int stage_x;    // the tile's input span is staged in LDS behind the taps
  int x_off;      // where it starts, in f64 elements
  int64_t x_cap;  // samples it holds
  int64_t M_max, tiles, items;
  double *y;
  float *y32;
  unsigned *peak;  // the bits of a non-negative float: they order as the floats do
  int64_t *out_lens;
};

__device__ __forceinline__ int64_t clamp_len(const int64_t *lens, int b, int n_max) {
  const int64_t nl = lens != nullptr ? lens[b] : n_max;
  return nl < 0 ? 0 : (nl > n_max ? n_max : nl);
}

// One output: the terms lo .. hi in ascending order. src[i - off] is sample i: the utterance's row in
// global memory (off 0) or the tile's span staged in LDS. kAhead terms at a time: their samples and
// taps are fetched before the first is added, so that the chain of adds waits for memory once per
// group, not once per term.
template <typename T>
__device__ __forceinline__ double fir_output(const T *src, int64_t off, const double *H, const RsRange r, int up) {
  double acc = 0.0;
  int k = (int)(r.c - r.lo * up);  // in [0, 2 * half] whenever lo <= hi
  const int n_terms = (int)(r.hi - r.lo + 1);
  src += r.lo - off;
  for (int t = 0; t < n_terms; t += kAhead, k -= kAhead * up) {
    double xv[kAhead], hv[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      // past the last term: fetch the last term again (a valid address, no branch); it is not added
      const int dj = t + j < n_terms ? j : n_terms - 1 - t;
      const int kj = k - dj * up;
      xv[j] = (double)src[t + dj];
      hv[j] = H[kj + (kj >> FS2_RS_PAD_SHIFT)];
    }
#pragma unroll
    for (int j = 0; j < kAhead; ++j)
      if (t + j < n_terms) acc = add_rn(acc, mul_rn(hv[j], xv[j]));
  }
  return acc;
}

template <typename T>
__global__ __launch_bounds__(kNT) void resample_kernel(const T *__restrict__ wav, RsArgs A) {
  __shared__ double H[FS2_RESAMPLE_LDS_BYTES / 8];  // the padded taps, then the tile's input span
  const int tid = threadIdx.x;
  const int64_t up = A.up, down = A.down, half = rs_half(up, down);
  T *X = reinterpret_cast<T *>(H + A.x_off);
  if (A.fir) {
    for (int k = tid; k < A.n_taps; k += kNT) H[rs_slot(k)] = A.taps[k];
    __syncthreads();
  }
  if (blockIdx.x == 0 && A.out_lens != nullptr)
    for (int b = tid; b < A.B; b += kNT) A.out_lens[b] = rs_out_len(clamp_len(A.lens, b, A.n_max), up, down);

  for (int64_t item = blockIdx.x; item < A.items; item += gridDim.x) {  // uniform
    const int b = (int)(item / A.tiles);
    const int64_t m0 = (item - (int64_t)b * A.tiles) * kTile;
    const int64_t n = clamp_len(A.lens, b, A.n_max), M = rs_out_len(n, up, down);
    const T *x = wav + (int64_t)b * A.stride;
    const int64_t row = (int64_t)b * A.M_max;
    int64_t s0 = 0;
    if (A.stage_x && m0 < M) {  // uniform: the samples the tile's outputs read, m0's first to the last one's last
      const int64_t m1 = (m0 + kTile < M ? m0 + kTile : M) - 1;
      s0 = rs_range(m0, n, up, down, half).lo;
      int64_t cnt = rs_range(m1, n, up, down, half).hi - s0 + 1;
      cnt = cnt > A.x_cap ? A.x_cap : cnt;  // never taken: rs_span bounds the span
      __syncthreads();                      // the previous tile's readers are done
      for (int p = tid; p < cnt; p += kNT) X[p] = x[s0 + p];
      __syncthreads();
    }
    unsigned pk = 0;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int64_t m = m0 + u * kNT + tid;
      if (m >= A.M_max) break;
      double acc = 0.0;
      if (m < M) {
        if (A.stage_x)
          acc = fir_output<T>(X, s0, H, rs_range(m, n, up, down, half), A.up);
        else if (A.fir)
          acc = fir_output<T>(x, 0, H, rs_range(m, n, up, down, half), A.up);
        else
          acc = (double)x[m];
      }
      const float a32 = (float)acc;
      if (A.y != nullptr) A.y[row + m] = acc;
      A.y32[row + m] = a32;
      const unsigned bits = __float_as_uint(a32) & 0x7fffffffu;
      pk = bits > pk ? bits : pk;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned other = (unsigned)__shfl_xor((int)pk, o, 64);
      pk = other > pk ? other : pk;
    }
    if ((tid & 63) == 0 && pk != 0) atomicMax(A.peak + b, pk);
  }
}

__global__ __launch_bounds__(256) void peak_int16_kernel(const float *__restrict__ y32, const float *__restrict__ peak,
                                                         const int64_t *__restrict__ out_lens, int M_max,
                                                         float max_wav_value, int16_t *__restrict__ q) {
  const int b = blockIdx.y;
  const float pk = peak[b];
  int64_t M = out_lens != nullptr ? out_lens[b] : M_max;
  M = M < 0 ? 0 : (M > M_max ? M_max : M);
  if (!(pk > 0.0f)) M = 0;  // silence, an empty utterance (and a NaN peak: out of contract): zeros
  const int64_t row = (int64_t)b * M_max;
  const double pkd = (double)pk;
  for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M_max; m += (int64_t)gridDim.x * blockDim.x) {
    int o = 0;
    if (m < M) {
      const float quot = (float)div_rn((double)y32[row + m], pkd);  // the correctly rounded f32 quotient
      const float v = mul_rn(quot, max_wav_value);
      o = v >= 32767.0f ? 32767 : (v <= -32768.0f ? -32768 : (v == v ? (int)v : 0));
    }
    q[row + m] = (int16_t)o;
  }
}

// Compute units of the current device (cached per device id).
int rs_num_cus() {
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

}  // namespace

extern "C" int64_t fs2_resample_out_len(int64_t n, int64_t up, int64_t down) {
  return up < 1 || down < 1 ? -1 : rs_out_len(n, up, down);
}

extern "C" int64_t fs2_resample_lds_bytes(int64_t up, int64_t down) {
  return up < 1 || down < 1 ? 0 : rs_lds_bytes(up, down);
}

extern "C" int fs2_resample(const void *wav, int dtype, int64_t row_stride, const int64_t *lens, int B, int n_max,
                            int up, int down, const double *taps, int n_taps, double *y, float *y32, float *peak,
                            int64_t *out_lens, fs2_stream_t stream) {
  if (wav == nullptr || y32 == nullptr || peak == nullptr) return FS2_EINVAL;
  if (B < 1 || n_max < 1 || row_stride < n_max) return FS2_EINVAL;
  const int rc = rs_check(n_max, up, down, n_taps);
  if (rc != FS2_OK) return rc;
  const bool fir = !(up == 1 && down == 1);
  if (fir && taps == nullptr) return FS2_EINVAL;
  if (dtype != FS2_I16 && dtype != FS2_F32) return FS2_EUNSUPPORTED;
  RsArgs a;
  a.stride = row_stride;
  a.lens = lens;
  a.taps = taps;
  a.B = B;
  a.n_max = n_max;
  a.up = up;
  a.down = down;
  a.n_taps = n_taps;
  a.fir = fir ? 1 : 0;
  // behind the taps the LDS holds the input span of a tile, where it fits; otherwise (a float32
  // batch at a large down / up) the samples are read from global memory: the same bits either way
  const int64_t esize = dtype == FS2_I16 ? 2 : 4;
  a.x_off = fir ? (int)(rs_lds_bytes(up, down) / 8) : 0;
  a.x_cap = (FS2_RESAMPLE_LDS_BYTES - 8 * (int64_t)a.x_off) / esize;
  a.stage_x = fir && rs_span(kTile, up, down) <= a.x_cap ? 1 : 0;
  a.M_max = rs_out_len(n_max, up, down);
  a.tiles = (a.M_max + kTile - 1) / kTile;
  a.items = a.tiles * B;
  a.y = y;
  a.y32 = y32;
  a.peak = reinterpret_cast<unsigned *>(peak);
  a.out_lens = out_lens;
  const int cus = rs_num_cus();
  const int64_t slots = (int64_t)(cus > 0 ? cus : 256) * kPerCU;
  const dim3 grid((unsigned)(a.items < slots ? a.items : slots));
  if (hipMemsetAsync(peak, 0, sizeof(float) * (size_t)B, as_stream(stream)) != hipSuccess) return FS2_ELAUNCH;
  if (dtype == FS2_I16)
    hipLaunchKernelGGL(resample_kernel<int16_t>, grid, dim3(kNT), 0, as_stream(stream),
                       static_cast<const int16_t *>(wav), a);
  else
    hipLaunchKernelGGL(resample_kernel<float>, grid, dim3(kNT), 0, as_stream(stream), static_cast<const float *>(wav),
                       a);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_peak_int16(const float *y32, const float *peak, const int64_t *out_lens, int B, int M_max,
                              float max_wav_value, int16_t *q, fs2_stream_t stream) {
  if (y32 == nullptr || peak == nullptr || q == nullptr) return FS2_EINVAL;
  if (B < 1 || M_max < 1) return FS2_EINVAL;
  if (B > 65535) return FS2_EUNSUPPORTED;
  const int64_t want = ((int64_t)M_max + 256 * 8 - 1) / (256 * 8);  // about eight samples per thread
  const dim3 grid((unsigned)(want < 1024 ? want : 1024), B);
  hipLaunchKernelGGL(peak_int16_kernel, grid, dim3(256), 0, as_stream(stream), y32, peak, out_lens, M_max,
                     max_wav_value, q);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}
