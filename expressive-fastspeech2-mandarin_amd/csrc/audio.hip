// Waveform -> log-mel + energy on CDNA4 (include/fs2hip_audio.h): TacotronSTFT.mel_spectrogram
// (audio/stft.py:130-178) as one launch, and the phoneme-level segment mean
// (preprocessor/preprocessor.py:293-302).
//
// mel kernel: one workgroup (4 waves) takes kTile = 64 consecutive frames of ONE utterance.
//   1. The frames' signal span (63*256 + 1024 samples) is staged once in LDS, reflect-padded at the
//      utterance's own ends by index arithmetic, clipped (f32) or scaled (int16) on the way in.
//      Every 256 samples are followed by 4 pad floats, so that the 32 lanes of an operand read
//      (one frame each, 256 samples apart) fall in distinct LDS banks with 16-byte reads.
//   2. STFT as specT[bin][frame] = basis[bin][k] * frame[k]: v_mfma_f32_32x32x2_f32 with the
//      basis as A (streamed from L2, a full 128-byte line per row per 32-k block) and the frames
//      as B (read from LDS at stride hop). A wave owns bin tiles w, w+4, w+8, w+12 (32 bins each)
//      and holds the re and im accumulators of the same bins for both 32-frame halves: one lane
//      has re and im of the same (bin, frame), the magnitude needs no exchange.
//      Inside a 32-k block MFMA q pairs k = kb+q (lanes 0-31) with k = kb+16+q (lanes 32-63), so a
//      lane reads 16 consecutive floats of its row: a fixed permutation of the summation order.
//   3. The magnitude tile has its bins in the 16 accumulator registers and its frame on the lane:
//      it is the B operand of melT[m][frame] += mel_basis[m][bin] * mag[bin][frame] as it stands
//      (no LDS, no lane movement); the wave accumulates its bins' share of the 80 bands (3 tiles
//      of 32 rows, rows >= 80 are zero operands) and of the energy's sum of squares.
//   4. The Nyquist bin (512) is a VALU dot product over the staged span (4 threads per frame).
//   5. The four waves' mel shares are added in wave order in LDS (over the dead signal span), then
//      the Nyquist share, then log(max(., clip)); rows go out coalesced, channels-last.
// Nothing in 1-5 depends on B, the batch slot, n_max or the row stride.
#include <math.h>

#include "fs2_common.h"
#include "fs2hip_audio.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kNfft = 1024, kHop = 256, kBins = kNfft / 2 + 1, kMel = 80;
constexpr int kTile = 64;                              // frames per workgroup
constexpr int kSpan = (kTile - 1) * kHop + kNfft;      // samples a tile reads
constexpr int kSigLds = kSpan + (kSpan >> 8) * 4 + 4;  // with 4 pad floats per 256 samples
constexpr int kMelLd = kMel + 1;                       // LDS row of the mel reduction
constexpr int kMelLds = kTile * kMelLd;                // [frame][band]
constexpr int kELds = 4 * 2 * kTile;                   // energy shares [wave][lane half][frame]
static_assert(kMelLds + kELds + kTile <= kSigLds, "the reduction buffers alias the signal span");

__device__ __forceinline__ int sig_idx(int s) { return s + ((s >> 8) << 2); }

// row (of a 32-row MFMA result tile) held in accumulator register r by lane half h
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

template <bool I16>
__global__ __launch_bounds__(256) void mel_kernel(const void *__restrict__ wav, int64_t wav_stride,
                                                  const int64_t *__restrict__ lens, int n_max, int T_out,
                                                  float inv_max, const float *__restrict__ basis,
                                                  const float *__restrict__ melb, float clip_val, float log_clip,
                                                  float *__restrict__ mel, float *__restrict__ energy,
                                                  float *__restrict__ mag, int64_t *__restrict__ frames_out) {
  __shared__ __attribute__((aligned(16))) float sm[kSigLds];
  const int b = blockIdx.y, t0 = blockIdx.x * kTile;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int j = lane & 31, h = lane >> 5;

  int64_t len64 = lens != nullptr ? lens[b] : (int64_t)n_max;
  const int len = (int)(len64 < 0 ? 0 : (len64 > n_max ? n_max : len64));
  const int nfr = len > kNfft / 2 ? 1 + len / kHop : 0;
  if (blockIdx.x == 0 && tid == 0 && frames_out != nullptr) frames_out[b] = nfr;
  const int t_valid = min(nfr, T_out);            // rows [0, t_valid) carry data
  const int t_end = min(t0 + kTile, T_out);       // this tile's rows are [t0, t_end)
  const int64_t row0 = (int64_t)b * T_out + t0;

  if (t0 >= t_valid) {  // a tile of padding rows only (block-uniform)
    const int rows = t_end - t0;
    for (int e = tid; e < rows * kMel; e += 256) mel[row0 * kMel + e] = 0.0f;
    for (int e = tid; e < rows; e += 256) energy[row0 + e] = 0.0f;
    if (mag != nullptr)
      for (int e = tid; e < rows * kBins; e += 256) mag[row0 * kBins + e] = 0.0f;
    return;
  }

  // 1. stage the span; sample p of the span is padded-signal index t0*hop + p, i.e. sample
  //    s = t0*hop + p - n_fft/2 of the utterance, reflected at 0 and at len-1 (len > n_fft/2, so
  //    one reflection suffices for every valid frame; what a padding frame would read past that
  //    is 0 and its results are dropped)
  {
    const int64_t wbase = (int64_t)b * wav_stride;
    for (int p = tid; p < kSpan; p += 256) {
      int64_t s = (int64_t)t0 * kHop + p - kNfft / 2;
      if (s < 0) s = -s;
      if (s >= len) s = 2 * (int64_t)(len - 1) - s;
      float v = 0.0f;
      if (s >= 0 && s < len) {
        if constexpr (I16) {
          v = (float)reinterpret_cast<const int16_t *>(wav)[wbase + s] * inv_max;
        } else {
          v = reinterpret_cast<const float *>(wav)[wbase + s];
          v = fminf(fmaxf(v, -1.0f), 1.0f);
        }
      }
      sm[sig_idx(p)] = v;
    }
  }
  __syncthreads();

  // 4. (early, while the span is live) the Nyquist bin: thread -> (frame tid>>2, quarter tid&3)
  float nyq;
  {
    const int fr = tid >> 2, part = tid & 3;
    const float4 *bre = reinterpret_cast<const float4 *>(basis + (int64_t)(kBins - 1) * kNfft + part * 256);
    const float4 *bim = reinterpret_cast<const float4 *>(basis + (int64_t)(2 * kBins - 1) * kNfft + part * 256);
    const float *x = sm + sig_idx(fr * kHop + part * 256);
    float re = 0.0f, im = 0.0f;
#pragma unroll 4
    for (int q = 0; q < 64; ++q) {
      const float4 xv = *reinterpret_cast<const float4 *>(x + 4 * q);
      const float4 r4 = bre[q], i4 = bim[q];
      re = fmaf(r4.x, xv.x, re); re = fmaf(r4.y, xv.y, re); re = fmaf(r4.z, xv.z, re); re = fmaf(r4.w, xv.w, re);
      im = fmaf(i4.x, xv.x, im); im = fmaf(i4.y, xv.y, im); im = fmaf(i4.z, xv.z, im); im = fmaf(i4.w, xv.w, im);
    }
    re += __shfl_xor(re, 1, 64); re += __shfl_xor(re, 2, 64);
    im += __shfl_xor(im, 1, 64); im += __shfl_xor(im, 2, 64);
    nyq = sqrtf(re * re + im * im);
    if (mag != nullptr && part == 0 && t0 + fr < t_valid) mag[(row0 + fr) * kBins + (kBins - 1)] = nyq;
  }

  // 2 + 3. bin tiles
  f32x16 macc[2][3];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int mt = 0; mt < 3; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) macc[f][mt][r] = 0.0f;
  float esum[2] = {0.0f, 0.0f};

  const float *x0 = sm + sig_idx(j * kHop) + 16 * h;          // frame j of half 0; + kb (+ pad) per block
  const float *x1 = sm + sig_idx((32 + j) * kHop) + 16 * h;   // frame 32 + j
  for (int bt = wid; bt < (kBins - 1) / 32; bt += 4) {
    const int bin0 = bt * 32;
    const float4 *are = reinterpret_cast<const float4 *>(basis + (int64_t)(bin0 + j) * kNfft + 16 * h);
    const float4 *aim = reinterpret_cast<const float4 *>(basis + (int64_t)(kBins + bin0 + j) * kNfft + 16 * h);
    f32x16 cre[2], cim[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) cre[0][r] = cre[1][r] = cim[0][r] = cim[1][r] = 0.0f;
    float4 ar[4], ai[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { ar[c] = are[c]; ai[c] = aim[c]; }
    for (int kb = 0; kb < kNfft; kb += 32) {
      float4 nr[4], ni[4];
      const int kn = kb + 32 < kNfft ? kb + 32 : kb;  // the last block reloads itself (unused)
#pragma unroll
      for (int c = 0; c < 4; ++c) { nr[c] = are[(kn >> 2) + c]; ni[c] = aim[(kn >> 2) + c]; }
      const int ko = kb + ((kb >> 8) << 2);  // j*hop + kb + 16h never crosses a 256 boundary inside a block
      float4 b0[4], b1[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        b0[c] = *reinterpret_cast<const float4 *>(x0 + ko + 4 * c);
        b1[c] = *reinterpret_cast<const float4 *>(x1 + ko + 4 * c);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float a_re[4] = {ar[c].x, ar[c].y, ar[c].z, ar[c].w}, a_im[4] = {ai[c].x, ai[c].y, ai[c].z, ai[c].w};
        const float v0[4] = {b0[c].x, b0[c].y, b0[c].z, b0[c].w}, v1[4] = {b1[c].x, b1[c].y, b1[c].z, b1[c].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          cre[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_re[e], v0[e], cre[0], 0, 0, 0);
          cim[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_im[e], v0[e], cim[0], 0, 0, 0);
          cre[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_re[e], v1[e], cre[1], 0, 0, 0);
          cim[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_im[e], v1[e], cim[1], 0, 0, 0);
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) { ar[c] = nr[c]; ai[c] = ni[c]; }
    }
    // magnitudes of (bin0 + acc_row(r, h), frame 32f + j); mel and energy shares
    float mg[2][16];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float m = sqrtf(cre[f][r] * cre[f][r] + cim[f][r] * cim[f][r]);
        mg[f][r] = m;
        esum[f] = fmaf(m, m, esum[f]);
      }
    if (mag != nullptr) {
#pragma unroll
      for (int f = 0; f < 2; ++f)
        if (t0 + 32 * f + j < t_valid) {
          float *mo = mag + (row0 + 32 * f + j) * kBins + bin0;
#pragma unroll
          for (int r = 0; r < 16; ++r) mo[acc_row(r, h)] = mg[f][r];
        }
    }
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) {
      const int m = 32 * mt + j;  // A row: mel band (rows >= 80 are zero)
      const float *mb = melb + (int64_t)(m < kMel ? m : 0) * kBins + bin0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float a = m < kMel ? mb[acc_row(r, h)] : 0.0f;
        macc[0][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, mg[0][r], macc[0][mt], 0, 0, 0);
        macc[1][mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, mg[1][r], macc[1][mt], 0, 0, 0);
      }
    }
  }

  // 5. reduce the waves' shares in wave order over the dead span
  float *melS = sm, *eS = sm + kMelLds, *nyqS = sm + kMelLds + kELds;
  __syncthreads();
  for (int w = 0; w < 4; ++w) {
    if (wid == w) {
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int mt = 0; mt < 3; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = 32 * mt + acc_row(r, h);
            if (m < kMel) {
              float *p = melS + (32 * f + j) * kMelLd + m;
              *p = w == 0 ? macc[f][mt][r] : *p + macc[f][mt][r];
            }
          }
      eS[(w * 2 + h) * kTile + j] = esum[0];
      eS[(w * 2 + h) * kTile + 32 + j] = esum[1];
    }
    __syncthreads();
  }
  if ((tid & 3) == 0) nyqS[tid >> 2] = nyq;
  __syncthreads();

  for (int e = tid; e < (t_end - t0) * kMel; e += 256) {
    const int fr = e / kMel, m = e - fr * kMel;
    float o = 0.0f;
    if (t0 + fr < t_valid) {
      const float lin = fmaf(melb[(int64_t)m * kBins + (kBins - 1)], nyqS[fr], melS[fr * kMelLd + m]);
      o = lin <= clip_val ? log_clip : logf(lin);
    }
    mel[row0 * kMel + e] = o;
  }
  if (tid < t_end - t0) {
    float o = 0.0f;
    if (t0 + tid < t_valid) {
      float s = 0.0f;
#pragma unroll
      for (int q = 0; q < 8; ++q) s += eS[q * kTile + tid];
      o = sqrtf(fmaf(nyqS[tid], nyqS[tid], s));
    }
    energy[row0 + tid] = o;
  }
  if (mag != nullptr) {  // padding rows inside a tile that has data
    const int first = t_valid - t0;  // >= 1
    for (int e = first * kBins + tid; e < (t_end - t0) * kBins; e += 256) mag[row0 * kBins + e] = 0.0f;
  }
}

// One wave per utterance: exclusive scan of the durations (each lane a contiguous chunk, the
// idiom of lr_durations_kernel), then each lane sums its phonemes' frames left to right.
__global__ __launch_bounds__(64) void segment_mean_kernel(const float *__restrict__ values,
                                                          const int64_t *__restrict__ dur, int T, int L,
                                                          float *__restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int per = (L + 63) / 64;
  const int i0 = min(lane * per, L), i1 = min(i0 + per, L);
  const int64_t *d = dur + (int64_t)b * L;
  const float *v = values + (int64_t)b * T;
  int64_t local = 0;
  for (int i = i0; i < i1; ++i) local += d[i] > 0 ? d[i] : 0;
  int64_t incl = local;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    int64_t y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  int64_t run = incl - local;
  for (int i = i0; i < i1; ++i) {
    const int64_t di = d[i] > 0 ? d[i] : 0;
    const int64_t s0 = run < T ? run : T, s1 = run + di < T ? run + di : T;
    float s = 0.0f;
    for (int64_t t = s0; t < s1; ++t) s += v[t];
    out[(int64_t)b * L + i] = s1 > s0 ? s / (float)(s1 - s0) : 0.0f;
    run += di;
  }
}

}  // namespace

extern "C" int fs2_mel_spectrogram(const fs2_mel_desc *d, fs2_stream_t stream) {
  if (d == nullptr || d->wav == nullptr || d->basis == nullptr || d->mel_basis == nullptr || d->mel == nullptr ||
      d->energy == nullptr)
    return FS2_EINVAL;
  if (d->B < 1 || d->n_max < 1 || d->T_out < 1 || d->wav_row_stride < d->n_max || !(d->clip_val > 0.0f))
    return FS2_EINVAL;
  if (d->wav_dtype != FS2_F32 && d->wav_dtype != FS2_I16) return FS2_EINVAL;
  if (d->wav_dtype == FS2_I16 && !(d->max_wav_value > 0.0f)) return FS2_EINVAL;
  if (d->n_fft != kNfft || d->win != kNfft || d->hop != kHop || d->n_mel != kMel) return FS2_EUNSUPPORTED;
  if (d->B > 65535) return FS2_EUNSUPPORTED;
  // T_out against every frame count the host can see
  if (d->lens_host != nullptr) {
    for (int b = 0; b < d->B; ++b) {
      int64_t n = d->lens_host[b];
      n = n < 0 ? 0 : (n > d->n_max ? d->n_max : n);
      if (n > kNfft / 2 && 1 + n / kHop > d->T_out) return FS2_EINVAL;
    }
  } else if (d->lens == nullptr) {
    if (d->n_max > kNfft / 2 && 1 + d->n_max / kHop > d->T_out) return FS2_EINVAL;
  }
  const float log_clip = (float)log((double)d->clip_val);
  dim3 grid((d->T_out + kTile - 1) / kTile, d->B);
  hipStream_t s = as_stream(stream);
  if (d->wav_dtype == FS2_I16)
    hipLaunchKernelGGL(mel_kernel<true>, grid, dim3(256), 0, s, d->wav, d->wav_row_stride, d->lens, d->n_max, d->T_out,
                       1.0f / d->max_wav_value, d->basis, d->mel_basis, d->clip_val, log_clip, d->mel, d->energy,
                       d->mag, d->frames_out);
  else
    hipLaunchKernelGGL(mel_kernel<false>, grid, dim3(256), 0, s, d->wav, d->wav_row_stride, d->lens, d->n_max,
                       d->T_out, 1.0f, d->basis, d->mel_basis, d->clip_val, log_clip, d->mel, d->energy, d->mag,
                       d->frames_out);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_segment_mean(const float *values, const int64_t *dur, int B, int T, int L, float *out,
                                fs2_stream_t stream) {
  if (values == nullptr || dur == nullptr || out == nullptr || B < 1 || T < 1 || L < 1) return FS2_EINVAL;
  hipLaunchKernelGGL(segment_mean_kernel, dim3(B), dim3(64), 0, as_stream(stream), values, dur, T, L, out);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}
