// Waveform <-> spectrum on CDNA4 (include/fs2hip_audio_inv.h): STFT.transform with its full
// spectrum, STFT.inverse (audio/stft.py:52-122) and the two launches of a Griffin-Lim iteration
// (audio/audio_processing.py:66-82). Exact f32 on v_mfma_f32_32x32x2_f32, like audio.hip.
//
// stft kernel: the staging and spectrum pass of audio.hip's mel kernel (one workgroup per 64 frames
//   of ONE utterance, reflection by index arithmetic, basis as the A operand from L2), kept
//   separate so that the mel kernel's registers and LDS stay what they are. The spectrum comes out
//   transposed, specT[bin][frame], with the frame on the lane: bin-major rows [B, 1026 | 513, T_out]
//   store as 128-byte lines. It does not clip unless asked, and it can project the spectrum onto
//   target magnitudes in its epilogue (recomb = m z / |z|, no atan2 / cos / sin). The 1024-term sum
//   is two-level (four quarters of 256 in the MFMA chain, added in order), which halves its
//   distance from float64; the Nyquist bin's VALU sum has four partial sums already.
//
// istft kernel: the overlap-add as a gather. Output hop block jo (256 samples, ola block jo + 2)
//   and phase r:   out[jo, r] = sum_g sum_{q=0..3} sum_{c in group g} recomb[c, jo + 2 - q] * inv[c, 256 q + r]
//   One workgroup (4 waves) takes 64 hop blocks of ONE utterance times all 256 phases; a wave owns
//   64 phases (2 tiles) x 64 blocks (2 tiles) = 64 accumulator registers. The MFMA rows are the hop
//   blocks and its columns the phases, so that an accumulator register holds 32 consecutive
//   samples over the lanes and stores as a 128-byte line. The recomb operand is staged in LDS in
//   chunks of 24 channels x 67 frames (the tile's frames with a 3-frame halo), double-buffered: the
//   next chunk is loaded into registers before the current one's 192 MFMAs and written after
//   them. A lane group of an operand read (ds_read_b32, 32 lanes) takes 32 consecutive floats of one
//   channel row: conflict-free. The inverse basis is read from L2,
//   repacked on the host so that a lane reads one float4 (its phase, 4 channel pairs) per step
//   and a wave 2 KB contiguous; the next step's two float4 are in flight during the current MFMAs.
//   Frames outside [0, T) are staged as 0. The sum is two-level: a chunk's 96 terms in the MFMA
//   chain, the 43 chunk sums added in chunk order; the order (chunk, group, q, channel pair) is fixed.
#include <math.h>

#include "fs2_common.h"
#include "fs2hip_audio_inv.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kNfft = 1024, kHop = 256, kBins = kNfft / 2 + 1;
constexpr int kTile = 64;                              // frames (stft) / hop blocks (istft) per workgroup
constexpr int kSpan = (kTile - 1) * kHop + kNfft;      // samples an stft tile reads
constexpr int kSigLds = kSpan + (kSpan >> 8) * 4 + 4;  // with 4 pad floats per 256 samples

constexpr int kChan = 2 * kBins;                       // 1026 recomb channels
constexpr int kKpad = FS2_ISTFT_KPAD;                  // padded to 129 groups of 8
constexpr int kChunkG = 3, kChunkC = 8 * kChunkG;      // channel groups / channels per LDS chunk
constexpr int kChunks = kKpad / kChunkC;               // 43
constexpr int kFr = kTile + 3;                         // frames a tile of hop blocks reads
constexpr int kLd = kFr + 1;                           // LDS row pitch (68)
constexpr int kStage = (kChunkC * kFr + 255) / 256;    // staged elements per thread (7)
static_assert(kChunks * kChunkC == kKpad && kKpad >= kChan && kKpad % 8 == 0, "channel padding");

__device__ __forceinline__ int sig_idx(int s) { return s + ((s >> 8) << 2); }

// row (of a 32-row MFMA result tile) held in accumulator register r by lane half h
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// m * z / |z|, and (m, 0) for z = 0. z is divided by max(|re|, |im|) first: one of the two ratios
// is +-1, the other at most 1 in magnitude, so the squares neither overflow nor underflow.
__device__ __forceinline__ void project(float re, float im, float m, float &pr, float &pi) {
  const float s = fmaxf(fabsf(re), fabsf(im));
  if (s == 0.0f) {
    pr = m;
    pi = 0.0f;
    return;
  }
  const float a = re / s, b = im / s;
  const float n = sqrtf(fmaf(a, a, b * b));
  pr = m * (a / n);
  pi = m * (b / n);
}

__global__ __launch_bounds__(256, 2) void stft_kernel(const float *__restrict__ wav, int64_t wav_stride,
                                                      const int64_t *__restrict__ lens, int n_max, int T_out, int clip,
                                                      const float *__restrict__ basis,
                                                      const float *__restrict__ mag_target, int64_t mag_stride,
                                                      float *__restrict__ spec, float *__restrict__ mag,
                                                      float *__restrict__ recomb, int64_t *__restrict__ frames_out) {
  __shared__ __attribute__((aligned(16))) float sm[kSigLds];
  const int b = blockIdx.y, t0 = blockIdx.x * kTile;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int j = lane & 31, h = lane >> 5;

  int64_t len64 = lens != nullptr ? lens[b] : (int64_t)n_max;
  const int len = (int)(len64 < 0 ? 0 : (len64 > n_max ? n_max : len64));
  const int nfr = len > kNfft / 2 ? 1 + len / kHop : 0;
  if (blockIdx.x == 0 && tid == 0 && frames_out != nullptr) frames_out[b] = nfr;
  const int t_valid = min(nfr, T_out);       // columns [0, t_valid) carry data
  const int t_end = min(t0 + kTile, T_out);  // this tile's columns are [t0, t_end)
  float *spec_b = spec != nullptr ? spec + (int64_t)b * kChan * T_out : nullptr;
  float *rec_b = recomb != nullptr ? recomb + (int64_t)b * kChan * T_out : nullptr;
  float *mag_b = mag != nullptr ? mag + (int64_t)b * kBins * T_out : nullptr;
  const float *tgt_b = mag_target != nullptr ? mag_target + (int64_t)b * kBins * mag_stride : nullptr;

  if (t0 >= t_valid) {  // a tile of padding columns only (block-uniform)
    const int cols = t_end - t0;
    for (int e = tid; e < kChan * cols; e += 256) {
      const int c = e / cols, t = t0 + (e - c * cols);
      if (spec_b != nullptr) spec_b[(int64_t)c * T_out + t] = 0.0f;
      if (rec_b != nullptr) rec_b[(int64_t)c * T_out + t] = 0.0f;
      if (mag_b != nullptr && c < kBins) mag_b[(int64_t)c * T_out + t] = 0.0f;
    }
    return;
  }

  // stage the span: sample p of the span is sample s = t0*hop + p - n_fft/2 of the utterance,
  // reflected at 0 and at len-1 (len > n_fft/2: one reflection suffices for every valid frame;
  // what a padding frame would read past that is 0 and its results are dropped)
  {
    const int64_t wbase = (int64_t)b * wav_stride;
    for (int p = tid; p < kSpan; p += 256) {
      int64_t s = (int64_t)t0 * kHop + p - kNfft / 2;
      if (s < 0) s = -s;
      if (s >= len) s = 2 * (int64_t)(len - 1) - s;
      float v = 0.0f;
      if (s >= 0 && s < len) {
        v = wav[wbase + s];
        if (clip) v = fminf(fmaxf(v, -1.0f), 1.0f);
      }
      sm[sig_idx(p)] = v;
    }
  }
  __syncthreads();

  // one (bin, frame) result: 0 in a padding column of a tile that has data
  auto emit = [&](int bin, int t, float re, float im) {
    if (t >= t_end) return;
    const bool valid = t < t_valid;
    if (!valid) re = im = 0.0f;
    const int64_t o_re = (int64_t)bin * T_out + t, o_im = (int64_t)(kBins + bin) * T_out + t;
    if (spec_b != nullptr) {
      spec_b[o_re] = re;
      spec_b[o_im] = im;
    }
    if (mag_b != nullptr) mag_b[o_re] = sqrtf(re * re + im * im);
    if (rec_b != nullptr) {
      float pr = 0.0f, pi = 0.0f;
      if (valid) project(re, im, tgt_b[(int64_t)bin * mag_stride + t], pr, pi);
      rec_b[o_re] = pr;
      rec_b[o_im] = pi;
    }
  };

  // the Nyquist bin: thread -> (frame tid>>2, quarter tid&3), a VALU dot product over the span
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
    if (part == 0) emit(kBins - 1, t0 + fr, re, im);
  }

  // bin tiles: a wave owns tiles wid, wid+4, wid+8, wid+12 (32 bins each), re and im of both
  // 32-frame halves; MFMA q of a 32-k block pairs k = kb+q (lanes 0-31) with k = kb+16+q
  const float *x0 = sm + sig_idx(j * kHop) + 16 * h;         // frame j of half 0; + kb (+ pad) per block
  const float *x1 = sm + sig_idx((32 + j) * kHop) + 16 * h;  // frame 32 + j
  for (int bt = wid; bt < (kBins - 1) / 32; bt += 4) {
    const int bin0 = bt * 32;
    const float4 *are = reinterpret_cast<const float4 *>(basis + (int64_t)(bin0 + j) * kNfft + 16 * h);
    const float4 *aim = reinterpret_cast<const float4 *>(basis + (int64_t)(kBins + bin0 + j) * kNfft + 16 * h);
    // two-level sum: 256 terms in the MFMA chain (cre, cim), the four quarter sums in tre, tim
    f32x16 cre[2], cim[2], tre[2], tim[2];
#pragma unroll
    for (int r = 0; r < 16; ++r)
      cre[0][r] = cre[1][r] = cim[0][r] = cim[1][r] = tre[0][r] = tre[1][r] = tim[0][r] = tim[1][r] = 0.0f;
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
      if ((kb & 255) == 224) {  // a quarter (256 k) is done
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            tre[f][r] += cre[f][r];
            tim[f][r] += cim[f][r];
            cre[f][r] = cim[f][r] = 0.0f;
          }
      }
    }
    // (bin0 + acc_row(r, h), frame t0 + 32f + j): 32 lanes write 32 consecutive frames of a bin row
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) emit(bin0 + acc_row(r, h), t0 + 32 * f + j, tre[f][r], tim[f][r]);
  }
}

__global__ __launch_bounds__(256) void istft_kernel(const float *__restrict__ recomb, int64_t rec_stride,
                                                    const int64_t *__restrict__ frames, int T_in, int n_out_max,
                                                    const float *__restrict__ inv_packed,
                                                    const float *__restrict__ wsum_table, float *__restrict__ wav,
                                                    int64_t wav_stride, int64_t *__restrict__ lens_out) {
  __shared__ float sm[2][kChunkC * kLd];
  const int b = blockIdx.y, jo0 = blockIdx.x * kTile;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int j = lane & 31, h = lane >> 5;

  const int64_t T64 = frames != nullptr ? frames[b] : (int64_t)T_in;
  const int T = (int)(T64 < 0 ? 0 : (T64 > T_in ? T_in : T64));
  const int nb = T > 1 ? T - 1 : 0;  // output hop blocks of this utterance
  if (blockIdx.x == 0 && tid == 0 && lens_out != nullptr) lens_out[b] = (int64_t)kHop * nb;
  const int64_t s0 = (int64_t)jo0 * kHop;  // first sample of the tile (< n_out_max by the grid)
  const int n_tile = (int)(n_out_max - s0 < kTile * kHop ? n_out_max - s0 : kTile * kHop);
  float *wout = wav + (int64_t)b * wav_stride + s0;

  if (jo0 >= nb) {  // a tile past the utterance's end (block-uniform)
    for (int e = tid; e < n_tile; e += 256) wout[e] = 0.0f;
    return;
  }

  // chunk ck of the recomb operand: channels 24 ck .. 24 ck + 23, frames jo0 - 1 .. jo0 + 65; a
  // frame outside [0, T) and a channel past 1026 read nothing and stage 0
  const float *rb = recomb + (int64_t)b * kChan * rec_stride;
  auto load_chunk = [&](int ck, float v[kStage]) {
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
      const int e = tid + 256 * i;
      const int cl = e / kFr, fl = e - cl * kFr;
      const int c = ck * kChunkC + cl, fr = jo0 - 1 + fl;
      v[i] = (e < kChunkC * kFr && c < kChan && fr >= 0 && fr < T) ? rb[(int64_t)c * rec_stride + fr] : 0.0f;
    }
  };
  auto store_chunk = [&](float *buf, const float v[kStage]) {
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
      const int e = tid + 256 * i;
      const int cl = e / kFr, fl = e - cl * kFr;
      if (e < kChunkC * kFr) buf[cl * kLd + fl] = v[i];
    }
  };

  // two-level sum: a chunk's 96 terms accumulate in acc (the MFMA chain), the 43 chunk sums in tot.
  // One chain of 4104 f32 additions is 4-5x further from float64 than the reference's blocked sum.
  f32x16 acc[2][2], tot[2][2];  // [phase tile][block tile]
#pragma unroll
  for (int pt = 0; pt < 2; ++pt)
#pragma unroll
    for (int ft = 0; ft < 2; ++ft)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[pt][ft][r] = tot[pt][ft][r] = 0.0f;

  float v[kStage];
  load_chunk(0, v);
  store_chunk(sm[0], v);
  __syncthreads();

  // step s = 4 g + q reads float4 (s*256 + phase)*2 + h: the lane's phase, channels 8g + 2e + h
  constexpr int kSteps = (kKpad / 8) * 4;
  const float4 *ap = reinterpret_cast<const float4 *>(inv_packed) + (wid * 64 + j) * 2 + h;
  float4 a_cur[2] = {ap[0], ap[64]};
  for (int ck = 0; ck < kChunks; ++ck) {
    if (ck + 1 < kChunks) load_chunk(ck + 1, v);
    const float *buf = sm[ck & 1];
#pragma unroll
    for (int gl = 0; gl < kChunkG; ++gl) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int step = (ck * kChunkG + gl) * 4 + q;
        const int nstep = step + 1 < kSteps ? step + 1 : step;  // the last step reloads itself (unused)
        const float4 a_nxt[2] = {ap[(int64_t)nstep * 512], ap[(int64_t)nstep * 512 + 64]};
        // block jo0 + 32 ft + j reads frame jo + 2 - q: staged column 32 ft + j + 3 - q
        float fv[2][4];
#pragma unroll
        for (int ft = 0; ft < 2; ++ft)
#pragma unroll
          for (int e = 0; e < 4; ++e) fv[ft][e] = buf[(gl * 8 + 2 * e + h) * kLd + 32 * ft + j + 3 - q];
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
          const float a[4] = {a_cur[pt].x, a_cur[pt].y, a_cur[pt].z, a_cur[pt].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[pt][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fv[0][e], a[e], acc[pt][0], 0, 0, 0);
            acc[pt][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fv[1][e], a[e], acc[pt][1], 0, 0, 0);
          }
        }
        a_cur[0] = a_nxt[0];
        a_cur[1] = a_nxt[1];
      }
    }
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
      for (int ft = 0; ft < 2; ++ft)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          tot[pt][ft][r] += acc[pt][ft][r];
          acc[pt][ft][r] = 0.0f;
        }
    if (ck + 1 < kChunks) store_chunk(sm[(ck + 1) & 1], v);
    __syncthreads();
  }

  // block jo0 + 32 ft + acc_row(r, h), phase 64 wid + 32 pt + j: divide by the window sum of the
  // frames that exist (q = 0..3 hop blocks back from ola block jo + 2), times n_fft / hop
#pragma unroll
  for (int ft = 0; ft < 2; ++ft)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jl = 32 * ft + acc_row(r, h), jo = jo0 + jl;
      const int mask = (jo + 2 < T ? 1 : 0) | (jo + 1 < T ? 2 : 0) | (jo < T ? 4 : 0) | (jo >= 1 ? 8 : 0);
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) {
        const int ph = wid * 64 + pt * 32 + j;
        const int s = jl * kHop + ph;
        if (s < n_tile) wout[s] = jo < nb ? tot[pt][ft][r] / wsum_table[mask * kHop + ph] * 4.0f : 0.0f;
      }
    }
}

}  // namespace

extern "C" int fs2_stft(const fs2_stft_desc *d, fs2_stream_t stream) {
  if (d == nullptr || d->wav == nullptr || d->basis == nullptr) return FS2_EINVAL;
  if (d->spec == nullptr && d->mag == nullptr && d->recomb == nullptr) return FS2_EINVAL;
  if ((d->mag_target != nullptr) != (d->recomb != nullptr)) return FS2_EINVAL;
  if (d->B < 1 || d->n_max < 1 || d->T_out < 1 || d->wav_row_stride < d->n_max) return FS2_EINVAL;
  if (d->mag_target != nullptr && d->mag_row_stride < d->T_out) return FS2_EINVAL;
  if (d->n_fft != kNfft || d->win != kNfft || d->hop != kHop) return FS2_EUNSUPPORTED;
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
  dim3 grid((d->T_out + kTile - 1) / kTile, d->B);
  hipLaunchKernelGGL(stft_kernel, grid, dim3(256), 0, as_stream(stream), d->wav, d->wav_row_stride, d->lens, d->n_max,
                     d->T_out, d->clip, d->basis, d->mag_target, d->mag_row_stride, d->spec, d->mag, d->recomb,
                     d->frames_out);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_istft(const fs2_istft_desc *d, fs2_stream_t stream) {
  if (d == nullptr || d->recomb == nullptr || d->inv_packed == nullptr || d->wsum_table == nullptr ||
      d->wav == nullptr)
    return FS2_EINVAL;
  if (d->B < 1 || d->T_in < 1 || d->n_out_max < 1 || d->recomb_row_stride < d->T_in ||
      d->wav_row_stride < d->n_out_max)
    return FS2_EINVAL;
  if (d->n_fft != kNfft || d->win != kNfft || d->hop != kHop) return FS2_EUNSUPPORTED;
  if (d->B > 65535) return FS2_EUNSUPPORTED;
  // n_out_max against every frame count the host can see
  if (d->frames_host != nullptr) {
    for (int b = 0; b < d->B; ++b) {
      int64_t t = d->frames_host[b];
      t = t < 0 ? 0 : (t > d->T_in ? d->T_in : t);
      if (t > 1 && (t - 1) * kHop > d->n_out_max) return FS2_EINVAL;
    }
  } else if (d->frames == nullptr) {
    if (d->T_in > 1 && (int64_t)(d->T_in - 1) * kHop > d->n_out_max) return FS2_EINVAL;
  }
  const int blocks = (d->n_out_max + kHop - 1) / kHop;
  dim3 grid((blocks + kTile - 1) / kTile, d->B);
  hipLaunchKernelGGL(istft_kernel, grid, dim3(256), 0, as_stream(stream), d->recomb, d->recomb_row_stride, d->frames,
                     d->T_in, d->n_out_max, d->inv_packed, d->wsum_table, d->wav, d->wav_row_stride, d->lens_out);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}
