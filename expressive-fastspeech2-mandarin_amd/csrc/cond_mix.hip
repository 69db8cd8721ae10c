// Conditioning vectors from weights over the embedding rows (include/fs2hip_cond_mix.h): utterance
// mixtures (fs2_cond_mix, the outputs of fs2_cond_vectors) and per-phoneme emotion curves added in
// place to the encoder output (fs2_cond_mix_rows). The emotion Linear + ReLU is cond.h's
// cond_linear_tile, the code fs2_cond_vectors runs; only the fill of its cat rows differs.
#include "fs2_common.h"
#include "fs2hip_cond_mix.h"
#include "cond.h"

namespace {

struct MixIn {  // one conditioning input
  const void *p;
  int kind;
  const float *table;
  int n, d;
};

struct MixArgs {
  MixIn spk, emo, aro, val;
  const float *lin_w, *lin_b;
  int B, D, L;
  int64_t rows;  // B (utterance level) or B * L
  float *spk_out, *emo_out;
};

constexpr int kMixRowsU = 16;  // positions per tile of the curve kernel (cond_linear_tile's U)

// Channel k of input m's mixed embedding for utterance b / position row (= b * L + i): an id reads
// its table row; weights run the fmaf chain over the table rows in ascending j from +0.0f.
__device__ __forceinline__ float mix_value(const MixIn &m, int64_t b, int64_t row, int k) {
  if (m.kind == FS2_COND_IDS)
    return m.table[cond_clampi(reinterpret_cast<const int64_t *>(m.p)[b], m.n) * m.d + k];
  const float *w = reinterpret_cast<const float *>(m.p) + (m.kind == FS2_COND_ROWS ? row : b) * m.n;
  float acc = 0.f;
  for (int j = 0; j < m.n; ++j) acc = fmaf(w[j], m.table[(int64_t)j * m.d + k], acc);
  return acc;
}

// cat [U][dc] for rows r0 .. r0 + U - 1 (zeros past the last row), threads tid < 256
template <int U>
__device__ __forceinline__ void fill_cat(const MixArgs &a, int64_t r0, int tid, int dc, float *cat) {
  for (int i = tid; i < U * dc; i += 256) {
    const int u = i / dc, k = i - u * dc;
    const int64_t row = r0 + u;
    float x = 0.f;
    if (row < a.rows) {
      const int64_t b = a.L > 0 ? row / a.L : row;
      if (k < a.emo.d)
        x = mix_value(a.emo, b, row, k);
      else if (k < a.emo.d + a.aro.d)
        x = mix_value(a.aro, b, row, k - a.emo.d);
      else
        x = mix_value(a.val, b, row, k - a.emo.d - a.aro.d);
    }
    cat[i] = x;
  }
}

// Utterance level: tile (64 channels, kCondU utterances) as cond_tile; L = 0, rows = B.
__global__ __launch_bounds__(256) void cond_mix_kernel(MixArgs a) {
  extern __shared__ float sm[];
  const int tid = threadIdx.x;
  const int n0 = blockIdx.x * 64, b0 = blockIdx.y * kCondU;
  if (a.spk.table != nullptr) {
    for (int i = tid; i < kCondU * 64; i += 256) {
      const int b = b0 + (i >> 6), n = n0 + (i & 63);
      if (b < a.B && n < a.D) a.spk_out[(int64_t)b * a.D + n] = mix_value(a.spk, b, b, n);
    }
  }
  if (a.emo.table == nullptr) return;  // uniform over the workgroup
  const int dc = a.emo.d + a.aro.d + a.val.d;
  float *cat = sm;                // [kCondU][dc]
  float *red = sm + kCondU * dc;  // [kCondU][4][64]
  fill_cat<kCondU>(a, b0, tid, dc, cat);
  cond_linear_tile<kCondU>(a.lin_w, a.lin_b, dc, a.D, n0, tid, true, cat, red, [&](int u, int nn, float v) {
    const int b = b0 + u;
    if (b < a.B) a.emo_out[(int64_t)b * a.D + nn] = v;
  });
}

// Curves: workgroup blockIdx.x takes positions [16 x, 16 x + 16) of the B * L rows, fills their cat
// rows once and walks the channel blocks blockIdx.y, + gridDim.y, ...; each emotion value goes from
// LDS straight into x.
template <typename TX>
__global__ __launch_bounds__(256) void cond_mix_rows_kernel(MixArgs a, TX *__restrict__ x) {
  extern __shared__ float sm[];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * kMixRowsU;
  const int dc = a.emo.d + a.aro.d + a.val.d;
  float *cat = sm;                   // [kMixRowsU][dc]
  float *red = sm + kMixRowsU * dc;  // [kMixRowsU][4][64]
  fill_cat<kMixRowsU>(a, r0, tid, dc, cat);
  const int nbx = (a.D + 63) >> 6;
  for (int bx = blockIdx.y; bx < nbx; bx += gridDim.y) {  // uniform over the workgroup
    cond_linear_tile<kMixRowsU>(a.lin_w, a.lin_b, dc, a.D, bx * 64, tid, true, cat, red, [&](int u, int nn, float v) {
      const int64_t row = r0 + u;
      if (row < a.rows) {
        TX *px = x + row * a.D + nn;
        *px = (TX)(to_f32(*px) + v);
      }
    });
  }
}

bool kind_ok(int kind, const void *p, bool rows) {
  return p != nullptr && (kind == FS2_COND_IDS || kind == FS2_COND_MIX || (rows && kind == FS2_COND_ROWS));
}

// the emotion part's argument rows shared by the two entry points
int emo_check(const fs2_cond_mix_desc *d, bool rows) {
  if (!kind_ok(d->emo_kind, d->emotions, rows) || !kind_ok(d->aro_kind, d->arousals, rows) ||
      !kind_ok(d->val_kind, d->valences, rows))
    return FS2_EINVAL;
  if (d->aro_table == nullptr || d->val_table == nullptr || d->lin_w == nullptr || d->lin_b == nullptr)
    return FS2_EINVAL;
  if (d->n_emo <= 0 || d->n_aro <= 0 || d->n_val <= 0 || d->d_emo <= 0 || d->d_aro <= 0 || d->d_val <= 0)
    return FS2_EINVAL;
  return FS2_OK;
}

MixArgs mix_args(const fs2_cond_mix_desc *d, int L, int64_t rows) {
  MixArgs a;
  a.spk = MixIn{d->speakers, d->spk_kind, d->speaker_table, d->n_speaker, d->D};
  a.emo = MixIn{d->emotions, d->emo_kind, d->emo_table, d->n_emo, d->d_emo};
  a.aro = MixIn{d->arousals, d->aro_kind, d->aro_table, d->n_aro, d->d_aro};
  a.val = MixIn{d->valences, d->val_kind, d->val_table, d->n_val, d->d_val};
  a.lin_w = d->lin_w;
  a.lin_b = d->lin_b;
  a.B = d->B;
  a.D = d->D;
  a.L = L;
  a.rows = rows;
  a.spk_out = d->spk_out;
  a.emo_out = d->emo_out;
  return a;
}

}  // namespace

extern "C" int fs2_cond_mix(const fs2_cond_mix_desc *d, fs2_stream_t stream) {
  if (d == nullptr) return FS2_EINVAL;
  if (d->B < 0 || d->D <= 0) return FS2_EINVAL;
  if (d->speaker_table != nullptr &&
      (!kind_ok(d->spk_kind, d->speakers, false) || d->spk_out == nullptr || d->n_speaker <= 0))
    return FS2_EINVAL;
  if (d->emo_table != nullptr) {
    if (emo_check(d, false) != FS2_OK || d->emo_out == nullptr) return FS2_EINVAL;
  }
  if (d->B == 0 || (d->speaker_table == nullptr && d->emo_table == nullptr)) return FS2_OK;
  const int64_t dc = d->emo_table != nullptr ? (int64_t)d->d_emo + d->d_aro + d->d_val : 0;
  const int64_t smem = (int64_t)kCondU * (dc + 256) * (int64_t)sizeof(float);
  if (smem > 65536) return FS2_EUNSUPPORTED;
  MixArgs a = mix_args(d, 0, d->B);
  if (d->emo_table == nullptr) a.emo.d = a.aro.d = a.val.d = 0;
  hipLaunchKernelGGL(cond_mix_kernel, dim3((unsigned)((d->D + 63) / 64), (unsigned)((d->B + kCondU - 1) / kCondU)),
                     dim3(256), (size_t)smem, as_stream(stream), a);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}

extern "C" int fs2_cond_mix_rows(const fs2_cond_mix_desc *d, int L, void *x, int x_dtype, fs2_stream_t stream) {
  if (d == nullptr || x == nullptr) return FS2_EINVAL;
  if (d->B < 0 || L < 0 || d->D <= 0) return FS2_EINVAL;
  if (d->emo_table == nullptr) return FS2_EINVAL;
  if (emo_check(d, true) != FS2_OK) return FS2_EINVAL;
  if (x_dtype != FS2_F32 && x_dtype != FS2_BF16) return FS2_EUNSUPPORTED;
  const int64_t dc = (int64_t)d->d_emo + d->d_aro + d->d_val;
  const int64_t smem = (int64_t)kMixRowsU * (dc + 256) * (int64_t)sizeof(float);
  const int64_t rows = (int64_t)d->B * L;
  if (smem > 65536 || rows >= ((int64_t)1 << 31)) return FS2_EUNSUPPORTED;
  if (rows == 0) return FS2_OK;
  const MixArgs a = mix_args(d, L, rows);
  const int64_t tiles = (rows + kMixRowsU - 1) / kMixRowsU;
  // few row tiles: the channel blocks spread over workgroups too (the bits do not depend on it)
  const int nbx = (d->D + 63) / 64;
  dim3 grid((unsigned)tiles, (unsigned)(tiles < 256 ? min(nbx, 65535) : 1));
  hipStream_t s = as_stream(stream);
  if (x_dtype == FS2_F32)
    hipLaunchKernelGGL(cond_mix_rows_kernel<float>, grid, dim3(256), (size_t)smem, s, a, reinterpret_cast<float *>(x));
  else
    hipLaunchKernelGGL(cond_mix_rows_kernel<bf16>, grid, dim3(256), (size_t)smem, s, a, reinterpret_cast<bf16 *>(x));
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}
