// The size arithmetic of include/fs2hip_vad.h in one place: the entry points validate and size their
// launches with it, the kernels lay out their LDS with it, and fs2_vad_frames / fs2_vad_workspace_bytes /
// fs2_vad_lds_bytes report it. Plain C++, in 64 bits throughout and saturating, so that it also
// compiles for the host alone (tools/vad_sizes_check.cpp runs it under the sanitizers). Every argument
// is at most INT32_MAX where a product is formed: the largest, 8 * B * tiles, stays under 2^63 then.
#pragma once
#include <stdint.h>

#include "fs2hip_vad.h"

#ifdef __HIPCC__
#define FS2_VAD_HD __host__ __device__
#else
#define FS2_VAD_HD
#endif

#define FS2_VAD_SUMS_MAX (FS2_VAD_SUMS_BYTES / 8)  // block sums a tile keeps in LDS

// frames of a row of n samples: 0 for n < 1, else 1 + n / hop. hop >= 1.
FS2_VAD_HD static inline int64_t vad_frames(int64_t n, int64_t hop) { return n < 1 ? 0 : 1 + n / hop; }

// g = gcd(frame_length, hop), both >= 1: a frame is frame_length / g whole blocks of g samples, and
// neighbouring frames are hop / g blocks apart
FS2_VAD_HD static inline int64_t vad_gcd(int64_t a, int64_t b) {
  while (b != 0) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// elements between the first samples of two neighbouring blocks in LDS: g rounded up so that the
// distance is an odd number of 32-bit words (esize 4) or of 16-bit pairs (esize 2), which keeps the
// 64 lanes of a wave, one block each, on different banks
FS2_VAD_HD static inline int64_t vad_row_stride(int64_t g, int64_t esize) {
  return esize == 4 ? (g | 1) : g + ((2 - g % 4) + 4) % 4;
}

// frames per workgroup: as many as FS2_VAD_TILE_FRAMES, as few as the block sums of the tile,
// (G - 1) * (hop / g) + frame_length / g, fit FS2_VAD_SUMS_MAX; 0 where one frame's do not.
// 1 <= hop <= frame_length.
FS2_VAD_HD static inline int64_t vad_tile_frames(int64_t frame_length, int64_t hop) {
  const int64_t g = vad_gcd(frame_length, hop), q = frame_length / g, h = hop / g;
  if (q > FS2_VAD_SUMS_MAX) return 0;
  const int64_t G = (FS2_VAD_SUMS_MAX - q) / h + 1;
  return G < FS2_VAD_TILE_FRAMES ? G : FS2_VAD_TILE_FRAMES;
}

// block sums of a tile of G >= 1 frames
FS2_VAD_HD static inline int64_t vad_tile_blocks(int64_t frame_length, int64_t hop, int64_t G) {
  const int64_t g = vad_gcd(frame_length, hop);
  return (G - 1) * (hop / g) + frame_length / g;
}

// the least LDS a launch with this geometry needs: the block sums of one frame as f64 and one block of
// f32 samples at its padded stride. 0 for a size below 1 or hop > frame_length.
FS2_VAD_HD static inline int64_t vad_lds_bytes(int64_t frame_length, int64_t hop) {
  if (frame_length < 1 || hop < 1 || hop > frame_length) return 0;
  const int64_t g = vad_gcd(frame_length, hop);
  return 8 * (frame_length / g) + 4 * vad_row_stride(g, 4);
}

// whether both parts fit their areas (the sums FS2_VAD_SUMS_BYTES, the block FS2_VAD_AREA_BYTES)
FS2_VAD_HD static inline int vad_fits(int64_t frame_length, int64_t hop) {
  const int64_t g = vad_gcd(frame_length, hop);
  return 8 * (frame_length / g) <= FS2_VAD_SUMS_BYTES && 4 * vad_row_stride(g, 4) <= FS2_VAD_AREA_BYTES;
}

// tiles over F_max frames; 0 for F_max < 1 or a geometry that does not fit
FS2_VAD_HD static inline int64_t vad_tiles(int64_t F_max, int64_t frame_length, int64_t hop) {
  if (F_max < 1 || frame_length < 1 || hop < 1 || hop > frame_length) return 0;
  const int64_t G = vad_tile_frames(frame_length, hop);
  return G < 1 ? 0 : (F_max + G - 1) / G;
}

// bytes of the workspace of fs2_vad_power: one f64 maximum per tile and row. 0 for a size below 1.
FS2_VAD_HD static inline int64_t vad_workspace_bytes(int64_t B, int64_t F_max, int64_t frame_length, int64_t hop) {
  const int64_t t = vad_tiles(F_max, frame_length, hop);
  if (B < 1 || t < 1) return 0;
  return B > INT64_MAX / 8 / t ? INT64_MAX : 8 * B * t;
}

// FS2_OK, or why fs2_vad_power refuses these sizes (the codes of include/fs2hip.h)
FS2_VAD_HD static inline int vad_check(int64_t B, int64_t n_max, int64_t frame_length, int64_t hop) {
  if (B < 1 || n_max < 1 || frame_length < 1 || hop < 1 || hop > frame_length) return FS2_EINVAL;
  if (B > FS2_VAD_B_MAX || !vad_fits(frame_length, hop)) return FS2_EUNSUPPORTED;
  const int64_t F = vad_frames(n_max, hop);
  if (F > INT32_MAX || B * F > INT32_MAX / 8) return FS2_EUNSUPPORTED;  // P's bytes
  return FS2_OK;
}
