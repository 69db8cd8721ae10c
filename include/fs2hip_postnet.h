/*
 * fs2hip_postnet.h — fs2_pn_head3: mel_linear (model/fastspeech2.py:127) and the PostNet's first
 * three convolutions (transformer/Layers.py:92-137, layers 0..2: 80 -> 512 -> 512 -> 512, k = 5,
 * pad 2, BatchNorm folded, tanh) in one launch on padded [B, T] rows, bf16:
 *   mel[m] = x[rowmap[m]] W_mel^T + b_mel     (rowmap NULL: x[m]; rowmap[m] < 0, a padded frame: b_mel)
 *   out    = tanh(conv(tanh(conv(tanh(conv(bf16(mel); w[0]) + bias[0]); w[1]) + bias[1]); w[2]) + bias[2])
 * The same bits as fs2_conv1d with KS = 1, FS2_EPI_BIAS, f32 out and the bf16 out2 copy, then
 * fs2_wconv with w2 (layers 0 + 1), then fs2_wconv for layer 2: the bf16 mel and the two 512-channel
 * intermediates never leave the chip. mel_w: bf16 [80][256] row-major (what fs2_conv1d takes for
 * KS = 1, Cin = 256); w[0]: 512 * 416 elements, w[1], w[2]: 512 * 2560, all three in fs2_wconv's
 * fragment order (fs2hip.h).
 */
#ifndef FS2HIP_POSTNET_H
#define FS2HIP_POSTNET_H

#include "fs2hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fs2_pn_head3_desc {
  const void *x;            /* bf16 decoder rows [x_rows, >= 256]                                 */
  int64_t x_row_stride;
  int64_t x_rows;
  const int32_t *rowmap;    /* [B*T] source row of each padded row (-1: zeros), or NULL           */
  const void *mel_w;
  const float *mel_b;       /* [80]                                                               */
  float *mel;               /* f32 [B*T, >= 80]                                                   */
  int64_t mel_row_stride;
  void *mel_bf16;           /* optional bf16 [B*T, 80] copy of mel (NULL: not written)            */
  const void *w[3];
  const float *bias[3];     /* [512] each                                                         */
  int B, T;
  void *out;                /* bf16 [B*T, >= 512]: layer 2's output                               */
  int64_t out_row_stride;
} fs2_pn_head3_desc;

int fs2_pn_head3(const fs2_pn_head3_desc *d, fs2_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* FS2HIP_POSTNET_H */
