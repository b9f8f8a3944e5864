/* pixelsynth_fid.h -- the C ABI of libpixelsynth_fid.so, the passes of the FID network (csrc/fid.hip): Inception-v3 as pytorch_fid
 * runs it (dims = 2048), on fp32 NHWC maps.  A library of its own next to libpixelsynth_hip.so.  Same conventions as
 * include/pixelsynth_hip.h (int status, 0 = success; ps_fid_last_error() says why not; the last parameter is the stream).  Each call is
 * one launch on `stream`: no allocation, no synchronisation, no atomics; an output element's value depends neither on its image's
 * place in the batch nor on the batch's size. */
#ifndef PIXELSYNTH_FID_H
#define PIXELSYNTH_FID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* ps_fid_input: images img (B, 3, H, W) read through element strides (dtype PS_DTYPE_F32 = 0, values in [0, 1], or PS_DTYPE_U8 = 1,
 *   x / 255.0f) -> out (B, 299, 299, 4) fp32 NHWC, channel 3 zero, 16-byte aligned: F.interpolate(size = (299, 299), mode = "bilinear",
 *   align_corners = False) in fp32 (scale = (float)in / 299, src = max(scale * (dst + 0.5f) - 0.5f, 0), i0 = (int)src,
 *   i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1, l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d)), then 2 * v - 1.
 *   A 299 x 299 input is not interpolated. */
int ps_fid_input(const void *img, const int64_t *strides, int dtype, int B, int H, int W, float *out, void *stream);

/* ps_fid_conv: y[n, ho, wo, coff + co] = max(bias[co] + sum_{kh, kw, ci} x[n, ho * stride - ph + kh, wo * stride - pw + kw, ci] *
 *   w[co, kh, kw, ci], 0), taps outside the map zero; Ho = (H + 2 ph - KH) / stride + 1, Wo likewise.  x (N, H, W, ldx floats per
 *   pixel, the first Ci read), y (N, Ho, Wo, ldy floats per pixel, channels coff .. coff + Co - 1 written and no other).  fp32
 *   operands on v_mfma_f32_16x16x4_f32, summed over k = (kh KW + kw) Ci + ci in a fixed order on three levels: a chunk of 16 k is one
 *   fp32 fma chain from zero (k = 16 chunk + 4 kk + j, j outer, kk inner), 16 chunks ascending add up to a middle sum, the middle sums
 *   ascending to the total; the bias is added last.  A NaN sum stays NaN (torch.relu's rule, not fmaxf's): a NaN in x reaches the
 *   outputs whose taps read it and no other.
 *   ps_fid_conv_takes: 1 <= KH, KW <= 7, stride 1 or 2, 0 <= ph < KH, 0 <= pw < KW, Ci a positive multiple of 4, Co >= 1.
 *   ps_fid_conv_co_tile(Co): the output channels of a workgroup, 32 or 64 (the one that pads Co less, 64 on a tie).
 *   wp: the weights packed for the kernel, ps_fid_conv_packed_floats(KH, KW, Ci, Co) floats (wp_floats says how many there are).
 *   With T = the co tile, K = KH KW Ci, S = ceil(K / 64) and w2[co][k] the (Co, K) matrix above, zero where co >= Co or k >= K:
 *   wp[((((cb S + s) 4 + c) (T / 16) + t) 64 + kk 16 + i) 4 + j] = w2[cb T + 16 t + i][64 s + 16 c + 4 kk + j].
 *   x, wp, y + coff 16-byte aligned; ldx, ldy, coff multiples of 4. */
int ps_fid_conv_takes(int KH, int KW, int stride, int ph, int pw, int Ci, int Co);
int ps_fid_conv_co_tile(int Co);
size_t ps_fid_conv_packed_floats(int KH, int KW, int Ci, int Co);
int ps_fid_conv(const float *x, int ldx, const float *wp, size_t wp_floats, const float *bias, int N, int H, int W, int Ci, int KH, int KW,
                int stride, int ph, int pw, int Co, float *y, int ldy, int coff, void *stream);

/* ps_fid_pool: x (N, H, W, ldx floats per pixel, the first C read, C a multiple of 4) -> y at channel offset coff of rows of ldy
 *   floats, as ps_fid_conv writes.  PS_FID_MAX_S2: 3 x 3 max, stride 2, no padding -> (N, (H - 3) / 2 + 1, (W - 3) / 2 + 1);
 *   PS_FID_MAX_S1: 3 x 3 max, stride 1, padding 1 (the padding never wins) -> (N, H, W); PS_FID_AVG_S1: 3 x 3 average, stride 1,
 *   padding 1, the sum over the taps inside the map (kh, then kw ascending) divided by their number -> (N, H, W); PS_FID_MEAN: the
 *   mean over the map, summed and divided in fp64, rounded to fp32 once -> (N, 1, 1).  A window (a map) that holds a NaN gives NaN in
 *   every mode, as F.max_pool2d and F.avg_pool2d do. */
enum { PS_FID_MAX_S2 = 0, PS_FID_MAX_S1 = 1, PS_FID_AVG_S1 = 2, PS_FID_MEAN = 3 };
int ps_fid_pool(const float *x, int ldx, int mode, int N, int H, int W, int C, float *y, int ldy, int coff, void *stream);

/* ps_fid_last_error: the message of this library's last failed call. */
const char *ps_fid_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_FID_H */
