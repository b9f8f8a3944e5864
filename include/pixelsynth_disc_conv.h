/* pixelsynth_disc_conv.h -- the C ABI of libpixelsynth_disc_conv.so: the discriminator's 4 x 4 convolution (stride 1 or 2, padding 2,
 * no bias) and its backward pass on the fp16 matrix pipe (csrc/disc_conv.hip).  A library of its own beside libpixelsynth_hip.so, whose
 * pinned set of exports it leaves as it is.  Same conventions: int status, 0 = success, ps_disc_conv_last_error() says why not; every
 * buffer and the workspace are the caller's; the last parameter is the stream; no allocation, no synchronisation, no device-to-host
 * copy, no atomics.  Every result is bit-identical from run to run, and an element of y or grad_x depends neither on its frame's place
 * in the batch nor on the size of the batch.
 *
 * Notation: x (B,Ci,H,W), weight (Co,Ci,4,4), y and g = grad_y (B,Co,Ho,Wo), all fp32 dense NCHW, aligned to 4 bytes;
 *   Ho = (H + 2 pad - 4) / stride + 1, Wo likewise;  y[b,o,oy,ox] = sum_{c,ky,kx} w[o,c,ky,kx] xpad[b,c,oy stride + ky, ox stride + kx],
 *   xpad = x with `pad` zeros around the frame.  Hp = H + 2 pad, Wp = W + 2 pad, Wo8 = Wo rounded up to a multiple of 8.
 *
 * What is taken (ps_disc_conv_takes): stride 1 or 2; pad 2 and only 2 (the argument is there for a later layer); Ci and Co multiples of
 * 64 up to 512; H, W >= 1; 1 <= B <= 65535; and every frame within 32-bit offsets: Hp Wp Ci, (Ho + 2)(Wo + 2) Co, Ci Hp Wo8 and
 * Co Ho Wo8 below 2^31, and B ceil(Ho Wo8 / 16) below 2^31.
 *
 * Arithmetic.  Every product runs on v_mfma_f32_32x32x16_f16 with both operands split as csrc/conv_f16x3.hip splits them
 * (hi = fp16(v), lo = fp16(v - hi)), three MFMAs per product (lo * hi, hi * lo, hi * hi), fp32 sums.  The split keeps its 22 bits only
 * down to 2^-3, so
 *   - the WEIGHT (weight_orig / sigma, entries around 1e-2) is multiplied by a power of two sw before it is split, and the sums by
 *     1 / sw: sw = 2^(15 - e) with max|w| = f 2^e, f in [0.5, 1), the exponent held in [-126, 126]; sw = 1 for a maximum of 0 or one
 *     that is not finite.  Found, kept and applied on the device at every call;
 *   - grad_y is multiplied by sg, the same rule on max|g|, and the gradients by 1 / sg (grad_x: (sum * (1 / sw)) * (1 / sg));
 *   - x is split as it is, as the 3 x 3 convolutions split their activations.
 * All of these are exact.
 *
 * Passes and sum orders.
 *   pack         max|w| (order-free), then w * sw split into [tap][out channel][in channel] fp16 planes: forward u = 4 ky + kx;
 *                grad_x at stride 1 the flipped, transposed weight, u = 4 (3 - ky) + (3 - kx); at stride 2 the four parities,
 *                u = 4 (2 (ky & 1) + (kx & 1)) + 2 (1 - (ky >> 1)) + (1 - (kx >> 1)).
 *   layout       x (or g * sg) NCHW -> split fp16 channels-last with the zero border written out: (B,Hp,Wp,Ci), g with a border of 1.
 *   product      one implicit-GEMM kernel for y and grad_x: an element is one chain of fp32 sums, taps in ascending u, inside a tap
 *                the channels in ascending blocks of 16.  grad_x at stride 1 is that kernel on g * sg with pad 1; at stride 2 four
 *                2 x 2 stride-1 products, one per parity (iy & 1, ix & 1) of the input pixel, each writing every second pixel of every
 *                second row (a gather: no scatter, no zero-inserted copy).
 *   grad_weight  a GEMM whose reduction runs over the pixels.  g * sg and x are laid out pixel-minor in rows of Wo8 (zeros behind Wo):
 *                g (B,Co,Ho,Wo8); x once per kx, (4,B,Ci,Hp,Wo8) with [kx][b][c][yp][j] = xpad[b,c,yp,j stride + kx], rows outside the
 *                frame zeros.  A step is 16 pixels: the 8-pixel chunks q = 2 i and 2 i + 1 of a frame's Ho (Wo8 / 8) chunks
 *                (row-major; a chunk past the last one counts as zeros).  The steps of all frames, frame by frame, are cut into parts:
 *                     steps          = B ceil(Ho (Wo8 / 8) / 2)
 *                     blocks         = (Co / 64) (Ci / 32)
 *                     steps per part = max(8, ceil(steps / min(PS_DISC_CONV_MAX_PARTS, ceil(512 / blocks))))
 *                     parts          = ceil(steps / steps per part)
 *                a function of the sizes alone; the last part may be shorter and a part may span frames.  A part is one chain of fp32
 *                sums per element in ascending step order; a second kernel adds the parts in ascending order and multiplies by 1 / sg.
 *
 * Overflow.  *overflow is set to 1 where a value of x with |v| > 65000 or a NaN is met, or a scaled weight that is not finite (the
 * results are then wrong); *grad_overflow likewise for g * sg (and the weight, in the backward pass).  Neither is ever cleared here. */
#ifndef PIXELSYNTH_DISC_CONV_H
#define PIXELSYNTH_DISC_CONV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_DISC_CONV_MAX_PARTS 256

/* 1 where the sizes are taken (above), else 0. */
int ps_disc_conv_takes(int B, int Ci, int Co, int H, int W, int stride, int pad);

/* Bytes of workspace either pass needs for these sizes (device memory, 256-byte aligned); 0 for sizes that are refused. */
size_t ps_disc_conv_workspace_bytes(int B, int Ci, int Co, int H, int W, int stride, int pad);

/* The number of parts the grad_weight reduction of these sizes is cut into (1 .. PS_DISC_CONV_MAX_PARTS); 0 for sizes refused. */
int ps_disc_conv_parts(int B, int Ci, int Co, int H, int W, int stride, int pad);

/* y = conv2d(x, weight, stride, pad). */
int ps_disc_conv_forward_f16x3(const float *x, const float *weight, int B, int Ci, int Co, int H, int W, int stride, int pad, float *y,
                               int *overflow, void *workspace, size_t workspace_bytes, void *stream);

/* grad_x (B,Ci,H,W) and grad_weight (Co,Ci,4,4) of the convolution above for g = grad_y; either may be NULL and is then not
 * computed.  scale2 (two floats on the device) receives {sg, 1 / sg}. */
int ps_disc_conv_backward_f16x3(const float *x, const float *weight, const float *g, int B, int Ci, int Co, int H, int W, int stride,
                                int pad, float *grad_x, float *grad_weight, float *scale2, int *overflow, int *grad_overflow,
                                void *workspace, size_t workspace_bytes, void *stream);

/* ps_disc_conv_last_error: the message of this library's last failed call. */
const char *ps_disc_conv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_DISC_CONV_H */
