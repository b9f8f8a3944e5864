/* pixelsynth_percsim.h -- the C ABI of libpixelsynth_percsim.so, the PercSim passes (csrc/percsim.hip).  A library of its own next to
 * libpixelsynth_hip.so, whose entry points it does not repeat: the convolutions of a pass are that library's.  Same conventions as
 * include/pixelsynth_hip.h (int status, 0 = success; ps_percsim_last_error() says why not; the last parameter is the stream). */
#ifndef PIXELSYNTH_PERCSIM_H
#define PIXELSYNTH_PERCSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* ---- PercSim, the VGG16 perceptual similarity (csrc/percsim.hip): the passes around the convolutions of the reference's PNet
 * (models/networks/pretrained_networks.py:11-93, :199-240).  The 13 convolutions are ps_conv3x3_thin_in_f16x3_nhwc (conv1_1, its weight
 * padded to 4 input channels) and ps_conv3x3_f16x3_nhwc (the rest, the ReLU as act with scale 1, shift 0; conv1_1's bias folded into
 * conv1_2's act as shift = -bias).  A network pass holds P pairs as 2P images: image i is in0 of pair i, image P + i its in1.
 * ps_percsim_input: image pairs img1, img2 (B, 3, H, W) read through element strides as ps_image_metrics reads them (dtype
 *   PS_DTYPE_F32 = 0 or PS_DTYPE_U8 = 1 of include/pixelsynth_hip.h, x / 255.0f) -> out0 (from img1), out1 (from img2) (B, H, W, 4) fp32 NHWC, channel 3 zero, 16-byte
 *   aligned.  Per element, the reference's fp32 operations in its order: u = x / 255 (uint8); PS_PERCSIM_VIS: u * m, PS_PERCSIM_INVIS:
 *   u * (1 - m), m the mask (B, 1, H, W) f32 contiguous (calc_errors_quality.py:38-47; NULL otherwise); t = u * 2 - 1
 *   (evaluation/metrics.py:27-31); (t - shift_c) / scale_c, shift (-0.030, -0.088, -0.188), scale (0.458, 0.448, 0.450).
 *   PS_PERCSIM_RAW: fp32 images already in [-1, 1] (PNet.forward's input), the last step only.
 * ps_percsim_tap: the tapped layer `layer` (0 .. 4: relu1_2, relu2_2, relu3_3, relu4_3, relu5_3) of a pass at image size H x W (multiples
 *   of 128): y (2P, H >> layer, W >> layer, C) fp32 NHWC, the layer's PRE-ReLU output, C a multiple of 64.  Adds the layer's per-tile
 *   sums of cos_sim(relu(y[i]), relu(y[P + i])) to the workspace; pooled (2P, H >> (layer + 1), W >> (layer + 1), C) or NULL: the
 *   2 x 2 stride-2 max-pool of y (pre-ReLU), written by the same read.  Non-finite values go through as torch.relu and
 *   F.max_pool2d hand them on: a NaN in y stays a NaN (not the 0 of a maxNum), so a NaN -- or a +inf, inf / inf -- in any channel of a
 *   pixel of either image of a pair makes that layer's score and that pair's total NaN and touches no other pair; a pooled window
 *   that holds a NaN is NaN; -inf is a negative value like any other.
 * ps_percsim_finish: -> layers (P, 5) f32, 1 - mean_pixels(cos_sim) per tapped layer, and total (P) f32, their sum: PNet's
 *   retPerLayer scores and its value.  After the five taps of a pass.
 *   workspace: >= ps_percsim_workspace_bytes(P, H, W) bytes of device memory (per-tile partial sums), shared by a pass's taps and its
 *   finish.  Its layout: doubles [layer][pair][tile], layer l's block P * tiles_l long with tiles_l = (H_l / 2)(W_l / 2) / 16,
 *   H_l = H >> l, W_l = W >> l; a tile is 16 consecutive 2 x 2 pixel blocks of the map in row-major order, its double the sum of its
 *   64 pixels' cosines.  A tap writes every double of its layer's block and nothing else; the finish reads all five blocks (a layer
 *   whose block is zero scores 1).  Each call one launch on `stream`, no allocation, no synchronisation, no atomics:
 *   bit-reproducible, and a pair's numbers depend neither on its place in the pass nor on P.
 * ps_percsim_workspace_bytes: host-only arithmetic; 0 when H or W is not a multiple of 128. */
enum { PS_PERCSIM_PLAIN = 0, PS_PERCSIM_VIS = 1, PS_PERCSIM_INVIS = 2, PS_PERCSIM_RAW = 3 };
size_t ps_percsim_workspace_bytes(int P, int H, int W);
int ps_percsim_input(const void *img1, const int64_t *strides1, const void *img2, const int64_t *strides2, int dtype, const float *mask,
                     int mode, int B, int H, int W, float *out0, float *out1, void *stream);
int ps_percsim_tap(const float *y, int P, int H, int W, int layer, int C, float *pooled, void *workspace, size_t workspace_bytes,
                   void *stream);
int ps_percsim_finish(const void *workspace, size_t workspace_bytes, int P, int H, int W, float *layers, float *total, void *stream);
/* ps_percsim_last_error: the message of this library's last failed call. */
const char *ps_percsim_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_PERCSIM_H */
