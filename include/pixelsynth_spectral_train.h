/* pixelsynth_spectral_train.h -- the C ABI of libpixelsynth_spectral_train.so: the spectral normalisation of ALL layers of a network in
 * training, forward and backward, in a number of launches that does not depend on how many layers there are (csrc/spectral_train.hip).
 * The arithmetic is that of torch's legacy torch.nn.utils.spectral_norm hook with n_power_iterations = 1 and dim = 0.
 * libpixelsynth_hip.so's pinned set of exports stays as it is.  Same conventions: int status, 0 = success,
 * ps_spectral_train_last_error() says why not; every buffer and the workspace are the caller's; the last parameter of a queued call is
 * the stream; no allocation, no synchronisation, no copy in either direction, no atomics.  Every result is bit-identical from run to run,
 * and the results of a layer are the same bits whether it is passed alone or in a table with others.
 *
 * A layer is a matrix W (R, C) of fp32 values, dense and row-major (weight_orig reshaped to (Co, -1)), with the stored vectors u (R)
 * and v (C) and the hook's eps.  Where the layer ITERATES (the module is in training mode), in place,
 *     t = W^T u        v = t / max(|t|, eps)        s = W v        u = s / max(|s|, eps)
 * and where it does not, u and v are left alone and s = W v.  In both cases
 *     sigma = sum_r u_r s_r        W_sn = W / sigma                                    (a true division, as torch's)
 * Every sum over a row or a column is taken in fp64 (a product of two fp32 values is exact there) in ONE fixed order, and what is not
 * stored stays fp64: t, |t|, s and |s| are never rounded to fp32.  A STORED value is one rounding of its fp64 expression:
 * v_c = fp32(t_c / max(|t|, eps)), u_r = fp32(s_r / max(|s|, eps)) with s from the stored v, sigma = fp32(sum u_r s_r) with the stored u;
 * W_sn = W / sigma is an fp32 division by the stored sigma.  max(n, eps) keeps a NaN n.  A zero matrix gives sigma = 0 and a W_sn of
 * NaN, as torch's does.
 * The backward pass, with the u, v, sigma and W_sn of ITS forward (the forward writes copies of u and v for it) and G = dL/dW_sn:
 *     d = fp32(sum G * W_sn)  (fp64)        dW = (G - (d * u_r) * v_c) / sigma         (fp32, every operation rounded on its own)
 *
 * The orders of the sums, all functions of a layer's R and C alone:
 *   t_c     rows in parts of PS_SPECTRAL_PART_ROWS: inside a part ascending, then the parts ascending;
 *   s_r     a wavefront per row: lane l adds the columns 4 (l + 64 k) .. + 3, k ascending, then the lanes as a butterfly (lane ^ 1 .. ^ 32);
 *   |t|^2, |s|^2, sigma   a workgroup of 256: thread t adds the entries t, t + 256, ... ascending, the lanes of a wavefront as a
 *           butterfly, the four wavefronts ascending;
 *   d       the R C values in tiles of PS_SPECTRAL_TILE: inside a tile thread t adds the values 4 (t + 256 k) .. + 3, k ascending, lanes and
 *           wavefronts as above; then the tiles of the layer, tile j by thread j % 256, ascending, lanes and wavefronts as above.
 * Rows and tiles are read 16 bytes at a time where their addresses allow (C a multiple of 4 and a base aligned to 16 bytes) and value by
 * value elsewhere; which of the two does not change which thread adds what. */
#ifndef PIXELSYNTH_SPECTRAL_TRAIN_H
#define PIXELSYNTH_SPECTRAL_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_SPECTRAL_MAX_LAYERS 64       /* layers per table, at the most */
#define PS_SPECTRAL_PART_ROWS 16        /* rows of a part of W^T u */
#define PS_SPECTRAL_TILE 4096           /* values of a tile of the elementwise passes */
#define PS_SPECTRAL_FORWARD_LAUNCHES 5  /* kernels ps_spectral_forward_f32 queues, whatever the table holds */
#define PS_SPECTRAL_BACKWARD_LAUNCHES 2 /* kernels ps_spectral_backward_f32 queues */

/* Bytes of a table (the same for every number of layers); the caller keeps one image of it in host memory and one on the device. */
size_t ps_spectral_table_bytes(void);

/* Fill the host image `table` (table_bytes >= ps_spectral_table_bytes()) for n_layers layers, 1 .. PS_SPECTRAL_MAX_LAYERS: weights, us, vs
 * are HOST arrays of DEVICE addresses (W aligned to 4 bytes at least), rows / cols the sizes (R, C >= 1, R C < 2^31), iterate whether
 * layer k runs the power iteration, eps its eps (> 0).  interleave[k] = I says how the columns lie in memory: column m of the dense
 * (R, C) matrix at weights[k] is column (m % I) * (C / I) + m / I of W, the matrix u and v belong to (C % I == 0).  I = 1: as they
 * are; I = Ci: a (Co, Ci, kh, kw) convolution weight in channels-last storage.  W_sn, dW and the gradients have the layout of
 * weights[k]; v_saved is in memory order as well.  With I > 1 the sums over the columns (|t|^2, s_r) run in memory order: a layer's
 * bits are a function of R, C and I.  A pure host function: nothing is queued.  The caller copies the image to the
 * device (once: it changes only when an address, a size or a flag does) and passes both images to the calls below.
 * The flat buffers of the calls below hold layer k's values at offsets that are functions of the sizes in the table alone:
 *   elem_offsets[k]   of W_sn and dW, in values, a multiple of 4;    row_offsets[k] of the copies of u;    col_offsets[k] of those of v
 * (each n_layers + 1 entries, the last being the size of the buffer; any of the three may be NULL). */
int ps_spectral_plan(const void *const *weights, const void *const *us, const void *const *vs, const int *rows, const int *cols,
                     const int *interleave, const int *iterate, const float *eps, int n_layers, void *table, size_t table_bytes,
                     long long *elem_offsets, long long *row_offsets, long long *col_offsets);

/* Bytes of workspace both calls below need for the host image `table` (device memory, aligned to 16 bytes); 0 for a table
 * ps_spectral_plan did not fill. */
size_t ps_spectral_workspace_bytes(const void *table);

/* The forward pass of every layer of the table, PS_SPECTRAL_FORWARD_LAUNCHES kernels: u and v of the iterating layers updated in place,
 * w_sn (elem_offsets[n]) the normalised weights, u_saved (row_offsets[n]) and v_saved (col_offsets[n]) the vectors sigma was computed
 * with, sigma (n_layers).  table_host and table_device are the two images of one table; w_sn aligned to 16 bytes. */
int ps_spectral_forward_f32(const void *table_host, const void *table_device, float *w_sn, float *u_saved, float *v_saved, float *sigma,
                            void *workspace, size_t workspace_bytes, void *stream);

/* The backward pass, PS_SPECTRAL_BACKWARD_LAUNCHES kernels: grads is a HOST array of n_layers DEVICE addresses (they travel in the
 * kernels' arguments), each a dense (R, C) fp32 gradient aligned to 4 bytes or NULL, which stands for a gradient of zeros; w_sn, u_saved,
 * v_saved, sigma as the forward pass wrote them; dw (elem_offsets[n], aligned to 16 bytes) receives every layer's gradient.  Only the
 * sizes and offsets of the table are read: not W, u or v. */
int ps_spectral_backward_f32(const void *table_host, const void *table_device, const void *const *grads, const float *w_sn,
                             const float *u_saved, const float *v_saved, const float *sigma, float *dw, void *workspace,
                             size_t workspace_bytes, void *stream);

/* ps_spectral_train_last_error: the message of this library's last failed call. */
const char *ps_spectral_train_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_SPECTRAL_TRAIN_H */
