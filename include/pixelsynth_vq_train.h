/* pixelsynth_vq_train.h -- the C ABI of libpixelsynth_vq_train.so: the training half of the VQ-VAE's quantiser (csrc/vq_train.hip; the
 * reference's Quantize.forward in training mode, models/vqvae2/vqvae.py:41-74) -- the straight-through output and the commitment
 * term, the per-code statistics, the EMA update of the codebook, and the backward pass.  The codes themselves are ps_vq_nearest_f32's
 * (libpixelsynth_hip.so), whose pinned set of exports this library leaves as it is.  Same conventions: int status, 0 = success,
 * ps_vq_train_last_error() says why not; every buffer and the workspace are the caller's; the last parameter is the stream; no
 * allocation, no synchronisation, no device-to-host copy, no atomics.  Every result is bit-identical from run to run.
 *
 * Notation: z (N,D) row-major, the latent vectors; idx (N) int32, their codes; embed (D,K), the codebook as the module keeps it;
 * rows (K,D), the same codebook transposed (one code per row: what a gather reads); D <= 64 (the limit of ps_vq_nearest_f32).  A code
 * outside 0 .. K-1 selects a row of zeros in the gathers and counts for no code in the statistics. */
#ifndef PIXELSYNTH_VQ_TRAIN_H
#define PIXELSYNTH_VQ_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The N vectors are split into parts of consecutive rows, each a multiple of PS_VQ_TRAIN_PART_ROWS rows long, the smallest multiple
 * that gives at most PS_VQ_TRAIN_MAX_PARTS parts: rows per part = PART_ROWS * ceil(ceil(N / PART_ROWS) / MAX_PARTS).  A function of
 * N alone.  A per-code sum is one fused-multiply-add chain per part, in ascending row, and the parts are added in ascending order. */
#define PS_VQ_TRAIN_MAX_PARTS 128
#define PS_VQ_TRAIN_PART_ROWS 512

/* Bytes of workspace the entry points below need for these sizes (device memory, 256-byte aligned; one size serves all of them);
 * 0 for sizes they refuse: N, D, K < 1, D > 64, N > 2^30, K > 2^20. */
size_t ps_vq_train_workspace_bytes(int N, int D, int K);

/* counts[k]  = #{n : idx[n] = k}                       (K) int32
 * sums[d][k] = sum_{n : idx[n] = k} z[n][d]            (D,K) like embed
 * The segmented sum is the product z^T (D x N) . onehot (N x K) on v_mfma_f32_16x16x4_f32: the A operand a 16-channel x 4-row slice
 * of z, the B operand idx[n] == k ? 1 : 0 built in registers; products with 0 and 1 are exact, so a sum is the fp32 additions of its
 * terms in ascending row within a part.  One wave per (part, 32 codes); D and K padded to 16 in the workspace.  The counts are integer
 * adds in the same waves. */
int ps_vq_train_stats_f32(const float *z, const int32_t *idx, int N, int D, int K, int32_t *counts, float *sums, void *workspace,
                          size_t workspace_bytes, void *stream);

/* r = rows[idx[n]][d] - z[n][d] (one fp32 rounding); quantize[n][d] = z[n][d] + r (N,D): the straight-through output, the reference's
 * value; diff[0] = mean(r^2), the squares and their sum in fp64 (one partial per workgroup of 16384 elements, a fixed tree inside,
 * the partials added in ascending order), rounded to fp32 at the end. */
int ps_vq_train_quantize_f32(const float *z, const int32_t *idx, const float *rows, int N, int D, int K, float *quantize, float *diff,
                             void *workspace, size_t workspace_bytes, void *stream);

/* The EMA update (vqvae.py:60-69), cluster_size (K) and embed_avg (D,K) in place, the new codebook to embed_out (D,K):
 *   cluster_size <- decay * cluster_size + alpha * counts         embed_avg <- decay * embed_avg + alpha * sums
 *   n = sum_k cluster_size (fp64, ascending k, rounded to fp32)   s = (cluster_size + eps) / (n + K * eps) * n
 *   embed_out = embed_avg / s
 * fp32, every product and sum rounded on its own.  alpha is the caller's 1 - decay (computed in double, as the reference does).
 * embed_out may be the codebook itself; it must not overlap the other buffers. */
int ps_vq_train_update_f32(const int32_t *counts, const float *sums, int D, int K, float decay, float alpha, float eps,
                           float *cluster_size, float *embed_avg, float *embed_out, void *workspace, size_t workspace_bytes,
                           void *stream);

/* grad_input[n][d] = grad_quantize[n][d] + grad_diff[0] * 2 / (N D) * (z[n][d] - rows[idx[n]][d])      (N,D)
 * grad_quantize (N,D) and grad_diff (one float, on the device) may each be NULL and then count as zero, not both.  The factor
 * grad_diff * 2 / (N D) is kept in fp64; z - rows is rounded once in fp32, the product once, the sum once.  With grad_diff zero (or
 * NULL) grad_input is grad_quantize bit for bit. */
int ps_vq_train_backward_f32(const float *z, const int32_t *idx, const float *rows, const float *grad_quantize, const float *grad_diff,
                             int N, int D, int K, float *grad_input, void *stream);

/* ps_vq_train_last_error: the message of this library's last failed call. */
const char *ps_vq_train_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PIXELSYNTH_VQ_TRAIN_H */
