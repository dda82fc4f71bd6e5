/* C ABI of libmliis_region.so: the Tversky region term of the inner loop's loss on the MI355X (gfx950), on the focal, foreground-weighted
 * pixel term of include/mliis_loss.h -- the counterparts of mliis_focal_ce and mliis_head_focal_fused for a learner built with
 * tversky=(alpha, beta).  Same conventions as include/mliis_hip.h: fp32 NHWC device tensors, every call asynchronous on `stream`, no
 * allocation, no synchronisation, returns MLIIS_OK (0) or a negative MLIIS_ERR_* of mliis_hip.h; mliis_region_last_error() returns this
 * library's thread-local message.
 *
 * For image n, with p1 the channel-1 softmax of the logits and y1 the stored, UNSMOOTHED foreground label:
 *     I = sum p1 y1,   Sp = sum p1,   St = sum y1
 *     D_n = I + alpha (Sp - I) + beta (St - I) + eps,   T_n = (I + eps) / D_n,   eps = 1e-7
 *     T = mean_n T_n
 *     loss = L_pix - ln(2 T / (T + 1)) + extra_loss
 * L_pix is the pixel term of include/mliis_loss.h (gamma = 0, fg_weight = 1: the cross-entropy); label smoothing applies to L_pix only.
 * alpha = beta = 1 is the soft IoU (the dice term of mliis_softmax_ce), alpha = beta = 1/2 the soft Dice coefficient; beta > alpha
 * weighs a missed foreground pixel more than a false alarm.  The region term's gradient w.r.t. z1 (w.r.t. z0: its negative), with
 * dL/dT = -1 / (T (T + 1)):
 *     dp1_i = (A_n y1_i - B_n (alpha + (1 - alpha - beta) y1_i)) p1_i (1 - p1_i)
 *     A_n = (1 / D_n) (dL/dT) / N,   B_n = ((I + eps) / D_n^2) (dL/dT) / N
 *     out[0] = loss,   out[1] = L_pix,   out[2] = the soft IoU (alpha = beta = 1) whatever alpha and beta are;   out[3] is not written.
 * Partial sums are per workgroup, folded in double precision in a fixed order (no atomics, no fences): the same inputs give the same bits.
 *
 * Refused before any launch, with nothing written (MLIIS_ERR_ARG unless noted): a null required pointer; N, H or W (Hd, Wd) not positive
 * or out of range; alpha or beta negative or not finite, or alpha + beta = 0; gamma negative or not finite; fg_weight not positive or
 * not finite; label_smoothing outside [0, 1); a workspace smaller than the size query's answer or not 16-byte aligned
 * (MLIIS_ERR_WORKSPACE); tensors not 8-byte aligned (MLIIS_ERR_ALIGN). */
#ifndef MLIIS_REGION_H_
#define MLIIS_REGION_H_

#include <stddef.h>

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

const char* mliis_region_last_error(void);

/* Floats of the workspace of mliis_tversky_ce (no device work; 0 when N, H or W is not positive). */
size_t mliis_tversky_ce_workspace_floats(int N, int H, int W);

/* logits [N,H,W,2]; labels [S,H,W,2] addressed through img_idx (nullable: image n reads label n).  Writes out[0..2] (device) and
 * dlogits [N,H,W,2] (nullable: no gradient is written, two launches).  N <= 65535, H W <= 2^29.  Three launches: partial sums, the
 * fold, the gradient.  The region term is always on. */
int mliis_tversky_ce(const float* logits, const float* labels, const int* img_idx, int N, int H, int W, float label_smoothing, float gamma,
                     float fg_weight, float alpha, float beta, float extra_loss, float* dlogits, float* out, float* ws, size_t ws_floats,
                     hipStream_t stream);

/* 1 when mliis_head_tversky_fused takes this pair of maps, else 0 (use mliis_resize_bilinear_fwd -> mliis_tversky_ce ->
 * mliis_resize_bilinear_bwd): the predicate of mliis_head_ce_fused_supported, the same tiling. */
int mliis_head_tversky_fused_supported(int Hd, int Wd, int H, int W);
size_t mliis_head_tversky_fused_workspace_floats(int N, int Hd, int Wd, int H, int W);

/* The training step's tail with the region term: small [N,Hd,Wd,2] = the final conv's output on the decoder's map; logits = bilinear
 * resize (align_corners) to [H,W]; the loss above against labels [S,H,W,2]; dsmall [N,Hd,Wd,2] = the gradient w.r.t. small -- what
 * mliis_resize_bilinear_fwd -> mliis_tversky_ce -> mliis_resize_bilinear_bwd compute, by the same per-pixel arithmetic, with no
 * full-resolution tensor written.  The region gradient needs the images' sums first, so the head makes two passes over the decoder's
 * map, three launches: the sums (every image pixel's logits rebuilt from small, partial sums per workgroup), the fold into out[0..2] and
 * the images' {A_n, B_n}, then the gradient tiles (8 x 8 decoder pixels each, an image-side footprint of at most 48 x 48 in LDS).
 * MLIIS_ERR_UNSUPPORTED when mliis_head_tversky_fused_supported is 0. */
int mliis_head_tversky_fused(const float* small, const float* labels, const int* img_idx, int N, int Hd, int Wd, int H, int W,
                             float label_smoothing, float gamma, float fg_weight, float alpha, float beta, float extra_loss, float* dsmall,
                             float* out, float* ws, size_t ws_floats, hipStream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
