/* C ABI of libmliis_loss.so: the focal, foreground-weighted form of the inner loop's pixel loss on the MI355X (gfx950) -- the counterparts
 * of mliis_softmax_ce and mliis_head_ce_fused (include/mliis_hip.h) for a learner built with focal_gamma != 0 or fg_weight != 1.  Same
 * conventions as include/mliis_hip.h: fp32 NHWC device tensors, every call asynchronous on `stream`, no allocation, no synchronisation,
 * returns MLIIS_OK (0) or a negative MLIIS_ERR_* of mliis_hip.h; mliis_loss_last_error() returns this library's thread-local message.
 *
 * Per pixel, with z = (z0, z1) the logits, (l0, l1) = log_softmax(z), (p0, p1) = softmax(z), (y0, y1) the stored labels,
 * t_c = y_c (1 - ls) + ls / 2 the smoothed targets, w = 1 + (fg_weight - 1) y1 the pixel's weight (from the UNSMOOTHED label) and
 * gamma >= 0:
 *     l     = -w ( t0 exp(gamma l1) l0 + t1 exp(gamma l0) l1 )
 *     L_pix = sum(l) / (N H W)                      (the divisor of the cross-entropy: NOT sum(w))
 *     dl/dz1 = -dl/dz0 = w ( t1 [gamma exp(gamma l0) p1 l1 - exp(gamma l0) p0] - t0 [gamma exp(gamma l1) p0 l0 - exp(gamma l1) p1] )
 * In the two-class case (1 - p_c)^gamma is the other class's probability to the power gamma: it is formed as exp(gamma l_other) -- no
 * powf, no 1 - p, no log(p): everything comes from the log-softmax, so saturated logits stay finite.  gamma = 0, fg_weight = 1 is the
 * cross-entropy of mliis_softmax_ce.  The dice term (-ln(2 iou / (iou + 1)), iou = the mean over images of (I + 1e-7) / (U + 1e-7) on the
 * channel-1 probability) and extra_loss compose with it exactly as they do there:
 *     out[0] = L_pix (+ dice term) + extra_loss,   out[1] = L_pix,   out[2] = iou (also when the dice term is off).
 * Partial sums are per workgroup, folded in double precision in a fixed order (no atomics, no fences): the same inputs give the same bits.
 *
 * Refused before any launch, with nothing written (MLIIS_ERR_ARG unless noted): a null required pointer; N, H or W (Hd, Wd) not positive
 * or out of range; gamma negative or not finite; fg_weight not positive or not finite; label_smoothing outside [0, 1); a workspace
 * smaller than the size query's answer or not 16-byte aligned (MLIIS_ERR_WORKSPACE); tensors not 8-byte aligned (MLIIS_ERR_ALIGN). */
#ifndef MLIIS_LOSS_H_
#define MLIIS_LOSS_H_

#include <stddef.h>

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

const char* mliis_loss_last_error(void);

/* Floats of the workspace of mliis_focal_ce (no device work; 0 when N, H or W is not positive). */
size_t mliis_focal_ce_workspace_floats(int N, int H, int W);

/* logits [N,H,W,2]; labels [S,H,W,2] addressed through img_idx (nullable: image n reads label n).  Writes out[0..2] (device) and
 * dlogits [N,H,W,2] (nullable: no gradient is written).  N <= 65535, H W <= 2^29.  Launches: partial sums, the fold, the gradient; without
 * the dice term the gradient does not depend on the fold, which then rides in the gradient launch's first workgroup (two launches).  There
 * is no prediction mask: evaluation keeps mliis_softmax_ce. */
int mliis_focal_ce(const float* logits, const float* labels, const int* img_idx, int N, int H, int W, float label_smoothing, float gamma,
                   float fg_weight, int dice, float extra_loss, float* dlogits, float* out, float* ws, size_t ws_floats, hipStream_t stream);

/* 1 when mliis_head_focal_fused takes this pair of maps, else 0 (use mliis_resize_bilinear_fwd -> mliis_focal_ce ->
 * mliis_resize_bilinear_bwd): the predicate of mliis_head_ce_fused_supported, the same tiling. */
int mliis_head_focal_fused_supported(int Hd, int Wd, int H, int W);
size_t mliis_head_focal_fused_workspace_floats(int N, int Hd, int Wd);

/* The training step's tail without the dice term: small [N,Hd,Wd,2] = the final conv's output on the decoder's map; logits = bilinear
 * resize (align_corners) to [H,W]; the loss above against labels [S,H,W,2]; dsmall [N,Hd,Wd,2] = the gradient w.r.t. small -- what
 * mliis_resize_bilinear_fwd -> mliis_focal_ce -> mliis_resize_bilinear_bwd compute, by the same per-pixel arithmetic, with no
 * full-resolution tensor written.  Two launches: the tiles (8 x 8 decoder pixels each, an image-side footprint of at most 48 x 48 in LDS,
 * one owner tile per image pixel for the loss terms), then the fold into out[0..2].  MLIIS_ERR_UNSUPPORTED when
 * mliis_head_focal_fused_supported is 0. */
int mliis_head_focal_fused(const float* small, const float* labels, const int* img_idx, int N, int Hd, int Wd, int H, int W,
                           float label_smoothing, float gamma, float fg_weight, float extra_loss, float* dsmall, float* out, float* ws,
                           size_t ws_floats, hipStream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
