/* C ABI of libmliis_sweep.so: the evaluation threshold sweep -- per-image histograms of the foreground probability, split by label
 * class, on the MI355X (gfx950).  Same conventions as include/mliis_hip.h and include/mliis_score.h: fp32 NHWC device tensors, every
 * call asynchronous on `stream`, returns MLIIS_OK (0) or a negative MLIIS_ERR_* of mliis_hip.h; mliis_sweep_last_error() returns this
 * library's thread-local message. */
#ifndef MLIIS_SWEEP_H_
#define MLIIS_SWEEP_H_

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

const char* mliis_sweep_last_error(void);

/* Bins per label class: 256. */
int mliis_prob_hist_bins(void);

/* hist (device uint32 [N][2][256]) of an evaluation batch: small [N,Hd,Wd,2] = the final conv's output on the decoder's map, labels
 * [S,H,W,2] (through img_idx, nullable), exactly the arguments of mliis_mask_iou_counts.  For every image pixel p1 = the channel-1
 * probability as mliis_mask_iou_counts forms it (the resize arithmetic of mliis_resize_bilinear_fwd, the softmax of mliis_softmax_ce);
 * its bin is b = clamp((int)ceilf(p1 * 256) - 1, 0, 255) -- bin b holds p1 in (b/256, (b+1)/256], bin 0 holds p1 == 0 as well; p1 * 256
 * is exact in fp32, so p1 > k/256 <=> b >= k for k = 1..255 and the counts mliis_mask_iou_counts writes are those of k = 128 -- and its
 * class is c = (label channel 1 rounded half to even != 0).  hist[n][c][b] = the number of pixels of image n with class c and bin b.
 * Two launches (zero, count); integer adds only, so the result does not depend on the order the workgroups arrive in; no workspace.
 * Shapes, sizes and alignment are checked as by mliis_mask_iou_counts (any Hd <= H, Wd <= W with H, W > 1, N <= 65535, H*W within 32-bit
 * pixel counts, small / labels 8-byte aligned); hist 4-byte aligned.  Nothing is launched when a check fails. */
int mliis_prob_histogram(const float* small, const float* labels, const int* img_idx, int N, int Hd, int Wd, int H, int W, unsigned* hist,
                         hipStream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
