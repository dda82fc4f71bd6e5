/* C ABI of libmliis_score.so: evaluation scores counted on the MI355X (gfx950).  Same conventions as include/mliis_hip.h: fp32 NHWC
 * device tensors, every call asynchronous on `stream`, returns MLIIS_OK (0) or a negative MLIIS_ERR_* of mliis_hip.h;
 * mliis_score_last_error() returns this library's thread-local message. */
#ifndef MLIIS_SCORE_H_
#define MLIIS_SCORE_H_

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

const char* mliis_score_last_error(void);

/* The score of an evaluation batch without its mask (reptile.py:526-549 on the device): small [N,Hd,Wd,2] = the final conv's output on
 * the decoder's map, labels [S,H,W,2] (through img_idx, nullable); counts (device int32 [N][4]) = {|P & L|, |P | L|, |P|, |L|} per
 * image: P = the channel-1 prediction exactly as mliis_resize_bilinear_fwd -> mliis_softmax_ce(pred) form it (same resize arithmetic,
 * softmax, p1 > 0.5: near-ties fall the same way), L = label channel 1 rounded half to even, != 0.
 * IoU = (counts[0] + eps) / (counts[1] + eps).  Any Hd <= H, Wd <= W with H, W > 1 (else MLIIS_ERR_ARG); small / labels 8-byte aligned; the
 * full-resolution logits and the mask are never written; no workspace (the launch sequence zeroes counts, then adds integers). */
int mliis_mask_iou_counts(const float* small, const float* labels, const int* img_idx, int N, int Hd, int Wd, int H, int W, int* counts,
                          hipStream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
