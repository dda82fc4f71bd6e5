/* C ABI of libmliis_score.so: evaluation scores counted, and prediction masks bit-packed, on the MI355X (gfx950).  Same conventions as include/mliis_hip.h: fp32 NHWC
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

/* The mask itself, one bit per pixel.  mliis_mask_pack_words: 64-bit words per image = ceil(H*W / 64) (<= 0 on bad arguments).
 * mliis_mask_pack: bits (device, [N][words], 8-byte aligned): bit l of word w of image n = P of linear pixel 64*w + l (pixel = ho*W + wo;
 * linear over the image: words may straddle rows, rows are not padded), P the channel-1 prediction mliis_mask_iou_counts scores, near-ties
 * included; the bits of the last word beyond H*W are written as 0.  Every word of every image is written exactly once (bits need not be
 * cleared) and nothing past N*words is touched.  labels and counts: both null (one launch, no counts work) or both given -- then
 * counts[n] is what mliis_mask_iou_counts writes (its zeroing launch in front, the same integer atomics), img_idx nullable as there; one
 * of the two alone, or bits null: MLIIS_ERR_ARG.  Shapes, alignment and sizes are checked as by mliis_mask_iou_counts. */
long long mliis_mask_pack_words(int H, int W);
int mliis_mask_pack(const float* small, const float* labels, const int* img_idx, int N, int Hd, int Wd, int H, int W,
                    unsigned long long* bits, int* counts, hipStream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
