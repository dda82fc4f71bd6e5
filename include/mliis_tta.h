/* C ABI of libmliis_tta.so: flip test-time augmentation at evaluation -- the mirrored copy of an input batch and the merge of the views'
 * decoder-resolution logits, on the MI355X (gfx950).  Same conventions as include/mliis_hip.h and include/mliis_score.h: fp32 NHWC device
 * tensors, every call asynchronous on `stream`, returns MLIIS_OK (0) or a negative MLIIS_ERR_* of mliis_hip.h; mliis_tta_last_error()
 * returns this library's thread-local message.  Every argument is checked before anything is launched. */
#ifndef MLIIS_TTA_H_
#define MLIIS_TTA_H_

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

const char* mliis_tta_last_error(void);

/* dst[n,h,w,c] = src[img_idx ? img_idx[n] : n, flip_rows ? H-1-h : h, flip_cols ? W-1-w : w, c]: images img_idx (device int32 [N],
 * nullable; repeats and permutations allowed; the caller keeps them inside src's pool) of src [S,H,W,C], mirrored, as the dense batch dst
 * [N,H,W,C].  The 32-bit words are copied, no arithmetic touches them; with both flags 0 it is a plain gather.  Any N, H, W >= 1 and
 * 1 <= C <= 4 with N H W C <= 2^31 - 1.  Every element of dst is written exactly once and nothing else is; src is only read.  dst must
 * not overlap src[0 .. N) (dst == src is refused; with img_idx the caller keeps dst outside the rest of the pool).  4-byte alignment is
 * enough: 16-byte stores are used when dst is 16-byte aligned and W C is a multiple of 4, a word per thread otherwise.  One launch. */
int mliis_view_gather(const float* src, const int* img_idx, int N, int H, int W, int C, int flip_rows, int flip_cols, float* dst,
                      hipStream_t stream);

/* dst[n,h,w,c] = (a[n,h,w,c] + b[n, flip_rows ? Hd-1-h : h, flip_cols ? Wd-1-w : w, c]) * scale, all [N,Hd,Wd,C] fp32: the addition and
 * the multiplication are rounded once each (no fused form); a == NULL: dst = b[...] * scale, no addition (with scale == 1 the words of b
 * as they are, a -0.0 included).  dst == a is allowed (in place: every thread reads the elements it writes); any other overlap of dst
 * with a, and any overlap with b (dst == b), is refused.  scale must be finite and positive.  Non-finite inputs propagate as the IEEE
 * arithmetic dictates; nothing is filtered.  Sizes, C and alignment as for mliis_view_gather (16-byte accesses when dst, a and b are
 * 16-byte aligned and Wd C is a multiple of 4).  One launch. */
int mliis_view_merge(float* dst, const float* a, const float* b, int N, int Hd, int Wd, int C, int flip_rows, int flip_cols, float scale,
                     hipStream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
