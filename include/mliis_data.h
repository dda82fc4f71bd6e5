/* C ABI of libmliis_data.so: a task's shots made resident from the bytes a dataset stores, on the MI355X (gfx950).  Same conventions as
 * include/mliis_hip.h: fp32 NHWC device outputs, every call asynchronous on `stream`, no workspace, no allocation, no synchronisation,
 * returns MLIIS_OK (0) or a negative MLIIS_ERR_* of mliis_hip.h; mliis_data_last_error() returns this library's thread-local message. */
#ifndef MLIIS_DATA_H_
#define MLIIS_DATA_H_

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

const char* mliis_data_last_error(void);

/* Expand (and resample) S examples of a byte pool into the float tensors the training step reads: images [n,h,w,3] uint8, masks [n,h,w]
 * uint8 (device), src_idx (device int32 [S], nullable = rows 0..S-1; an entry outside [0, n) is clamped into it, so nothing outside the
 * pool is read), x [S,H,W,3] and y [S,H,W,2] fp32, 16-byte aligned; every element of x and y is written once, nothing else is.
 *   h == H and w == W:  x = float(byte);  y[...,0] = (255 - m) / 255,  y[...,1] = m / 255, both correctly rounded in fp32 (a table of the
 *     256 quotients) -- the arrays of tfrecord.parse_example, bit for bit.
 *   otherwise:  the mask byte is the nearest sample at half-pixel centres in integers, source row = ((2 i + 1) h) / (2 H) (columns alike),
 *     and the label is formed from it as above; the image is bilinear at half-pixel centres with clamped edges (align_corners = false,
 *     no antialiasing): num = clamp((2 i + 1) h - H, 0, 2 H (h - 1)), i0 = num / (2 H), i1 = min(i0 + 1, h - 1),
 *     f = float(num % (2 H)) / float(2 H), columns alike; along the row first, then between the rows, each step a + (b - a) f in fp32.
 * Refused before any launch: a null pointer other than src_idx, or S, n, h, w, H, W < 1 (MLIIS_ERR_ARG); x or y not 16-byte aligned
 * (MLIIS_ERR_ALIGN); h, w, H or W > 16384 or more than 2^31 - 1 output pixels (MLIIS_ERR_UNSUPPORTED).  The pool needs no alignment and
 * any row pitch (3 w bytes) works; 4-byte aligned pools with h w a multiple of 4 are read a word at a time at the same size. */
int mliis_task_expand_u8(const unsigned char* images, const unsigned char* masks, const int* src_idx, int S, int n, int h, int w, int H,
                         int W, float* x, float* y, hipStream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
