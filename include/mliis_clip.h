/* C ABI of libmliis_clip.so: the inner loop's gradient clipping on the MI355X (gfx950).  Two launches between the backward pass and the
 * optimizer launch bound the packed gradient arena IN PLACE -- by its global L2 norm, or per tensor by a ratio of that tensor's parameter
 * norm -- and write one record per scale into a row of a ring in device memory; the row is taken from a device cursor the first launch
 * advances itself, so a captured graph that holds the launches fills a new row at every replay.  Same conventions as
 * include/mliis_layerlog.h: every call asynchronous on `stream`, no allocation, no synchronisation, returns MLIIS_OK (0) or a negative
 * MLIIS_ERR_* of mliis_hip.h; mliis_clip_last_error() returns this library's thread-local message. */
#ifndef MLIIS_CLIP_H_
#define MLIIS_CLIP_H_

#include <stddef.h>

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define MLIIS_CLIP_NORM 0  /* one scale for the whole gradient: s = C / ||g|| when ||g|| > C, otherwise exactly 1 */
#define MLIIS_CLIP_RATIO 1 /* one scale per tensor t: ref_t = LAMBDA * max(||theta_t||, eps), s_t = ref_t / ||g_t|| when ||g_t|| > ref_t */

const char* mliis_clip_last_error(void);

/* Size queries (no device work): the 16-byte quads of one chunk (the unit of work of both launches: mliis_amd/layerlog.py's chunk_table
 * builds the table from it), the bytes of the workspace a table of nchunks chunks and T tensors needs (0 when nchunks < 1 or T < 1), and
 * the 32-bit words of one record (8). */
int mliis_clip_chunk_quads(void);
size_t mliis_clip_workspace_bytes(int nchunks, int T);
int mliis_clip_record_words(void);

/* Clip the gradient arena g (n floats, n a positive multiple of 4; read and written with 16-byte accesses) and write R records into one
 * ring row: R = 1 in MLIIS_CLIP_NORM, R = T in MLIIS_CLIP_RATIO.  theta: the parameter arena of the same layout, read only, used in
 * MLIIS_CLIP_RATIO alone (may be null in MLIIS_CLIP_NORM).  The tables are the per-tensor log's (include/mliis_layerlog.h), int32, in
 * device memory, validated by the CALLER (they are addresses the kernels follow):
 *   chunks [nchunks][4] = {tensor, first quad (of the arena), quads (1 .. chunk_quads), valid elements (4 quads - 3 .. 4 quads)}
 *   segs   [T][4]       = {first quad, element count, first chunk, one past the last chunk}
 * ||.|| is the L2 norm over a tensor's counted elements (all tensors' in MLIIS_CLIP_NORM), squared and summed in double; the floats
 * between a tensor's count and its 4-float padded extent enter no norm.  threshold: C or LAMBDA; eps: the floor of ||theta_t||
 * (MLIIS_CLIP_RATIO; ignored in MLIIS_CLIP_NORM).  A scale is formed in double, rounded once to fp32 (and kept at or above FLT_MIN), and
 * every float of the tensor's quads -- its padding too, which stays zero when it was zero -- becomes the ONE fp32 product g * s
 * (round to nearest even, no fused multiply-add); a product below FLT_MIN is the IEEE subnormal (the kernels run with fp32 subnormals
 * on), not a flushed zero.  Where s is exactly 1 nothing is stored.  ||theta_t|| is taken over theta's finite elements.
 * NON-FINITE GRADIENTS ARE NOT FILTERED: if any counted element of g is NaN or +-inf, in either mode and in whichever tensor, no float
 * of g is written, every scale is 1 and every record of the row carries the bypassed flag.
 * Record r (0 in MLIIS_CLIP_NORM, the tensor in MLIIS_CLIP_RATIO), 8 words, at ring[(row * R + r) * 8] with row = *cursor % capacity
 * (*cursor as the first launch found it; the counter runs modulo 2^32):
 *   0  f32 g_l2       the pre-clip norm over the FINITE counted elements, rounded once to f32
 *   1  f32 ref        C, or ref_t rounded once to f32
 *   2  f32 scale      the factor that was applied (1 when not clipped or bypassed)
 *   3  u32 nonfinite  NaN / +-inf counted elements of this record's part of g, saturating at 2^32 - 1
 *   4  u32 flags      bit 0: clipped (norm > ref and not bypassed), bit 1: bypassed
 *   5-7               zero
 * TWO launches ordered by the stream, in both modes, one workgroup per chunk each.  The first leaves one partial per chunk in ws (sums
 * of squares of g and, in MLIIS_CLIP_RATIO, of theta, and the non-finite count; an element order fixed by the table); its first
 * workgroup stores row into ws and *cursor + 1 into *cursor.  In the second every workgroup folds the partials it needs -- all chunks',
 * and in MLIIS_CLIP_RATIO its own tensor's -- in an order that depends on the table alone, so that all workgroups of a scale arrive at
 * the same bits, multiplies its chunk, and the workgroup of a record's first chunk writes the record.  The kernel boundary is the only
 * synchronisation -- no counter, no fence, no atomic -- and the same inputs give the same bits.  ws: ws_bytes >=
 * mliis_clip_workspace_bytes(nchunks, T), owned by this clip (its contents before the call do not matter); launches that share a ws, a
 * cursor or g must be ordered on one stream.  Only g, that ring row, ws and *cursor are written.
 * Refused before any launch: a null g, chunks, segs, ws, ring or cursor (theta in MLIIS_CLIP_RATIO), a mode that is neither, n < 4 or
 * n % 4 != 0, T < 1, nchunks < T or nchunks > n / 4, capacity < 1, ws_bytes too small, a threshold (eps in MLIIS_CLIP_RATIO) that is not
 * finite and positive (MLIIS_ERR_ARG); g, theta, chunks, segs, ws or ring not 16-byte aligned, cursor not 4-byte aligned
 * (MLIIS_ERR_ALIGN). */
int mliis_clip_apply(int mode, float* g, const float* theta, long long n, const int* chunks, int nchunks, const int* segs, int T,
                     float threshold, float eps, void* ws, size_t ws_bytes, void* ring, int capacity, unsigned* cursor,
                     hipStream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
