/* C ABI of libmliis_layerlog.so: the inner loop's per-tensor log on the MI355X (gfx950).  Two launches at the tail of a training step
 * reduce the packed gradient and parameter arenas PER TENSOR and write one record per tensor into a row of a ring in device memory; the
 * row is taken from the step log's device cursor (include/mliis_steplog.h), which this library only reads, so record k of the step log and
 * row k of this ring describe the same step and a captured graph that holds the launches fills a new row at every replay.  Same
 * conventions as include/mliis_hip.h: every call asynchronous on `stream`, no allocation, no synchronisation, returns MLIIS_OK (0) or a
 * negative MLIIS_ERR_* of mliis_hip.h; mliis_layerlog_last_error() returns this library's thread-local message. */
#ifndef MLIIS_LAYERLOG_H_
#define MLIIS_LAYERLOG_H_

#include <stddef.h>

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define MLIIS_LAYERLOG_STEP 0  /* X = x (the gradient arena), Y = y (the parameter arena) */
#define MLIIS_LAYERLOG_DELTA 1 /* X = x - y element by element (one fp32 subtraction), Y = y */

const char* mliis_layerlog_last_error(void);

/* Size queries (no device work): the 16-byte quads of one chunk (the unit of work of the first launch: mliis_amd/layerlog.py builds the
 * chunk table from it), the bytes of the workspace a table of nchunks chunks needs (0 when nchunks < 1), and the 32-bit words of one
 * record (8). */
int mliis_layerlog_chunk_quads(void);
size_t mliis_layerlog_workspace_bytes(int nchunks);
int mliis_layerlog_record_words(void);

/* Write the T records of one row.  x, y: two fp32 arenas of n floats each (n a positive multiple of 4), read with 16-byte loads and never
 * written.  A tensor (segment) of the arenas is {first quad, element count >= 1}; the floats between its count and its 4-float padded
 * extent are read into no statistic.  Tables, int32, in device memory, validated by the CALLER (they are addresses the kernels follow):
 *   chunks [nchunks][4] = {tensor, first quad (of the arena), quads (1 .. chunk_quads), valid elements (4 quads - 3 .. 4 quads)}
 *   segs   [T][4]       = {first quad, element count, first chunk, one past the last chunk}
 * The chunks of a tensor are consecutive, ascending, and tile its quads exactly.  Record of tensor t, 8 words, at
 * ring[(row * T + t) * 8] with row = ((cursor ? *cursor : 0) + row_offset, modulo 2^32 like the step log's counter) % capacity:
 *   0  f32 x_l2         sqrt of the sum of squares of the FINITE elements of X, summed in double, rounded once to f32
 *   1  f32 x_absmax     the largest |x| over the finite elements of X (0 when there is none)
 *   2  f32 y_l2         the same two for Y
 *   3  f32 y_absmax
 *   4  u32 x_nonfinite  NaN / +-inf elements of X, saturating at 2^32 - 1
 *   5  u32 y_nonfinite  the same for Y
 *   6  u32 x_first      the lowest element index within the tensor of a non-finite element of X, 0xffffffff when there is none
 *   7  u32 y_first      the same for Y
 * Two launches ordered by the stream: the first writes one partial per chunk into ws (one workgroup per chunk, an element order fixed by
 * the table), the second folds each tensor's partials in chunk order and writes its record.  The kernel boundary is the only
 * synchronisation -- no counter, no fence, no atomic -- and the same inputs give the same bits.  ws: ws_bytes >=
 * mliis_layerlog_workspace_bytes(nchunks), owned by this log (its contents before the call do not matter); launches that share a ws or a
 * ring row must be ordered on one stream.  Only that row and ws are written; *cursor is read, never written.
 * Refused before any launch: a null x, y, chunks, segs, ws or ring, a mode that is neither, n < 4 or n % 4 != 0, T < 1, nchunks < T or
 * nchunks > n / 4, capacity < 1, ws_bytes too small (MLIIS_ERR_ARG); x, y, chunks, segs, ws or ring not 16-byte aligned, cursor not 4-byte
 * aligned (MLIIS_ERR_ALIGN). */
int mliis_layerlog_append(int mode, const float* x, const float* y, long long n, const int* chunks, int nchunks, const int* segs, int T,
                          void* ws, size_t ws_bytes, void* ring, int capacity, const unsigned* cursor, unsigned row_offset,
                          hipStream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
