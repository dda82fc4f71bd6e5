/* C ABI of libmliis_steplog.so: the inner loop's step log on the MI355X (gfx950).  One launch at the tail of a training step appends a
 * record of that step -- its loss scalars, the learning rate, the norm and the largest magnitude of the packed gradient, the number of
 * non-finite gradient and parameter elements -- to a ring in device memory; the host reads the ring when it wants to.  Same conventions as
 * include/mliis_hip.h: every call asynchronous on `stream`, no allocation, no synchronisation, returns MLIIS_OK (0) or a negative
 * MLIIS_ERR_* of mliis_hip.h; mliis_steplog_last_error() returns this library's thread-local message. */
#ifndef MLIIS_STEPLOG_H_
#define MLIIS_STEPLOG_H_

#include <stddef.h>

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

const char* mliis_steplog_last_error(void);

/* Size queries (no device work): the bytes of the workspace one log needs, and the 32-bit words of one record (8). */
size_t mliis_steplog_workspace_bytes(void);
int mliis_steplog_record_words(void);

/* Append one record.  loss4: the step's {loss, cross-entropy, soft IoU, -} as the head's finalize left them; lr_dev: the device learning
 * rate; grad, theta: the packed gradient and parameter arenas, n floats each (n a positive multiple of 4), read once with 16-byte loads and
 * never written.  ring: capacity records of 8 words; cursor: a device uint32, the number of records appended so far (modulo 2^32).  The
 * launch writes ring[*cursor % capacity] and stores *cursor + 1: the position is read on the device, so a captured graph that holds the
 * launch appends a new record at every replay.  Record words:
 *   0..2  f32 loss, ce, iou      loss4[0..2], bit for bit
 *   3     f32 lr                 *lr_dev, bit for bit
 *   4     f32 grad_l2            sqrt of the sum of squares of the FINITE elements of grad, summed in double, rounded once to f32
 *   5     f32 grad_absmax        the largest |g| over the finite elements of grad (0 when there is none)
 *   6     u32 grad_nonfinite     NaN / +-inf elements of grad, saturating at 2^32 - 1
 *   7     u32 theta_nonfinite    NaN / +-inf elements of theta, saturating
 * The grid and every thread's element sequence are fixed and the partial sums are folded in index order by the last workgroup to finish:
 * the same inputs give the same bits.  ws: mliis_steplog_workspace_bytes() bytes owned by this log, ZERO before its first launch (it holds
 * the arrival counter, which every launch leaves at zero again); launches that share a ws, ring or cursor must be ordered on one stream.
 * Only the one record, *cursor and ws are written.
 * Refused before any launch: a null pointer, n < 4 or n % 4 != 0, capacity < 1 (MLIIS_ERR_ARG); grad, theta, ws or ring not 16-byte
 * aligned, loss4, lr_dev or cursor not 4-byte aligned (MLIIS_ERR_ALIGN). */
int mliis_steplog_append(const float* loss4, const float* lr_dev, const float* grad, const float* theta, long long n, void* ws, void* ring,
                         int capacity, unsigned* cursor, hipStream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
