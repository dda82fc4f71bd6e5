// What the inner loop's arena reductions share: steplog.hip, layerlog.hip and clip.hip stream the packed gradient / parameter arenas
// through the same loop and check the same chunk-table arguments.  Each keeps its own workgroup fold: the record types differ and the order
// of a fold's additions is that file's determinism contract.
#pragma once
#include "common.hpp"

namespace mliis {

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ unsigned sat_u32(unsigned long long v) { return v > 0xffffffffull ? 0xffffffffu : (unsigned)v; }

// A thread's quads first, first + STRIDE, ... below nquads of one arena (ARENAS == 1: y is never dereferenced, b is zero) or of two, handed
// to use(i, a, b) -- i the quad's index, a / b its 16 bytes of x / y.  These launches have few waves per SIMD, so a thread that waits for
// each 16-byte load before it asks for the next one is bound by memory latency: DEPTH quads of each arena are requested before the first
// of them is used.  The order in which a thread consumes its elements -- and with it every sum -- is the order of the plain loop, then
// the tail one quad at a time.  I: the index type (int inside a chunk, long long over a whole arena).
template <int DEPTH, int ARENAS, int STRIDE, typename I, typename F>
__device__ __forceinline__ void stream_quads(const float* __restrict__ x, const float* __restrict__ y, I first, I nquads, F use) {
  static_assert(ARENAS == 1 || ARENAS == 2, "one arena or two");
  I i = first;
  for (; i + (DEPTH - 1) * STRIDE < nquads; i += DEPTH * STRIDE) {
    float4 a[DEPTH], b[DEPTH];
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) a[u] = ld4(x + (i + u * STRIDE) * 4);
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) b[u] = ARENAS == 2 ? ld4(y + (i + u * STRIDE) * 4) : f4zero();
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) use(i + u * STRIDE, a[u], b[u]);
  }
  for (; i < nquads; i += STRIDE) {
    const float4 a = ld4(x + i * 4), b = ARENAS == 2 ? ld4(y + i * 4) : f4zero();
    use(i, a, b);
  }
}

// The argument checks mliis_layerlog_append and mliis_clip_apply share, in two runs because clip's threshold and eps checks stand
// between them: the sizes of the chunk tables, then the workspace (`need` bytes) and the alignment of what the kernels address.  `who`
// begins every message; `arenas` names the two arenas in the alignment message; MLIIS_OK or the set_error code.
static inline int check_chunk_sizes(const char* who, long long n, int nchunks, int T, int capacity) {
  MLIIS_REQUIRE(n > 0 && (n & 3) == 0, MLIIS_ERR_ARG, "%s: n must be a positive multiple of 4 (arena is padded)", who);
  MLIIS_REQUIRE(n / 4 <= 0x7fffffffll, MLIIS_ERR_ARG, "%s: n = %lld (the tables address quads with 32 bits)", who, n);
  MLIIS_REQUIRE(T >= 1, MLIIS_ERR_ARG, "%s: T = %d (at least one tensor)", who, T);
  MLIIS_REQUIRE(nchunks >= T && (long long)nchunks <= n / 4, MLIIS_ERR_ARG,
                "%s: nchunks = %d (every one of the %d tensors has a chunk, every chunk a quad of the %lld)", who, nchunks, T, n / 4);
  MLIIS_REQUIRE(capacity >= 1, MLIIS_ERR_ARG, "%s: capacity = %d (the ring holds at least one row)", who, capacity);
  return MLIIS_OK;
}

static inline int check_chunk_buffers(const char* who, const char* arenas, const void* a, const void* b, const void* chunks, const void* segs,
                                      const void* ws, size_t ws_bytes, size_t need, const void* ring, const void* cursor) {
  MLIIS_REQUIRE(ws_bytes >= need, MLIIS_ERR_ARG, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
  MLIIS_REQUIRE(aligned16(a) && aligned16(b) && aligned16(chunks) && aligned16(segs) && aligned16(ws) && aligned16(ring), MLIIS_ERR_ALIGN,
                "%s: %s, chunks, segs, ws and ring must be 16-byte aligned", who, arenas);
  MLIIS_REQUIRE((reinterpret_cast<uintptr_t>(cursor) & 3u) == 0, MLIIS_ERR_ALIGN, "%s: cursor must be 4-byte aligned", who);
  return MLIIS_OK;
}

}  // namespace mliis
