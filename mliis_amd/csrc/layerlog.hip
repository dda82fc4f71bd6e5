// libmliis_layerlog.so: the inner loop's per-tensor log (include/mliis_layerlog.h).  A library of its own beside libmliis_hip.so,
// libmliis_score.so, libmliis_data.so and libmliis_steplog.so -- the training step's library, the step log's and their C ABIs are untouched
// by it.  Two launches at the tail of a step reduce the packed gradient and parameter arenas per tensor and write one record per tensor
// into the ring row the step log's device cursor names; the cursor is only read here, so the launches replay inside the step's graph.
#include "../../include/mliis_layerlog.h"
#include "arena_reduce.hpp"

namespace mliis {

// (this library's own error slot: common.hpp's MLIIS_REQUIRE / MLIIS_CHECK_LAUNCH report through set_error of the library they are linked into)
MLIIS_DEFINE_ERROR_SLOT(g_layerlog_err)

// One workgroup of kLayerThreads threads per chunk: thread t reads quads t, t + 256, ... of the chunk from both arenas (consecutive lanes
// read consecutive 16 bytes), so what a thread sums and in which order depends on the chunk table alone.  A chunk is at most
// kLayerChunkQuads quads (64 KB of each arena: 16 quads a thread); a tensor shorter than that is one chunk whose loop ends with it.
constexpr int kLayerThreads = 256, kLayerWaves = kLayerThreads / kWave;
constexpr int kLayerChunkQuads = 4096;
constexpr int kRecordWords = 8;
constexpr int kLayerDepth = 4;   // quads of each arena a thread has in flight
constexpr unsigned kNone = 0xffffffffu;

struct Stat {   // one arena's share of a chunk or of a tensor
  double ss;            // sum of squares of the finite elements
  float amax;           // their largest magnitude
  unsigned first;       // lowest index within the tensor of a non-finite element, kNone
  unsigned long long nf;   // non-finite elements
};
struct LayerPartial {   // one chunk, 48 bytes
  Stat x, y;
};
static_assert(sizeof(Stat) == 24 && sizeof(LayerPartial) == 48, "partial layout");

__device__ __forceinline__ Stat stat_zero() {
  Stat s;
  s.ss = 0.0;
  s.amax = 0.f;
  s.first = kNone;
  s.nf = 0ull;
  return s;
}

// element `idx` of the tensor (idx < limit: inside the tensor's count, not its padding)
__device__ __forceinline__ void stat_elem(float v, unsigned idx, unsigned limit, Stat& s) {
  if (idx >= limit) return;
  if (finite_f(v)) {
    const double d = (double)v;   // (squared in double: 1e30^2 is past fp32)
    s.ss = fma(d, d, s.ss);
    s.amax = fmaxf(s.amax, fabsf(v));
  } else {
    ++s.nf;
    s.first = min(s.first, idx);
  }
}

__device__ __forceinline__ void stat_quad(float4 v, unsigned idx, unsigned limit, Stat& s) {
  stat_elem(v.x, idx, limit, s);
  stat_elem(v.y, idx + 1u, limit, s);
  stat_elem(v.z, idx + 2u, limit, s);
  stat_elem(v.w, idx + 3u, limit, s);
}

// b folded into a (a's elements come first)
__device__ __forceinline__ void stat_fold(Stat& a, const Stat& b) {
  a.ss += b.ss;
  a.amax = fmaxf(a.amax, b.amax);
  a.first = min(a.first, b.first);
  a.nf += b.nf;
}

__device__ __forceinline__ Stat stat_shfl_xor(const Stat& s, int o) {
  Stat r;
  r.ss = __shfl_xor(s.ss, o, kWave);
  r.amax = __shfl_xor(s.amax, o, kWave);
  r.first = __shfl_xor(s.first, o, kWave);
  r.nf = __shfl_xor(s.nf, o, kWave);
  return r;
}

__device__ __forceinline__ Stat stat_shfl(const Stat& s, int src) {
  Stat r;
  r.ss = __shfl(s.ss, src, kWave);
  r.amax = __shfl(s.amax, src, kWave);
  r.first = __shfl(s.first, src, kWave);
  r.nf = __shfl(s.nf, src, kWave);
  return r;
}

// MLIIS_LAYERLOG_DELTA: X is one fp32 subtraction per element (no other rounding: __fsub_rn is never contracted)
template <int MODE>
__device__ __forceinline__ float4 x_of(float4 a, float4 b) {
  if (MODE == MLIIS_LAYERLOG_STEP) return a;
  return make_float4(__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y), __fsub_rn(a.z, b.z), __fsub_rn(a.w, b.w));
}

// ---- launch 1: one partial per chunk
template <int MODE>
__global__ __launch_bounds__(kLayerThreads) void layerlog_partial_k(const float* __restrict__ xa, const float* __restrict__ ya,
                                                                    const int4* __restrict__ chunks, const int4* __restrict__ segs,
                                                                    LayerPartial* __restrict__ part) {
  __shared__ LayerPartial s_part[kLayerWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int4 ch = chunks[blockIdx.x];                       // {tensor, first quad, quads, valid elements}
  const float* x = xa + (long long)ch.y * 4;
  const float* y = ya + (long long)ch.y * 4;
  const int quads = ch.z;
  const unsigned base = (unsigned)(ch.y - segs[ch.x].x) * 4u;   // the chunk's first element within its tensor
  const unsigned limit = base + (unsigned)ch.w;

  Stat sx = stat_zero(), sy = stat_zero();
  stream_quads<kLayerDepth, 2, kLayerThreads>(x, y, tid, quads, [&](int i, float4 a, float4 b) {
    const unsigned idx = base + (unsigned)i * 4u;
    stat_quad(x_of<MODE>(a, b), idx, limit, sx);
    stat_quad(b, idx, limit, sy);
  });

  // workgroup fold: a fixed butterfly inside each wave, then the waves in index order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const Stat ox = stat_shfl_xor(sx, o), oy = stat_shfl_xor(sy, o);
    stat_fold(sx, ox);
    stat_fold(sy, oy);
  }
  if (lane == 0) {
    s_part[wave].x = sx;
    s_part[wave].y = sy;
  }
  __syncthreads();
  if (tid == 0) {
    LayerPartial p = s_part[0];
    for (int w = 1; w < kLayerWaves; ++w) {
      stat_fold(p.x, s_part[w].x);
      stat_fold(p.y, s_part[w].y);
    }
    part[blockIdx.x] = p;
  }
}

// ---- launch 2: one tensor per wave folds its chunks' partials in chunk order and writes its record
__global__ __launch_bounds__(kLayerThreads) void layerlog_fold_k(const LayerPartial* __restrict__ part, const int4* __restrict__ segs, int T,
                                                                 uint4* __restrict__ ring, unsigned capacity,
                                                                 const unsigned* __restrict__ cursor, unsigned row_offset) {
  const int lane = threadIdx.x & (kWave - 1);
  const int t = blockIdx.x * kLayerWaves + threadIdx.x / kWave;
  if (t >= T) return;   // (wave-uniform; no barrier below)
  const int4 seg = segs[t];                                 // {first quad, element count, first chunk, one past the last chunk}
  Stat ax = stat_zero(), ay = stat_zero();
  for (int c0 = seg.z; c0 < seg.w; c0 += kWave) {
    const int m = min(kWave, seg.w - c0);
    // the loads of up to 64 partials are in flight at once; they are then added one by one, chunk c0 first, in every lane alike
    Stat px = stat_zero(), py = stat_zero();
    if (lane < m) {
      const LayerPartial p = part[c0 + lane];
      px = p.x;
      py = p.y;
    }
    for (int j = 0; j < m; ++j) {
      const Stat bx = stat_shfl(px, j), by = stat_shfl(py, j);
      stat_fold(ax, bx);
      stat_fold(ay, by);
    }
  }
  if (lane == 0) {
    const unsigned c = (cursor ? *cursor : 0u) + row_offset;   // (modulo 2^32 like the step log's counter)
    uint4* rec = ring + ((size_t)(c % capacity) * (size_t)T + (size_t)t) * 2;
    rec[0] = make_uint4(__float_as_uint((float)sqrt(ax.ss)), __float_as_uint(ax.amax), __float_as_uint((float)sqrt(ay.ss)),
                        __float_as_uint(ay.amax));
    rec[1] = make_uint4(sat_u32(ax.nf), sat_u32(ay.nf), ax.first, ay.first);
  }
}

}  // namespace mliis

using namespace mliis;

extern "C" {

const char* mliis_layerlog_last_error(void) { return g_layerlog_err; }

int mliis_layerlog_chunk_quads(void) { return kLayerChunkQuads; }

size_t mliis_layerlog_workspace_bytes(int nchunks) { return nchunks < 1 ? 0 : (size_t)nchunks * sizeof(LayerPartial); }

int mliis_layerlog_record_words(void) { return kRecordWords; }

// include/mliis_layerlog.h.  Two launches.
int mliis_layerlog_append(int mode, const float* x, const float* y, long long n, const int* chunks, int nchunks, const int* segs, int T,
                          void* ws, size_t ws_bytes, void* ring, int capacity, const unsigned* cursor, unsigned row_offset,
                          hipStream_t stream) {
  MLIIS_REQUIRE(x && y && chunks && segs && ws && ring, MLIIS_ERR_ARG, "layerlog_append: null pointer");
  MLIIS_REQUIRE(mode == MLIIS_LAYERLOG_STEP || mode == MLIIS_LAYERLOG_DELTA, MLIIS_ERR_ARG, "layerlog_append: mode = %d (0 step, 1 delta)", mode);
  if (int e = check_chunk_sizes("layerlog_append", n, nchunks, T, capacity)) return e;
  if (int e = check_chunk_buffers("layerlog_append", "x, y", x, y, chunks, segs, ws, ws_bytes, mliis_layerlog_workspace_bytes(nchunks), ring, cursor))
    return e;
  const int4* ch = reinterpret_cast<const int4*>(chunks);
  const int4* sg = reinterpret_cast<const int4*>(segs);
  LayerPartial* part = reinterpret_cast<LayerPartial*>(ws);
  if (mode == MLIIS_LAYERLOG_STEP)
    hipLaunchKernelGGL(layerlog_partial_k<MLIIS_LAYERLOG_STEP>, dim3(nchunks), dim3(kLayerThreads), 0, stream, x, y, ch, sg, part);
  else
    hipLaunchKernelGGL(layerlog_partial_k<MLIIS_LAYERLOG_DELTA>, dim3(nchunks), dim3(kLayerThreads), 0, stream, x, y, ch, sg, part);
  MLIIS_CHECK_LAUNCH("layerlog_append (partials)");
  hipLaunchKernelGGL(layerlog_fold_k, dim3(ceil_div(T, kLayerWaves)), dim3(kLayerThreads), 0, stream, part, sg, T,
                     reinterpret_cast<uint4*>(ring), (unsigned)capacity, cursor, row_offset);
  MLIIS_CHECK_LAUNCH("layerlog_append (fold)");
  return MLIIS_OK;
}
}
