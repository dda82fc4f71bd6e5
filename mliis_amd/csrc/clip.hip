// libmliis_clip.so: the inner loop's gradient clipping (include/mliis_clip.h).  A library of its own beside libmliis_hip.so,
// libmliis_score.so, libmliis_data.so, libmliis_steplog.so and libmliis_layerlog.so -- the training step's library, the logs' and their C
// ABIs are untouched by it.  Two launches between the backward pass and the optimizer launch reduce the packed gradient arena (and, per
// tensor, the parameter arena), form the scale(s) and multiply the gradient in place; the ring position is a device counter the first
// launch advances, so the launches replay inside the step's captured graph.
#include <float.h>
#include <math.h>

#include "../../include/mliis_clip.h"
#include "arena_reduce.hpp"

namespace mliis {

// (this library's own error slot: common.hpp's MLIIS_REQUIRE / MLIIS_CHECK_LAUNCH report through set_error of the library they are linked into)
MLIIS_DEFINE_ERROR_SLOT(g_clip_err)

// One workgroup of kClipThreads threads per chunk in both launches: thread t handles quads t, t + 256, ... of the chunk (consecutive lanes,
// consecutive 16 bytes), so what a thread sums and in which order depends on the chunk table alone.  A chunk is at most kClipChunkQuads
// quads (64 KB of the arena: 16 quads a thread); a tensor shorter than that is one chunk whose loop ends with it.
constexpr int kClipThreads = 256, kClipWaves = kClipThreads / kWave;
constexpr int kClipChunkQuads = 4096;
constexpr int kRecordWords = 8;
constexpr int kClipDepth = 4;   // quads of each arena a thread has in flight
constexpr unsigned kFlagClipped = 1u, kFlagBypassed = 2u;

struct ClipPartial {   // one chunk, 32 bytes
  double gss;               // sum of squares of the finite counted gradient elements
  double tss;               // the same for the parameters (MLIIS_CLIP_RATIO; 0 otherwise)
  unsigned long long nf;    // non-finite counted gradient elements
  unsigned long long pad;
};
static_assert(sizeof(ClipPartial) == 32, "partial layout");
// workspace: [0, 16) the ring row of the call (one word used), then one partial per chunk
constexpr size_t kClipPartialsAt = 16;

struct Sum {
  double gss, tss;
  unsigned long long nf;
};

// element `idx` of the chunk (idx < valid: inside the tensor's count, not its padding)
__device__ __forceinline__ void grad_elem(float v, unsigned idx, unsigned valid, double& ss, unsigned& nf) {
  if (idx >= valid) return;
  if (finite_f(v)) {
    const double d = (double)v;   // (squared in double: 1e30^2 is past fp32)
    ss = fma(d, d, ss);
  } else {
    ++nf;
  }
}

__device__ __forceinline__ void theta_elem(float v, unsigned idx, unsigned valid, double& ss) {
  if (idx < valid && finite_f(v)) {
    const double d = (double)v;
    ss = fma(d, d, ss);
  }
}

template <int MODE>
__device__ __forceinline__ void sum_quad(float4 g, float4 w, unsigned idx, unsigned valid, double& gss, double& tss, unsigned& nf) {
  grad_elem(g.x, idx, valid, gss, nf);
  grad_elem(g.y, idx + 1u, valid, gss, nf);
  grad_elem(g.z, idx + 2u, valid, gss, nf);
  grad_elem(g.w, idx + 3u, valid, gss, nf);
  if (MODE == MLIIS_CLIP_RATIO) {
    theta_elem(w.x, idx, valid, tss);
    theta_elem(w.y, idx + 1u, valid, tss);
    theta_elem(w.z, idx + 2u, valid, tss);
    theta_elem(w.w, idx + 3u, valid, tss);
  }
}

// A workgroup's fold of one Sum per thread: a fixed butterfly inside each wave, then the waves in index order; every thread returns the
// same bits.  (Called by all threads of the workgroup; the barrier at its end lets s_wave be used again.)
__device__ __forceinline__ Sum block_fold(Sum s, Sum* s_wave) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s.gss += __shfl_xor(s.gss, o, kWave);
    s.tss += __shfl_xor(s.tss, o, kWave);
    s.nf += __shfl_xor(s.nf, o, kWave);
  }
  if (lane == 0) s_wave[wave] = s;
  __syncthreads();
  Sum r = s_wave[0];
#pragma unroll
  for (int w = 1; w < kClipWaves; ++w) {
    r.gss += s_wave[w].gss;
    r.tss += s_wave[w].tss;
    r.nf += s_wave[w].nf;
  }
  __syncthreads();
  return r;
}

// ---- launch 1: one partial per chunk; the first workgroup moves the ring position
template <int MODE>
__global__ __launch_bounds__(kClipThreads) void clip_partial_k(const float* __restrict__ ga, const float* __restrict__ ta,
                                                               const int4* __restrict__ chunks, ClipPartial* __restrict__ part,
                                                               unsigned* __restrict__ row, unsigned capacity, unsigned* __restrict__ cursor) {
  __shared__ Sum s_wave[kClipWaves];
  const int tid = threadIdx.x;
  const int4 ch = chunks[blockIdx.x];                       // {tensor, first quad, quads, valid elements}
  const float* g = ga + (long long)ch.y * 4;
  const float* w = ta + (long long)ch.y * 4;                // (never dereferenced in MLIIS_CLIP_NORM)
  const int quads = ch.z;
  const unsigned valid = (unsigned)ch.w;

  if (blockIdx.x == 0 && tid == 0) {
    const unsigned c = *cursor;   // (written by the call before this one on the stream)
    *row = c % capacity;
    *cursor = c + 1u;
  }

  double gss = 0.0, tss = 0.0;
  unsigned nf = 0u;   // (a thread sees at most 64 elements of a chunk)
  stream_quads<kClipDepth, MODE == MLIIS_CLIP_RATIO ? 2 : 1, kClipThreads>(
      g, w, tid, quads, [&](int i, float4 a, float4 b) { sum_quad<MODE>(a, b, (unsigned)i * 4u, valid, gss, tss, nf); });

  Sum s;
  s.gss = gss;
  s.tss = tss;
  s.nf = nf;
  s = block_fold(s, s_wave);
  if (tid == 0) {
    ClipPartial p;
    p.gss = s.gss;
    p.tss = s.tss;
    p.nf = s.nf;
    p.pad = 0ull;
    part[blockIdx.x] = p;
  }
}

// The fold of the partials [c0, c1) by one workgroup: thread t adds partials c0 + t, c0 + t + 256, ... in that order, then block_fold.  The
// order is a function of (c0, c1) alone, so every workgroup that folds the same range arrives at the same bits.
__device__ __forceinline__ Sum fold_partials(const ClipPartial* __restrict__ part, int c0, int c1, Sum* s_wave) {
  Sum s;
  s.gss = 0.0;
  s.tss = 0.0;
  s.nf = 0ull;
  for (int c = c0 + (int)threadIdx.x; c < c1; c += kClipThreads) {
    const ClipPartial p = part[c];
    s.gss += p.gss;
    s.tss += p.tss;
    s.nf += p.nf;
  }
  return block_fold(s, s_wave);
}

// one fp32 multiplication per element (__fmul_rn is never contracted into a fused multiply-add)
__device__ __forceinline__ float4 scaled(float4 v, float s) {
  return make_float4(__fmul_rn(v.x, s), __fmul_rn(v.y, s), __fmul_rn(v.z, s), __fmul_rn(v.w, s));
}

// ---- launch 2: every workgroup folds the partials of its scale, multiplies its chunk in place; a record's first chunk writes the record
template <int MODE>
__global__ __launch_bounds__(kClipThreads) void clip_scale_k(float* __restrict__ ga, const int4* __restrict__ chunks,
                                                             const int4* __restrict__ segs, int nchunks, int T,
                                                             const ClipPartial* __restrict__ part, const unsigned* __restrict__ row,
                                                             float threshold, float eps, uint4* __restrict__ ring) {
  __shared__ Sum s_wave[kClipWaves];
  const int tid = threadIdx.x;
  const int4 ch = chunks[blockIdx.x];                       // {tensor, first quad, quads, valid elements}
  const int4 seg = segs[ch.x];                              // {first quad, element count, first chunk, one past the last chunk}
  const Sum all = fold_partials(part, 0, nchunks, s_wave);  // (the same bits in every workgroup)
  Sum mine = all;
  if (MODE == MLIIS_CLIP_RATIO) mine = fold_partials(part, seg.z, seg.w, s_wave);   // (the same bits in every workgroup of the tensor)

  const bool bypassed = all.nf != 0ull;   // a non-finite element anywhere: nothing is touched
  const double norm = sqrt(mine.gss);
  const double ref = MODE == MLIIS_CLIP_RATIO ? (double)threshold * fmax(sqrt(mine.tss), (double)eps) : (double)threshold;
  const bool clipped = !bypassed && norm > ref;
  float s = 1.f;
  if (clipped) s = fmaxf((float)(ref / norm), FLT_MIN);   // formed in double, rounded once; in (0, 1]

  const bool writes = MODE == MLIIS_CLIP_RATIO ? blockIdx.x == (unsigned)seg.z : blockIdx.x == 0u;
  if (writes && tid == 0) {
    const int R = MODE == MLIIS_CLIP_RATIO ? T : 1, r = MODE == MLIIS_CLIP_RATIO ? ch.x : 0;
    uint4* rec = ring + ((size_t)(*row) * (size_t)R + (size_t)r) * 2;
    rec[0] = make_uint4(__float_as_uint((float)norm), __float_as_uint((float)ref), __float_as_uint(s), sat_u32(mine.nf));
    rec[1] = make_uint4((clipped ? kFlagClipped : 0u) | (bypassed ? kFlagBypassed : 0u), 0u, 0u, 0u);
  }
  if (s == 1.f) return;   // (uniform) not clipped, bypassed, or a scale that rounds to 1: the chunk stays bit for bit

  float* g = ga + (long long)ch.y * 4;
  const int quads = ch.z;
  int i = tid;
  for (; i + (kClipDepth - 1) * kClipThreads < quads; i += kClipDepth * kClipThreads) {
    float4 a[kClipDepth];
#pragma unroll
    for (int u = 0; u < kClipDepth; ++u) a[u] = ld4(g + (i + u * kClipThreads) * 4);
#pragma unroll
    for (int u = 0; u < kClipDepth; ++u) st4(g + (i + u * kClipThreads) * 4, scaled(a[u], s));
  }
  for (; i < quads; i += kClipThreads) st4(g + i * 4, scaled(ld4(g + i * 4), s));
}

}  // namespace mliis

using namespace mliis;

extern "C" {

const char* mliis_clip_last_error(void) { return g_clip_err; }

int mliis_clip_chunk_quads(void) { return kClipChunkQuads; }

size_t mliis_clip_workspace_bytes(int nchunks, int T) {
  return (nchunks < 1 || T < 1) ? 0 : kClipPartialsAt + (size_t)nchunks * sizeof(ClipPartial);
}

int mliis_clip_record_words(void) { return kRecordWords; }

// include/mliis_clip.h.  Two launches in both modes.
int mliis_clip_apply(int mode, float* g, const float* theta, long long n, const int* chunks, int nchunks, const int* segs, int T,
                     float threshold, float eps, void* ws, size_t ws_bytes, void* ring, int capacity, unsigned* cursor,
                     hipStream_t stream) {
  MLIIS_REQUIRE(mode == MLIIS_CLIP_NORM || mode == MLIIS_CLIP_RATIO, MLIIS_ERR_ARG, "clip_apply: mode = %d (0 norm, 1 ratio)", mode);
  MLIIS_REQUIRE(g && chunks && segs && ws && ring && cursor && (theta || mode == MLIIS_CLIP_NORM), MLIIS_ERR_ARG, "clip_apply: null pointer");
  if (int e = check_chunk_sizes("clip_apply", n, nchunks, T, capacity)) return e;
  MLIIS_REQUIRE(isfinite(threshold) && threshold > 0.f, MLIIS_ERR_ARG, "clip_apply: threshold = %g (finite and positive)", (double)threshold);
  MLIIS_REQUIRE(mode == MLIIS_CLIP_NORM || (isfinite(eps) && eps > 0.f), MLIIS_ERR_ARG, "clip_apply: eps = %g (finite and positive)", (double)eps);
  if (int e = check_chunk_buffers("clip_apply", "g, theta", g, theta, chunks, segs, ws, ws_bytes, mliis_clip_workspace_bytes(nchunks, T), ring, cursor))
    return e;
  const int4* ch = reinterpret_cast<const int4*>(chunks);
  const int4* sg = reinterpret_cast<const int4*>(segs);
  unsigned char* w = reinterpret_cast<unsigned char*>(ws);
  unsigned* row = reinterpret_cast<unsigned*>(w);
  ClipPartial* part = reinterpret_cast<ClipPartial*>(w + kClipPartialsAt);
  uint4* rg = reinterpret_cast<uint4*>(ring);
  if (mode == MLIIS_CLIP_NORM) {
    hipLaunchKernelGGL(clip_partial_k<MLIIS_CLIP_NORM>, dim3(nchunks), dim3(kClipThreads), 0, stream, g, theta, ch, part, row,
                       (unsigned)capacity, cursor);
    MLIIS_CHECK_LAUNCH("clip_apply (partials)");
    hipLaunchKernelGGL(clip_scale_k<MLIIS_CLIP_NORM>, dim3(nchunks), dim3(kClipThreads), 0, stream, g, ch, sg, nchunks, T, part, row,
                       threshold, eps, rg);
  } else {
    hipLaunchKernelGGL(clip_partial_k<MLIIS_CLIP_RATIO>, dim3(nchunks), dim3(kClipThreads), 0, stream, g, theta, ch, part, row,
                       (unsigned)capacity, cursor);
    MLIIS_CHECK_LAUNCH("clip_apply (partials)");
    hipLaunchKernelGGL(clip_scale_k<MLIIS_CLIP_RATIO>, dim3(nchunks), dim3(kClipThreads), 0, stream, g, ch, sg, nchunks, T, part, row,
                       threshold, eps, rg);
  }
  MLIIS_CHECK_LAUNCH("clip_apply (scale)");
  return MLIIS_OK;
}
}
