// libmliis_steplog.so: the inner loop's step log (include/mliis_steplog.h).  A library of its own beside libmliis_hip.so, libmliis_score.so
// and libmliis_data.so -- the training step's library and its C ABI (include/mliis_hip.h) are untouched by it.  One launch at the tail of a
// step reduces the packed gradient and parameter arenas and appends one record to a ring in device memory; the ring position is a device
// counter, so the launch replays inside the step's captured graph.
#include "../../include/mliis_steplog.h"
#include "arena_reduce.hpp"

namespace mliis {

// (this library's own error slot: common.hpp's MLIIS_REQUIRE / MLIIS_CHECK_LAUNCH report through set_error of the library they are linked into)
MLIIS_DEFINE_ERROR_SLOT(g_steplog_err)

// The grid is a constant: kLogBlocks workgroups of kLogThreads threads, thread t of the grid reads quads t, t + 65536, t + 2 * 65536, ...
// of both arenas (consecutive lanes read consecutive 16 bytes), so what a thread sums and in which order depends on n alone.
constexpr int kLogBlocks = 256, kLogThreads = 256, kLogWaves = kLogThreads / kWave;
constexpr int kRecordWords = 8;
constexpr int kLogDepth = 4;   // quads of each arena a thread has in flight

struct LogPartial {   // one workgroup's share, 32 bytes
  double ss;                       // sum of squares of its finite gradient elements
  float amax;                      // their largest magnitude
  unsigned pad;
  unsigned long long gnf, tnf;     // non-finite elements of grad / theta
};
// workspace: [0, 16) the arrival counter (one word used), then kLogBlocks partials
constexpr size_t kLogPartialsAt = 16;
constexpr size_t kLogWorkspaceBytes = kLogPartialsAt + (size_t)kLogBlocks * sizeof(LogPartial);

__device__ __forceinline__ void grad_elem(float v, double& ss, float& amax, unsigned& nf) {
  if (finite_f(v)) {
    const double d = (double)v;   // (squared in double: 1e30^2 is past fp32)
    ss = fma(d, d, ss);
    amax = fmaxf(amax, fabsf(v));
  } else {
    ++nf;
  }
}

__device__ __forceinline__ unsigned nonfinite4(float4 w) {
  return (finite_f(w.x) ? 0u : 1u) + (finite_f(w.y) ? 0u : 1u) + (finite_f(w.z) ? 0u : 1u) + (finite_f(w.w) ? 0u : 1u);
}

__global__ __launch_bounds__(kLogThreads) void steplog_append_k(const unsigned* __restrict__ loss4, const unsigned* __restrict__ lr_dev,
                                                                const float* __restrict__ grad, const float* __restrict__ theta,
                                                                long long nquads, unsigned* __restrict__ ticket, LogPartial* __restrict__ part,
                                                                uint4* __restrict__ ring, unsigned capacity, unsigned* __restrict__ cursor) {
  __shared__ double s_ss[kLogThreads];
  __shared__ float s_amax[kLogThreads];
  __shared__ unsigned long long s_gnf[kLogThreads], s_tnf[kLogThreads];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const long long first = (long long)blockIdx.x * kLogThreads + tid;

  double ss = 0.0;
  float amax = 0.f;
  unsigned gnf = 0u, tnf = 0u;   // (a thread sees n / 65536 elements: 32 bits hold them for any n the arenas can have)
  // (the launch has one wave per SIMD: kLogDepth quads of each arena in flight, consumed in the order of the plain loop)
  stream_quads<kLogDepth, 2, kLogBlocks * kLogThreads>(grad, theta, first, nquads, [&](long long, float4 g, float4 w) {
    grad_elem(g.x, ss, amax, gnf);
    grad_elem(g.y, ss, amax, gnf);
    grad_elem(g.z, ss, amax, gnf);
    grad_elem(g.w, ss, amax, gnf);
    tnf += nonfinite4(w);
  });

  // workgroup fold: a fixed butterfly inside each wave, then the waves in index order
  unsigned long long gn = gnf, tn = tnf;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ss += __shfl_xor(ss, o, kWave);
    amax = fmaxf(amax, __shfl_xor(amax, o, kWave));
    gn += __shfl_xor(gn, o, kWave);
    tn += __shfl_xor(tn, o, kWave);
  }
  if (lane == 0) {
    s_ss[wave] = ss;
    s_amax[wave] = amax;
    s_gnf[wave] = gn;
    s_tnf[wave] = tn;
  }
  __syncthreads();
  if (tid == 0) {
    LogPartial p;
    p.ss = s_ss[0];
    p.amax = s_amax[0];
    p.pad = 0u;
    p.gnf = s_gnf[0];
    p.tnf = s_tnf[0];
    for (int w = 1; w < kLogWaves; ++w) {
      p.ss += s_ss[w];
      p.amax = fmaxf(p.amax, s_amax[w]);
      p.gnf += s_gnf[w];
      p.tnf += s_tnf[w];
    }
    part[blockIdx.x] = p;
    // publish the partial to the other workgroups before the ticket is drawn: drain this lane's stores, agent-scope release, drain
    // again (the fence's own wait is not relied on), then a relaxed agent-scope add -- the arrival order decides only WHO folds
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned tk = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = tk == (unsigned)kLogBlocks - 1u;
  }
  __syncthreads();
  if (!s_last) return;   // (uniform)

  // the last workgroup to arrive: acquire once (this CU's L1 may hold stale lines of the partials), then plain loads
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  {
    const LogPartial p = part[tid];   // (kLogThreads == kLogBlocks)
    s_ss[tid] = p.ss;
    s_amax[tid] = p.amax;
    s_gnf[tid] = p.gnf;
    s_tnf[tid] = p.tnf;
  }
  __syncthreads();
  if (tid == 0) {
    double tss = 0.0;
    float tmax = 0.f;
    unsigned long long tg = 0ull, tt = 0ull;
    // index order, whichever workgroup does it (unrolled so that the LDS reads of 16 partials are in flight at once: one thread
    // that waits for each read spends more time here than the whole grid spends on the arenas)
#pragma unroll 16
    for (int b = 0; b < kLogBlocks; ++b) {
      tss += s_ss[b];
      tmax = fmaxf(tmax, s_amax[b]);
      tg += s_gnf[b];
      tt += s_tnf[b];
    }
    const unsigned c = *cursor;   // (written by the launch before this one on the stream)
    ring[(size_t)(c % capacity) * 2] = make_uint4(loss4[0], loss4[1], loss4[2], lr_dev[0]);
    ring[(size_t)(c % capacity) * 2 + 1] = make_uint4(__float_as_uint((float)sqrt(tss)), __float_as_uint(tmax), sat_u32(tg), sat_u32(tt));
    *cursor = c + 1u;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next launch
  }
}

static_assert(kLogThreads == kLogBlocks, "the fold loads one partial per thread");
static_assert(sizeof(LogPartial) == 32, "partial layout");

}  // namespace mliis

using namespace mliis;

extern "C" {

const char* mliis_steplog_last_error(void) { return g_steplog_err; }

size_t mliis_steplog_workspace_bytes(void) { return kLogWorkspaceBytes; }

int mliis_steplog_record_words(void) { return kRecordWords; }

// include/mliis_steplog.h.  One launch.
int mliis_steplog_append(const float* loss4, const float* lr_dev, const float* grad, const float* theta, long long n, void* ws, void* ring,
                         int capacity, unsigned* cursor, hipStream_t stream) {
  MLIIS_REQUIRE(loss4 && lr_dev && grad && theta && ws && ring && cursor, MLIIS_ERR_ARG, "steplog_append: null pointer");
  MLIIS_REQUIRE(n > 0 && (n & 3) == 0, MLIIS_ERR_ARG, "steplog_append: n must be a positive multiple of 4 (arena is padded)");
  MLIIS_REQUIRE(capacity >= 1, MLIIS_ERR_ARG, "steplog_append: capacity = %d (the ring holds at least one record)", capacity);
  MLIIS_REQUIRE(aligned16(grad) && aligned16(theta) && aligned16(ws) && aligned16(ring), MLIIS_ERR_ALIGN,
                "steplog_append: grad, theta, ws and ring must be 16-byte aligned");
  MLIIS_REQUIRE(((reinterpret_cast<uintptr_t>(loss4) | reinterpret_cast<uintptr_t>(lr_dev) | reinterpret_cast<uintptr_t>(cursor)) & 3u) == 0,
                MLIIS_ERR_ALIGN, "steplog_append: loss4, lr_dev and cursor must be 4-byte aligned");
  unsigned char* w = reinterpret_cast<unsigned char*>(ws);
  hipLaunchKernelGGL(steplog_append_k, dim3(kLogBlocks), dim3(kLogThreads), 0, stream, reinterpret_cast<const unsigned*>(loss4),
                     reinterpret_cast<const unsigned*>(lr_dev), grad, theta, n / 4, reinterpret_cast<unsigned*>(w),
                     reinterpret_cast<LogPartial*>(w + kLogPartialsAt), reinterpret_cast<uint4*>(ring), (unsigned)capacity, cursor);
  MLIIS_CHECK_LAUNCH("steplog_append");
  return MLIIS_OK;
}
}
