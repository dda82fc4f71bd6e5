// libmliis_tta.so: flip test-time augmentation at evaluation -- the mirrored copy of an input batch and the merge of the views'
// decoder-resolution logits (include/mliis_tta.h).  A library of its own beside libmliis_hip.so, libmliis_score.so and libmliis_sweep.so,
// none of which (nor their headers) is touched by it: the merged logits replace the plan's decoder-resolution logits before the existing
// scoring kernels read them.
#include "../../include/mliis_tta.h"
#include "common.hpp"

namespace mliis {

// (this library's own error slot: common.hpp's MLIIS_REQUIRE / MLIIS_CHECK_LAUNCH report through set_error of the library they are linked into)
MLIIS_DEFINE_ERROR_SLOT(g_tta_err)

// Both kernels are memory-bound elementwise passes over rows of L = W C words (an image row, all channels).  The row-quad form gives a
// thread four consecutive words of a destination row (one 16-byte store; L is a multiple of 4 and the base 16-byte aligned, so every row
// start is); the word form one word.  A mirrored row reverses the PIXELS, not the words (the channels of a pixel keep their order), so
// the source of a quad is four single-word loads there -- of one wave they fall into the same cache lines as a 16-byte load's would, in
// reverse order -- and a 16-byte load when the columns are not mirrored.

// the word of row `s` that destination word e of a row reads
__device__ __forceinline__ int src_word(int e, int W, int C, bool fc) {
  if (!fc) return e;
  const int w = e / C;
  return (W - 1 - w) * C + (e - w * C);
}

// row -> (image n, row h) -> the source row's first word
__device__ __forceinline__ long long src_row(long long row, int H, int L, bool fr, const int* __restrict__ idx) {
  const int n = (int)(row / H), h = (int)(row - (long long)n * H);
  const int sn = idx ? idx[n] : n;
  return ((long long)sn * H + (fr ? H - 1 - h : h)) * L;
}

__device__ __forceinline__ uint4 load_quad(const unsigned* __restrict__ s, int j, int W, int C, bool fc, bool vec) {
  if (!fc && vec) return *reinterpret_cast<const uint4*>(s + j);
  return make_uint4(s[src_word(j, W, C, fc)], s[src_word(j + 1, W, C, fc)], s[src_word(j + 2, W, C, fc)], s[src_word(j + 3, W, C, fc)]);
}

// dst row-quads <- src; kVec: the source rows are 16-byte aligned as well (used when the columns are not mirrored)
template <bool kVec>
__global__ __launch_bounds__(256) void view_gather_quad_k(const unsigned* __restrict__ src, const int* __restrict__ idx, int H, int W, int C,
                                                          int fr, int fc, unsigned* __restrict__ dst, long long quads) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= quads) return;
  const int L = W * C, Lq = L >> 2;
  const long long row = t / Lq;
  const int j = (int)(t - row * Lq) << 2;
  const uint4 v = load_quad(src + src_row(row, H, L, fr != 0, idx), j, W, C, fc != 0, kVec);
  *reinterpret_cast<uint4*>(dst + row * L + j) = v;
}

__global__ __launch_bounds__(256) void view_gather_word_k(const unsigned* __restrict__ src, const int* __restrict__ idx, int H, int W, int C,
                                                          int fr, int fc, unsigned* __restrict__ dst, long long words) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= words) return;
  const int L = W * C;
  const long long row = t / L;
  const int e = (int)(t - row * L);
  dst[t] = src[src_row(row, H, L, fr != 0, idx) + src_word(e, W, C, fc != 0)];
}

// (a + b) * scale: one rounding each; scalar fp32 arithmetic on the components of the 16-byte loads (the file is built without the SLP
// vectoriser: no packed fp32 form, common.hpp: lone())
template <bool kHasA>
__device__ __forceinline__ float merge1(float a, float b, float scale) {
  return kHasA ? (a + b) * scale : b * scale;
}

// dst may be a: no __restrict__ on the pair, every thread reads its own elements of a before it writes them
template <bool kHasA>
__global__ __launch_bounds__(256) void view_merge_quad_k(float* dst, const float* a, const float* __restrict__ b, int H, int W, int C, int fr,
                                                         int fc, float scale, long long quads) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= quads) return;
  const int L = W * C, Lq = L >> 2;
  const long long row = t / Lq;
  const int j = (int)(t - row * Lq) << 2;
  const uint4 u = load_quad(reinterpret_cast<const unsigned*>(b) + src_row(row, H, L, fr != 0, nullptr), j, W, C, fc != 0, true);
  float4 x = f4zero();
  if (kHasA) x = ld4(a + row * L + j);
  float4 o;
  o.x = merge1<kHasA>(x.x, __uint_as_float(u.x), scale);
  o.y = merge1<kHasA>(x.y, __uint_as_float(u.y), scale);
  o.z = merge1<kHasA>(x.z, __uint_as_float(u.z), scale);
  o.w = merge1<kHasA>(x.w, __uint_as_float(u.w), scale);
  st4(dst + row * L + j, o);
}

template <bool kHasA>
__global__ __launch_bounds__(256) void view_merge_word_k(float* dst, const float* a, const float* __restrict__ b, int H, int W, int C, int fr,
                                                         int fc, float scale, long long words) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= words) return;
  const int L = W * C;
  const long long row = t / L;
  const int e = (int)(t - row * L);
  const float y = b[src_row(row, H, L, fr != 0, nullptr) + src_word(e, W, C, fc != 0)];
  dst[t] = merge1<kHasA>(kHasA ? a[t] : 0.f, y, scale);
}

static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
// [p, p + bytes) and [q, q + bytes) share a byte
static inline bool overlap(const void* p, const void* q, long long bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(p), y = reinterpret_cast<uintptr_t>(q);
  return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}

}  // namespace mliis

using namespace mliis;

extern "C" {

const char* mliis_tta_last_error(void) { return g_tta_err; }

// include/mliis_tta.h.  One launch.
int mliis_view_gather(const float* src, const int* img_idx, int N, int H, int W, int C, int flip_rows, int flip_cols, float* dst,
                      hipStream_t stream) {
  MLIIS_REQUIRE(src && dst, MLIIS_ERR_ARG, "view_gather: null pointer");
  MLIIS_REQUIRE(N > 0 && H > 0 && W > 0, MLIIS_ERR_ARG, "view_gather: bad shape %d x %d x %d", N, H, W);
  MLIIS_REQUIRE(C >= 1 && C <= 4, MLIIS_ERR_ARG, "view_gather: %d channels (1..4 are supported)", C);
  const long long words = (long long)N * H * W * C;
  MLIIS_REQUIRE((long long)N * H <= 0x7fffffffLL && (long long)W * C <= 0x7fffffffLL && words <= 0x7fffffffLL, MLIIS_ERR_UNSUPPORTED,
                "view_gather: more than 2^31 - 1 elements");
  MLIIS_REQUIRE(aligned4(src) && aligned4(dst) && aligned4(img_idx), MLIIS_ERR_ALIGN, "view_gather: pointers must be 4-byte aligned");
  MLIIS_REQUIRE(!overlap(dst, src, words * 4), MLIIS_ERR_ARG, "view_gather: dst overlaps src (no in-place form)");
  const int L = W * C;
  const unsigned* s = reinterpret_cast<const unsigned*>(src);
  unsigned* d = reinterpret_cast<unsigned*>(dst);
  if ((L & 3) == 0 && aligned16(dst)) {
    const long long quads = words >> 2;
    if (aligned16(src))
      hipLaunchKernelGGL(view_gather_quad_k<true>, dim3(ceil_div(quads, 256)), dim3(256), 0, stream, s, img_idx, H, W, C, flip_rows, flip_cols, d, quads);
    else
      hipLaunchKernelGGL(view_gather_quad_k<false>, dim3(ceil_div(quads, 256)), dim3(256), 0, stream, s, img_idx, H, W, C, flip_rows, flip_cols, d, quads);
  } else {
    hipLaunchKernelGGL(view_gather_word_k, dim3(ceil_div(words, 256)), dim3(256), 0, stream, s, img_idx, H, W, C, flip_rows, flip_cols, d, words);
  }
  MLIIS_CHECK_LAUNCH("view_gather");
  return MLIIS_OK;
}

// include/mliis_tta.h.  One launch.
int mliis_view_merge(float* dst, const float* a, const float* b, int N, int Hd, int Wd, int C, int flip_rows, int flip_cols, float scale,
                     hipStream_t stream) {
  MLIIS_REQUIRE(dst && b, MLIIS_ERR_ARG, "view_merge: null pointer");
  MLIIS_REQUIRE(N > 0 && Hd > 0 && Wd > 0, MLIIS_ERR_ARG, "view_merge: bad shape %d x %d x %d", N, Hd, Wd);
  MLIIS_REQUIRE(C >= 1 && C <= 4, MLIIS_ERR_ARG, "view_merge: %d channels (1..4 are supported)", C);
  MLIIS_REQUIRE(scale > 0.f && scale <= 3.402823466e38f, MLIIS_ERR_ARG, "view_merge: scale must be finite and positive, got %g", (double)scale);
  const long long words = (long long)N * Hd * Wd * C;
  MLIIS_REQUIRE((long long)N * Hd <= 0x7fffffffLL && (long long)Wd * C <= 0x7fffffffLL && words <= 0x7fffffffLL, MLIIS_ERR_UNSUPPORTED,
                "view_merge: more than 2^31 - 1 elements");
  MLIIS_REQUIRE(aligned4(dst) && aligned4(a) && aligned4(b), MLIIS_ERR_ALIGN, "view_merge: pointers must be 4-byte aligned");
  MLIIS_REQUIRE(!overlap(dst, b, words * 4), MLIIS_ERR_ARG, "view_merge: dst overlaps b (only dst == a is merged in place)");
  MLIIS_REQUIRE(!a || a == dst || !overlap(dst, a, words * 4), MLIIS_ERR_ARG, "view_merge: dst overlaps a without being a");
  const int L = Wd * C;
  if ((L & 3) == 0 && aligned16(dst) && aligned16(b) && aligned16(a)) {
    const long long quads = words >> 2;
    if (a)
      hipLaunchKernelGGL(view_merge_quad_k<true>, dim3(ceil_div(quads, 256)), dim3(256), 0, stream, dst, a, b, Hd, Wd, C, flip_rows, flip_cols, scale, quads);
    else
      hipLaunchKernelGGL(view_merge_quad_k<false>, dim3(ceil_div(quads, 256)), dim3(256), 0, stream, dst, a, b, Hd, Wd, C, flip_rows, flip_cols, scale, quads);
  } else {
    if (a)
      hipLaunchKernelGGL(view_merge_word_k<true>, dim3(ceil_div(words, 256)), dim3(256), 0, stream, dst, a, b, Hd, Wd, C, flip_rows, flip_cols, scale, words);
    else
      hipLaunchKernelGGL(view_merge_word_k<false>, dim3(ceil_div(words, 256)), dim3(256), 0, stream, dst, a, b, Hd, Wd, C, flip_rows, flip_cols, scale, words);
  }
  MLIIS_CHECK_LAUNCH("view_merge");
  return MLIIS_OK;
}
}
