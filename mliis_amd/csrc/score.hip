// libmliis_score.so: scoring an evaluation batch on the device, and handing out its masks one bit per pixel (include/mliis_score.h).  A library of its own beside libmliis_hip.so --
// the training step's library and its C ABI (include/mliis_hip.h) are untouched by it -- that shares the per-pixel arithmetic of the
// decoder tail with head.hip through head_math.hpp.
// Reference: meta_learners/supervised_reptile/supervised_reptile/reptile.py:526-549 (_iou) behind models/efficientlab.py:166-176.
#include "../../include/mliis_score.h"
#include "common.hpp"
#include "head_math.hpp"

namespace mliis {

// (this library's own error slot: common.hpp's MLIIS_REQUIRE / MLIIS_CHECK_LAUNCH report through set_error of the library they are linked into)
MLIIS_DEFINE_ERROR_SLOT(g_score_err)

// Scoring an evaluation image needs two integers, not a mask: counts[n] = {|P & L|, |P | L|, |P|, |L|} with P the channel-1 prediction
// (the resize of `small` to the image, softmax, p1 > 0.5f -- bilinear_sample / softmax2, the arithmetic of resize_fwd_k<2> followed by
// ce_grad_k, so near-ties fall as they do there) and L = rintf(label channel 1) != 0 (np.round(...).astype(bool): half to even, any
// non-zero value counts).  One thread per IMAGE pixel gathers its four decoder pixels itself: no tile footprint, any Hd <= H; neither
// the full-resolution logits nor the mask are written.  A wave counts with two ballots and four popcounts, the four waves of a
// workgroup meet in LDS and four lanes add the workgroup's sums to counts[n] with integer atomicAdd -- counts is zeroed by a launch in
// front (zero_words_k).  Integer addition is associative, so the result does not depend on the order the workgroups arrive in; the
// alternative, per-workgroup partials and a fold launch, needs a workspace for 196 x 4 ints per 224 x 224 image and reads them back for
// the same integers.  (No last-arriver fold: see head_ce_fused_k's header in head.hip for what a device-scope fence costs on this part.)
__global__ __launch_bounds__(256) void zero_words_k(int* __restrict__ dst, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = 0;
}
// The channel-1 prediction of image pixel p of image n: the one place the mask is formed (the counts kernel and the packing kernel).
__device__ __forceinline__ bool predict_pixel(const float* __restrict__ small, int n, int p, int Hi, int Wi, int Wo, float sh, float sw) {
  const int ho = p / Wo, wo = p - ho * Wo;
  int y0, y1, x0, x1;
  float ly, lx;
  src_coord(ho, sh, Hi, y0, y1, ly);
  src_coord(wo, sw, Wi, x0, x1, lx);
  const float2 zz = bilinear_sample<float2>(small + (long long)n * Hi * Wi * 2, Wi, 2, y0, y1, x0, x1, ly, lx);
  float p0, p1;
  softmax2(zz, p0, p1);
  return p1 > 0.5f;
}
// L of label pixel p of label image src (labels [S,H,W,2]).
__device__ __forceinline__ bool label_pixel(const float* __restrict__ labels, int src, int HW, int p) {
  const float2 tt = *reinterpret_cast<const float2*>(labels + ((long long)src * HW + p) * 2);
  return rintf(tt.y) != 0.f;
}
// A workgroup's four waves' counts meet in LDS and four lanes add them to counts[n] (call with all 256 threads).
__device__ __forceinline__ void add_counts(int (*sm)[4], unsigned long long mp, unsigned long long ml, int n, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sm[wave][0] = __popcll(mp & ml);
    sm[wave][1] = __popcll(mp | ml);
    sm[wave][2] = __popcll(mp);
    sm[wave][3] = __popcll(ml);
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int s = sm[0][threadIdx.x] + sm[1][threadIdx.x] + sm[2][threadIdx.x] + sm[3][threadIdx.x];
    if (s != 0) atomicAdd(counts + (long long)n * 4 + threadIdx.x, s);
  }
}
__global__ __launch_bounds__(256) void mask_iou_counts_k(const float* __restrict__ small, const float* __restrict__ labels,
                                                         const int* __restrict__ idx, int Hi, int Wi, int Ho, int Wo, float sh, float sw,
                                                         int* __restrict__ counts) {
  __shared__ int sm[4][4];
  const int n = blockIdx.y;
  const int src = idx ? idx[n] : n;
  const int HW = Ho * Wo;
  const int p = blockIdx.x * 256 + threadIdx.x;
  bool pb = false, lb = false;
  if (p < HW) {
    pb = predict_pixel(small, n, p, Hi, Wi, Wo, sh, sw);
    lb = label_pixel(labels, src, HW, p);
  }
  const unsigned long long mp = __ballot(pb), ml = __ballot(lb);
  add_counts(sm, mp, ml, n, counts);
}

// The mask itself, one bit per pixel: the ballot the counts kernel popcounts is the word.  Same launch shape -- a workgroup's first pixel
// is a multiple of 256, so wave v of workgroup b holds exactly word b * 4 + v of its image (pixels 64 w .. 64 w + 63, linear over the
// image: words straddle rows); lanes past H * W vote 0, so the last word's tail bits are 0, and a wave that starts past H * W stores
// nothing -- every word of [N][words] is written once, by lane 0 of its wave, and nothing else.  COUNTS: the counts kernel's tail as well
// (labels / idx / counts are not read otherwise).
template <bool COUNTS>
__global__ __launch_bounds__(256) void mask_pack_k(const float* __restrict__ small, const float* __restrict__ labels,
                                                   const int* __restrict__ idx, int Hi, int Wi, int Ho, int Wo, float sh, float sw, int words,
                                                   unsigned long long* __restrict__ bits, int* __restrict__ counts) {
  __shared__ int sm[4][4];
  const int n = blockIdx.y;
  const int HW = Ho * Wo;
  const int p = blockIdx.x * 256 + threadIdx.x;
  bool pb = false, lb = false;
  if (p < HW) {
    pb = predict_pixel(small, n, p, Hi, Wi, Wo, sh, sw);
    if (COUNTS) lb = label_pixel(labels, idx ? idx[n] : n, HW, p);
  }
  const unsigned long long mp = __ballot(pb);
  const int w = p >> 6;   // (uniform over the wave)
  if ((threadIdx.x & 63) == 0 && w < words) bits[(long long)n * words + w] = mp;
  if (COUNTS) add_counts(sm, mp, __ballot(lb), n, counts);
}

}  // namespace mliis

using namespace mliis;

extern "C" {

const char* mliis_score_last_error(void) { return g_score_err; }

// include/mliis_score.h.  Two launches (zero, count); any Hd <= H, Wd <= W.
int mliis_mask_iou_counts(const float* small, const float* labels, const int* img_idx, int N, int Hd, int Wd, int H, int W, int* counts,
                          hipStream_t stream) {
  MLIIS_REQUIRE(small && labels && counts, MLIIS_ERR_ARG, "mask_iou_counts: null pointer");
  MLIIS_REQUIRE(N > 0 && Hd > 0 && Wd > 0 && H > 1 && W > 1 && N <= 65535, MLIIS_ERR_ARG,
                "mask_iou_counts: bad shape (the image must be larger than 1x1, as for mliis_resize_bilinear_fwd)");
  MLIIS_REQUIRE(H >= Hd && W >= Wd, MLIIS_ERR_ARG, "mask_iou_counts: the image (%d x %d) is smaller than the decoder's map (%d x %d)", H, W, Hd, Wd);
  MLIIS_REQUIRE((long long)H * W <= 0x7fffff00LL, MLIIS_ERR_UNSUPPORTED, "mask_iou_counts: image too large for 32-bit pixel counts");
  MLIIS_REQUIRE((reinterpret_cast<uintptr_t>(small) & 7u) == 0 && (reinterpret_cast<uintptr_t>(labels) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(counts) & 3u) == 0,
                MLIIS_ERR_ALIGN, "mask_iou_counts: small / labels must be 8-byte aligned, counts 4-byte aligned");
  const float sh = (float)(Hd - 1) / (float)(H - 1), sw = (float)(Wd - 1) / (float)(W - 1);   // (mliis_resize_bilinear_fwd's scales)
  hipLaunchKernelGGL(zero_words_k, dim3(ceil_div((long long)N * 4, 256)), dim3(256), 0, stream, counts, N * 4);
  MLIIS_CHECK_LAUNCH("mask_iou_counts_zero");
  hipLaunchKernelGGL(mask_iou_counts_k, dim3(ceil_div((long long)H * W, 256), N), dim3(256), 0, stream, small, labels, img_idx, Hd, Wd, H, W, sh,
                     sw, counts);
  MLIIS_CHECK_LAUNCH("mask_iou_counts");
  return MLIIS_OK;
}

long long mliis_mask_pack_words(int H, int W) {
  if (H <= 0 || W <= 0) return -1;
  return ((long long)H * W + 63) / 64;
}

// include/mliis_score.h.  With labels and counts: two launches (zero, pack + count); without: the one packing launch.
int mliis_mask_pack(const float* small, const float* labels, const int* img_idx, int N, int Hd, int Wd, int H, int W,
                    unsigned long long* bits, int* counts, hipStream_t stream) {
  MLIIS_REQUIRE(small && bits, MLIIS_ERR_ARG, "mask_pack: null pointer");
  MLIIS_REQUIRE((labels == nullptr) == (counts == nullptr), MLIIS_ERR_ARG, "mask_pack: labels and counts go together (both or neither)");
  MLIIS_REQUIRE(N > 0 && Hd > 0 && Wd > 0 && H > 1 && W > 1 && N <= 65535, MLIIS_ERR_ARG,
                "mask_pack: bad shape (the image must be larger than 1x1, as for mliis_resize_bilinear_fwd)");
  MLIIS_REQUIRE(H >= Hd && W >= Wd, MLIIS_ERR_ARG, "mask_pack: the image (%d x %d) is smaller than the decoder's map (%d x %d)", H, W, Hd, Wd);
  MLIIS_REQUIRE((long long)H * W <= 0x7fffff00LL, MLIIS_ERR_UNSUPPORTED, "mask_pack: image too large for 32-bit pixel counts");
  MLIIS_REQUIRE((reinterpret_cast<uintptr_t>(small) & 7u) == 0 && (reinterpret_cast<uintptr_t>(labels) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(bits) & 7u) == 0 && (reinterpret_cast<uintptr_t>(counts) & 3u) == 0,
                MLIIS_ERR_ALIGN, "mask_pack: small / labels / bits must be 8-byte aligned, counts 4-byte aligned");
  const float sh = (float)(Hd - 1) / (float)(H - 1), sw = (float)(Wd - 1) / (float)(W - 1);   // (mliis_resize_bilinear_fwd's scales)
  const int words = (int)mliis_mask_pack_words(H, W);
  const dim3 grid(ceil_div((long long)H * W, 256), N);
  if (counts) {
    hipLaunchKernelGGL(zero_words_k, dim3(ceil_div((long long)N * 4, 256)), dim3(256), 0, stream, counts, N * 4);
    MLIIS_CHECK_LAUNCH("mask_pack_zero");
    hipLaunchKernelGGL(mask_pack_k<true>, grid, dim3(256), 0, stream, small, labels, img_idx, Hd, Wd, H, W, sh, sw, words, bits, counts);
  } else {
    hipLaunchKernelGGL(mask_pack_k<false>, grid, dim3(256), 0, stream, small, labels, img_idx, Hd, Wd, H, W, sh, sw, words, bits, counts);
  }
  MLIIS_CHECK_LAUNCH("mask_pack");
  return MLIIS_OK;
}
}
