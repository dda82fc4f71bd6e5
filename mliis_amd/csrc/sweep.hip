// libmliis_sweep.so: the evaluation threshold sweep -- per-image histograms of the foreground probability (include/mliis_sweep.h).  A
// library of its own beside libmliis_hip.so and libmliis_score.so, neither of which (nor their headers) is touched by it; it shares the
// per-pixel arithmetic of the decoder tail with head.hip and score.hip through head_math.hpp.
#include "../../include/mliis_sweep.h"
#include "common.hpp"
#include "head_math.hpp"

namespace mliis {

// (this library's own error slot: common.hpp's MLIIS_REQUIRE / MLIIS_CHECK_LAUNCH report through set_error of the library they are linked into)
MLIIS_DEFINE_ERROR_SLOT(g_sweep_err)

constexpr int kBins = 256;      // bins per label class (mliis_prob_hist_bins)
constexpr int kStrip = 4096;    // image pixels per workgroup: 16 per thread
constexpr int kAhead = 4;       // pixels per thread whose loads are issued together (kStrip / 256 is a multiple)

__global__ __launch_bounds__(256) void zero_hist_k(unsigned* __restrict__ dst, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = 0u;
}
// The bin of the channel-1 probability of image pixel p of image n.  p1 is formed exactly as score.hip's predict_pixel forms it (the same
// calls in the same order: tests/test_sweep_gpu.py holds the k = 128 counts against mliis_mask_iou_counts bit for bit); p1 * 256 is exact,
// so b >= k <=> p1 > k/256 for k = 1..255.
__device__ __forceinline__ int prob_bin(const float* __restrict__ small, int n, int p, int Hi, int Wi, int Wo, float sh, float sw) {
  const int ho = p / Wo, wo = p - ho * Wo;
  int y0, y1, x0, x1;
  float ly, lx;
  src_coord(ho, sh, Hi, y0, y1, ly);
  src_coord(wo, sw, Wi, x0, x1, lx);
  const float2 zz = bilinear_sample<float2>(small + (long long)n * Hi * Wi * 2, Wi, 2, y0, y1, x0, x1, ly, lx);
  float p0, p1;
  softmax2(zz, p0, p1);
  const int b = (int)ceilf(p1 * 256.f) - 1;
  return b < 0 ? 0 : (b > kBins - 1 ? kBins - 1 : b);
}
// The class of label pixel p of label image src (labels [S,H,W,2]): score.hip's label_pixel.
__device__ __forceinline__ int label_class(const float* __restrict__ labels, int src, int HW, int p) {
  const float2 tt = *reinterpret_cast<const float2*>(labels + ((long long)src * HW + p) * 2);
  return rintf(tt.y) != 0.f ? 1 : 0;
}

// hist[n][c][b] += the pixels of one strip of image n.  A workgroup covers kStrip consecutive pixels of one image (blockIdx.y), thread t
// the pixels strip + 256 i + t; every wave counts into a table of its own in LDS (4 x 2 x 256 words = 8 KB) with LDS integer atomics, and
// after the strip the workgroup adds the non-zero sums of the four tables to hist[n] with global integer atomics: at most 512 per
// workgroup, contiguous within the image's 2 KB row.  hist is zeroed by a launch in front (zero_hist_k); integer addition is
// associative, so the result does not depend on the order workgroups or lanes arrive in -- no fence, no ticket, no fold.
// The probabilities of a segmenter pile up at the two ends, where many lanes of a wave add to one LDS address.  Counting bins 0 and 255 of
// either class per wave with a ballot and a popcount instead (as score.hip's add_counts counts its masks), and sending only the lanes in
// between to LDS, was measured and is NOT done: on logits N(0, 8) (45 % of the pixels in the end bins) the launch pair took 18.3 us with the
// split against 16.9 us without it at 64 images, and the two cannot be told apart at 5 and 11 images, where the launches' issue bounds the
// pair (profiles/sweep.md).  Every lane goes to the LDS atomics.
__global__ __launch_bounds__(256) void prob_histogram_k(const float* __restrict__ small, const float* __restrict__ labels,
                                                        const int* __restrict__ idx, int Hi, int Wi, int Ho, int Wo, float sh, float sw,
                                                        unsigned* __restrict__ hist) {
  __shared__ unsigned tab[4][2 * kBins];
  const int wave = threadIdx.x >> 6;
  for (int s = threadIdx.x; s < 4 * 2 * kBins; s += 256) (&tab[0][0])[s] = 0u;
  __syncthreads();
  const int n = blockIdx.y;
  const int src = idx ? idx[n] : n;
  const int HW = Ho * Wo;
  const long long strip = (long long)blockIdx.x * kStrip;   // (64-bit: the last strip's end may pass 2^31 - 1 although H W does not)
  for (int i = 0; i < kStrip / 256; i += kAhead) {
    const long long first = strip + (long long)i * 256;
    if (first >= HW) break;   // (uniform over the workgroup)
    int slot[kAhead];         // kAhead pixels' loads in flight before the first is counted; -1 = past the image
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      const long long pl = first + j * 256 + threadIdx.x;
      const int p = pl < HW ? (int)pl : HW - 1;   // (a lane past the image reads its last pixel: straight-line code, no load behind a branch)
      const int s = label_class(labels, src, HW, p) * kBins + prob_bin(small, n, p, Hi, Wi, Wo, sh, sw);
      slot[j] = pl < HW ? s : -1;
    }
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      if (slot[j] >= 0) atomicAdd(&tab[wave][slot[j]], 1u);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < 2 * kBins; s += 256) {
    const unsigned v = tab[0][s] + tab[1][s] + tab[2][s] + tab[3][s];
    if (v != 0u) atomicAdd(hist + (long long)n * (2 * kBins) + s, v);
  }
}

}  // namespace mliis

using namespace mliis;

extern "C" {

const char* mliis_sweep_last_error(void) { return g_sweep_err; }

int mliis_prob_hist_bins(void) { return kBins; }

// include/mliis_sweep.h.  Two launches (zero, count); any Hd <= H, Wd <= W.
int mliis_prob_histogram(const float* small, const float* labels, const int* img_idx, int N, int Hd, int Wd, int H, int W, unsigned* hist,
                         hipStream_t stream) {
  MLIIS_REQUIRE(small && labels && hist, MLIIS_ERR_ARG, "prob_histogram: null pointer");
  MLIIS_REQUIRE(N > 0 && Hd > 0 && Wd > 0 && H > 1 && W > 1 && N <= 65535, MLIIS_ERR_ARG,
                "prob_histogram: bad shape (the image must be larger than 1x1, as for mliis_resize_bilinear_fwd)");
  MLIIS_REQUIRE(H >= Hd && W >= Wd, MLIIS_ERR_ARG, "prob_histogram: the image (%d x %d) is smaller than the decoder's map (%d x %d)", H, W, Hd, Wd);
  MLIIS_REQUIRE((long long)H * W <= 0x7fffff00LL, MLIIS_ERR_UNSUPPORTED, "prob_histogram: image too large for 32-bit pixel counts");
  MLIIS_REQUIRE((reinterpret_cast<uintptr_t>(small) & 7u) == 0 && (reinterpret_cast<uintptr_t>(labels) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(hist) & 3u) == 0,
                MLIIS_ERR_ALIGN, "prob_histogram: small / labels must be 8-byte aligned, hist 4-byte aligned");
  const float sh = (float)(Hd - 1) / (float)(H - 1), sw = (float)(Wd - 1) / (float)(W - 1);   // (mliis_resize_bilinear_fwd's scales)
  const int words = N * 2 * kBins;
  hipLaunchKernelGGL(zero_hist_k, dim3(ceil_div(words, 256)), dim3(256), 0, stream, hist, words);
  MLIIS_CHECK_LAUNCH("prob_histogram_zero");
  hipLaunchKernelGGL(prob_histogram_k, dim3(ceil_div((long long)H * W, kStrip), N), dim3(256), 0, stream, small, labels, img_idx, Hd, Wd, H, W, sh,
                     sw, hist);
  MLIIS_CHECK_LAUNCH("prob_histogram");
  return MLIIS_OK;
}
}
