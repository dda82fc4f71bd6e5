// libmliis_region.so: the Tversky region term of the inner loop's loss (include/mliis_region.h) on the focal, foreground-weighted pixel
// term -- the counterparts of focal.hip's chain (focal_partial_k / focal_finalize_k / focal_grad_k) and of its fused head for a learner
// built with tversky=(alpha, beta).  A library of its own beside libmliis_hip.so and libmliis_loss.so.  The kernel bodies -- the
// partial-sum pass, the fold, the gradient pass, the fused head's tiling -- and the geometry are loss_kernels.hpp's, the ones head.hip's
// and focal.hip's kernels run, through their hooks: the fold's per-image part (TverskyRegion), the region gradient (TverskyGrad) and, for
// the fused head's sums, a logits source that rebuilds an image pixel's logits from the decoder's map (ResizedLogits).  The per-pixel
// policy is FocalPixel of focal_math.hpp throughout.
#include "../../include/mliis_region.h"
#include "common.hpp"
#include "focal_math.hpp"
#include "loss_kernels.hpp"

namespace mliis {

// (this library's own error slot: common.hpp's MLIIS_REQUIRE / MLIIS_CHECK_LAUNCH report through set_error of the library they are linked into)
MLIIS_DEFINE_ERROR_SLOT(g_region_err)

// the fold's per-image part: T_n = (I + eps) / D_n with D_n = I + alpha (Sp - I) + beta (St - I) + eps beside the soft IoU (out[2]), and
// the pair {1 / D_n, (I + eps) / D_n^2} the fold scales by (dL/dT) / N into coef[n] = {A_n, B_n}
struct TverskyRegion {
  static constexpr int kIndices = 2;
  int on;
  double alpha, beta;
  __device__ __forceinline__ double image(double I, double Sp, double St, double iou_n, float* __restrict__ coef, int n) const {
    const double eps = 1e-7;
    const double D = I + alpha * (Sp - I) + beta * (St - I) + eps;
    coef[2 * n + 0] = (float)(1.0 / D);
    coef[2 * n + 1] = (float)((I + eps) / (D * D));
    return (I + eps) / D;
  }
};

// the region term's d / dz1 at a pixel: (A_n y1 - B_n (alpha + (1 - alpha - beta) y1)) p1 (1 - p1); rest = 1 - alpha - beta (the host
// forms it in double); alpha = beta = 1 is JaccardGrad's expression
struct TverskyGrad {
  float alpha, rest;
  __device__ __forceinline__ float operator()(float An, float Bn, float y1, float p1) const {
    return (An * y1 - Bn * (alpha + rest * y1)) * p1 * (1.f - p1);
  }
};

// image pixel p's logits from the decoder's map: resize_fwd_k's arithmetic, what phase 1 of head_fused_tile forms for the same pixel
struct ResizedLogits {
  const float* small;   // [N][Hi][Wi][2]
  int Hi, Wi, Wo;
  float sh, sw;
  struct Image {
    const float* zb;
    int Hi, Wi, Wo;
    float sh, sw;
    __device__ __forceinline__ float2 operator()(int p) const {
      const int ho = p / Wo, wo = p - ho * Wo;
      int y0, y1, x0, x1;
      float ly, lx;
      src_coord(ho, sh, Hi, y0, y1, ly);
      src_coord(wo, sw, Wi, x0, x1, lx);
      return bilinear_sample<float2>(zb, Wi, 2, y0, y1, x0, x1, ly, lx);
    }
  };
  __device__ __forceinline__ Image image(int n) const { return Image{small + (long long)n * Hi * Wi * 2, Hi, Wi, Wo, sh, sw}; }
};

__global__ __launch_bounds__(256) void tversky_partial_k(const float* __restrict__ logits, const float* __restrict__ labels,
                                                         const int* __restrict__ idx, int HW, float ls, float gamma, float fgw,
                                                         float* __restrict__ part) {
  loss_partial(FocalPixel{ls, gamma, fgw, 0.f}, logits, labels, idx, HW, part);
}

// the fused head's sums: grid (part_blocks(Ho Wo), N), one image pixel per thread with loss_partial's grid-stride
__global__ __launch_bounds__(256) void head_tversky_sums_k(const float* __restrict__ small, const float* __restrict__ labels,
                                                           const int* __restrict__ idx, int Hi, int Wi, int Ho, int Wo, float sh, float sw,
                                                           float ls, float gamma, float fgw, float* __restrict__ part) {
  loss_partial_from(FocalPixel{ls, gamma, fgw, 0.f}, ResizedLogits{small, Hi, Wi, Wo, sh, sw}, labels, idx, Ho * Wo, part);
}

__global__ __launch_bounds__(256) void tversky_fold_k(const float* __restrict__ part, int nblk, int N, int HW, double alpha, double beta,
                                                      float extra_loss, float* __restrict__ out, float* __restrict__ coef) {
  loss_fold_with(TverskyRegion{1, alpha, beta}, part, nblk, N, HW, extra_loss, out, coef);
}

__global__ __launch_bounds__(256) void tversky_grad_k(const float* __restrict__ logits, const float* __restrict__ labels,
                                                      const int* __restrict__ idx, int HW, float ls, float gamma, float fgw, float inv_rows,
                                                      float alpha, float rest, const float* __restrict__ coef, float* __restrict__ dlogits) {
  loss_grad(FocalPixel{ls, gamma, fgw, inv_rows}, logits, labels, idx, HW, coef, dlogits, nullptr, nullptr, 0, 0, 0.f, nullptr, nullptr,
            TverskyGrad{alpha, rest});
}

__global__ __launch_bounds__(256) void head_tversky_tile_k(const float* __restrict__ small, const float* __restrict__ labels,
                                                           const int* __restrict__ idx, int Hi, int Wi, int Ho, int Wo, float sh, float sw,
                                                           float ls, float gamma, float fgw, float inv_rows, float alpha, float rest,
                                                           const float* __restrict__ coef, float* __restrict__ dsmall, int tiles_x) {
  head_fused_tile(FocalPixel{ls, gamma, fgw, inv_rows}, small, labels, idx, Hi, Wi, Ho, Wo, sh, sw, dsmall, nullptr, tiles_x, coef,
                  TverskyGrad{alpha, rest});
}

// the scalars every entry point takes (include/mliis_region.h: refused before any launch)
static int check_scalars(const char* name, float ls, float gamma, float fgw, float alpha, float beta) {
  MLIIS_REQUIRE(std::isfinite(alpha) && alpha >= 0.f, MLIIS_ERR_ARG, "%s: alpha must be finite and >= 0, got %g", name, (double)alpha);
  MLIIS_REQUIRE(std::isfinite(beta) && beta >= 0.f, MLIIS_ERR_ARG, "%s: beta must be finite and >= 0, got %g", name, (double)beta);
  MLIIS_REQUIRE(alpha + beta > 0.f, MLIIS_ERR_ARG, "%s: alpha + beta must be > 0", name);
  MLIIS_REQUIRE(std::isfinite(gamma) && gamma >= 0.f, MLIIS_ERR_ARG, "%s: gamma must be finite and >= 0, got %g", name, (double)gamma);
  MLIIS_REQUIRE(std::isfinite(fgw) && fgw > 0.f, MLIIS_ERR_ARG, "%s: fg_weight must be finite and > 0, got %g", name, (double)fgw);
  MLIIS_REQUIRE(ls >= 0.f && ls < 1.f, MLIIS_ERR_ARG, "%s: label_smoothing must be in [0, 1), got %g", name, (double)ls);
  return MLIIS_OK;
}

}  // namespace mliis

using namespace mliis;

extern "C" {

const char* mliis_region_last_error(void) { return g_region_err; }

size_t mliis_tversky_ce_workspace_floats(int N, int H, int W) { return loss_workspace_floats(N, H, W); }

// include/mliis_region.h.  ws = [N][nblk][4] partials, then coef [N][2].
int mliis_tversky_ce(const float* logits, const float* labels, const int* img_idx, int N, int H, int W, float label_smoothing, float gamma,
                     float fg_weight, float alpha, float beta, float extra_loss, float* dlogits, float* out, float* ws, size_t ws_floats,
                     hipStream_t stream) {
  MLIIS_REQUIRE(logits && labels && out && ws, MLIIS_ERR_ARG, "tversky_ce: null pointer");
  MLIIS_REQUIRE(N > 0 && H > 0 && W > 0 && N <= 65535 && (long long)H * W <= (1LL << 29), MLIIS_ERR_ARG,
                "tversky_ce: bad shape (N, H, W positive, N <= 65535, H W <= 2^29)");
  const int rc = check_scalars("tversky_ce", label_smoothing, gamma, fg_weight, alpha, beta);
  if (rc) return rc;
  MLIIS_REQUIRE(aligned8(logits) && aligned8(labels) && aligned8(dlogits), MLIIS_ERR_ALIGN, "tversky_ce: logits / labels / dlogits must be 8-byte aligned");
  MLIIS_REQUIRE(ws_floats >= mliis_tversky_ce_workspace_floats(N, H, W) && aligned16(ws), MLIIS_ERR_WORKSPACE,
                "tversky_ce: workspace too small or unaligned (%zu floats given, %zu needed)", ws_floats, mliis_tversky_ce_workspace_floats(N, H, W));
  const int HW = H * W;
  const int nblk = part_blocks(HW);
  float* coef = ws + (size_t)N * nblk * 4;
  hipLaunchKernelGGL(tversky_partial_k, dim3(nblk, N), dim3(256), 0, stream, logits, labels, img_idx, HW, label_smoothing, gamma, fg_weight, ws);
  MLIIS_CHECK_LAUNCH("tversky_ce_partial");
  hipLaunchKernelGGL(tversky_fold_k, dim3(1), dim3(256), 0, stream, ws, nblk, N, HW, (double)alpha, (double)beta, extra_loss, out, coef);
  MLIIS_CHECK_LAUNCH("tversky_ce_fold");
  if (dlogits) {
    hipLaunchKernelGGL(tversky_grad_k, dim3(ceil_div(HW, 256), N), dim3(256), 0, stream, logits, labels, img_idx, HW, label_smoothing, gamma,
                       fg_weight, 1.0f / ((float)N * (float)HW), alpha, (float)(1.0 - (double)alpha - (double)beta), coef, dlogits);
    MLIIS_CHECK_LAUNCH("tversky_ce_grad");
  }
  return MLIIS_OK;
}

int mliis_head_tversky_fused_supported(int Hd, int Wd, int H, int W) { return head_fused_supported(Hd, Wd, H, W); }

// the sums' partials are per partial block of the IMAGE ([N][part_blocks(H W)][4], then coef [N][2]): the chain's workspace
size_t mliis_head_tversky_fused_workspace_floats(int N, int Hd, int Wd, int H, int W) {
  if (Hd <= 0 || Wd <= 0) return 0;
  return loss_workspace_floats(N, H, W);
}

// include/mliis_region.h.  ws = [N][nblk][4] partials of the sums, then coef [N][2].
int mliis_head_tversky_fused(const float* small, const float* labels, const int* img_idx, int N, int Hd, int Wd, int H, int W,
                             float label_smoothing, float gamma, float fg_weight, float alpha, float beta, float extra_loss, float* dsmall,
                             float* out, float* ws, size_t ws_floats, hipStream_t stream) {
  MLIIS_REQUIRE(small && labels && dsmall && out && ws, MLIIS_ERR_ARG, "head_tversky_fused: null pointer");
  MLIIS_REQUIRE(N > 0 && Hd > 1 && Wd > 1 && H > 1 && W > 1 && N <= 65535 && (long long)H * W <= (1LL << 29) && Hd <= 32768 && Wd <= 32768,
                MLIIS_ERR_ARG, "head_tversky_fused: bad shape (both maps must be larger than 1x1)");
  const int rc = check_scalars("head_tversky_fused", label_smoothing, gamma, fg_weight, alpha, beta);
  if (rc) return rc;
  MLIIS_REQUIRE(mliis_head_tversky_fused_supported(Hd, Wd, H, W), MLIIS_ERR_UNSUPPORTED,
                "head_tversky_fused: up-sampling factor too large for the tile footprint (mliis_head_tversky_fused_supported)");
  MLIIS_REQUIRE(aligned8(small) && aligned8(labels) && aligned8(dsmall), MLIIS_ERR_ALIGN, "head_tversky_fused: tensors must be 8-byte aligned");
  MLIIS_REQUIRE(ws_floats >= mliis_head_tversky_fused_workspace_floats(N, Hd, Wd, H, W) && aligned16(ws), MLIIS_ERR_WORKSPACE,
                "head_tversky_fused: workspace too small or unaligned (%zu floats given, %zu needed)", ws_floats,
                mliis_head_tversky_fused_workspace_floats(N, Hd, Wd, H, W));
  const int HW = H * W;
  const int nblk = part_blocks(HW);
  const int tx = head_tiles(Wd), tiles = head_tiles(Hd) * tx;
  float* coef = ws + (size_t)N * nblk * 4;
  const float sh = (float)(Hd - 1) / (float)(H - 1), sw = (float)(Wd - 1) / (float)(W - 1);
  hipLaunchKernelGGL(head_tversky_sums_k, dim3(nblk, N), dim3(256), 0, stream, small, labels, img_idx, Hd, Wd, H, W, sh, sw, label_smoothing,
                     gamma, fg_weight, ws);
  MLIIS_CHECK_LAUNCH("head_tversky_sums");
  hipLaunchKernelGGL(tversky_fold_k, dim3(1), dim3(256), 0, stream, ws, nblk, N, HW, (double)alpha, (double)beta, extra_loss, out, coef);
  MLIIS_CHECK_LAUNCH("head_tversky_fold");
  hipLaunchKernelGGL(head_tversky_tile_k, dim3(tiles, N), dim3(256), 0, stream, small, labels, img_idx, Hd, Wd, H, W, sh, sw, label_smoothing,
                     gamma, fg_weight, 1.0f / ((float)N * (float)H * (float)W), alpha, (float)(1.0 - (double)alpha - (double)beta), coef,
                     dsmall, tx);
  MLIIS_CHECK_LAUNCH("head_tversky_tile");
  return MLIIS_OK;
}
}
