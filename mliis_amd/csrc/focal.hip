// libmliis_loss.so: the focal, foreground-weighted pixel loss of the inner loop (include/mliis_loss.h) -- the counterparts of head.hip's
// softmax cross-entropy (ce_partial_k / ce_finalize_k / ce_grad_k) and of its fused head (head_ce_fused_k) for a learner built with
// focal_gamma != 0 or fg_weight != 1.  A library of its own beside libmliis_hip.so.  The kernel bodies -- the partial-sum pass, the fold,
// the gradient pass, the fused head's tiling -- and the geometry are loss_kernels.hpp's, the ones head.hip's kernels run; this file
// instantiates them with the per-pixel arithmetic of focal_math.hpp (FocalPixel) and holds the library's entry points.
#include "../../include/mliis_loss.h"
#include "common.hpp"
#include "focal_math.hpp"
#include "loss_kernels.hpp"

namespace mliis {

// (this library's own error slot: common.hpp's MLIIS_REQUIRE / MLIIS_CHECK_LAUNCH report through set_error of the library they are linked into)
MLIIS_DEFINE_ERROR_SLOT(g_loss_err)

__global__ __launch_bounds__(256) void focal_partial_k(const float* __restrict__ logits, const float* __restrict__ labels,
                                                       const int* __restrict__ idx, int HW, float ls, float gamma, float fgw,
                                                       float* __restrict__ part) {
  loss_partial(FocalPixel{ls, gamma, fgw, 0.f}, logits, labels, idx, HW, part);
}

__global__ __launch_bounds__(256) void focal_finalize_k(const float* __restrict__ part, int nblk, int N, int HW, int dice, float extra_loss,
                                                        float* __restrict__ out, float* __restrict__ coef) {
  loss_fold(part, nblk, N, HW, dice, extra_loss, out, coef);
}

__global__ __launch_bounds__(256) void focal_grad_k(const float* __restrict__ logits, const float* __restrict__ labels,
                                                    const int* __restrict__ idx, int HW, float ls, float gamma, float fgw, float inv_rows,
                                                    const float* __restrict__ coef, float* __restrict__ dlogits,
                                                    const float* __restrict__ fin_part, int fin_nblk, int N, float extra_loss,
                                                    float* __restrict__ fin_out, float* __restrict__ fin_coef) {
  loss_grad(FocalPixel{ls, gamma, fgw, inv_rows}, logits, labels, idx, HW, coef, dlogits, nullptr, fin_part, fin_nblk, N, extra_loss, fin_out,
            fin_coef);
}

__global__ __launch_bounds__(256) void head_focal_fused_k(const float* __restrict__ small, const float* __restrict__ labels,
                                                          const int* __restrict__ idx, int N, int Hi, int Wi, int Ho, int Wo, float sh, float sw,
                                                          float ls, float gamma, float fgw, float inv_rows, float* __restrict__ dsmall,
                                                          float* __restrict__ part, int tiles_x) {
  head_fused_tile(FocalPixel{ls, gamma, fgw, inv_rows}, small, labels, idx, Hi, Wi, Ho, Wo, sh, sw, dsmall, part, tiles_x);
}

// the scalars every entry point takes (include/mliis_loss.h: refused before any launch)
static int check_scalars(const char* name, float ls, float gamma, float fgw) {
  MLIIS_REQUIRE(std::isfinite(gamma) && gamma >= 0.f, MLIIS_ERR_ARG, "%s: gamma must be finite and >= 0, got %g", name, (double)gamma);
  MLIIS_REQUIRE(std::isfinite(fgw) && fgw > 0.f, MLIIS_ERR_ARG, "%s: fg_weight must be finite and > 0, got %g", name, (double)fgw);
  MLIIS_REQUIRE(ls >= 0.f && ls < 1.f, MLIIS_ERR_ARG, "%s: label_smoothing must be in [0, 1), got %g", name, (double)ls);
  return MLIIS_OK;
}

}  // namespace mliis

using namespace mliis;

extern "C" {

const char* mliis_loss_last_error(void) { return g_loss_err; }

size_t mliis_focal_ce_workspace_floats(int N, int H, int W) { return loss_workspace_floats(N, H, W); }

// include/mliis_loss.h.  ws = [N][nblk][4] partials, then coef [N][2].
int mliis_focal_ce(const float* logits, const float* labels, const int* img_idx, int N, int H, int W, float label_smoothing, float gamma,
                   float fg_weight, int dice, float extra_loss, float* dlogits, float* out, float* ws, size_t ws_floats, hipStream_t stream) {
  MLIIS_REQUIRE(logits && labels && out && ws, MLIIS_ERR_ARG, "focal_ce: null pointer");
  MLIIS_REQUIRE(N > 0 && H > 0 && W > 0 && N <= 65535 && (long long)H * W <= (1LL << 29), MLIIS_ERR_ARG,
                "focal_ce: bad shape (N, H, W positive, N <= 65535, H W <= 2^29)");
  const int rc = check_scalars("focal_ce", label_smoothing, gamma, fg_weight);
  if (rc) return rc;
  MLIIS_REQUIRE(aligned8(logits) && aligned8(labels) && aligned8(dlogits), MLIIS_ERR_ALIGN, "focal_ce: logits / labels / dlogits must be 8-byte aligned");
  MLIIS_REQUIRE(ws_floats >= mliis_focal_ce_workspace_floats(N, H, W) && aligned16(ws), MLIIS_ERR_WORKSPACE,
                "focal_ce: workspace too small or unaligned (%zu floats given, %zu needed)", ws_floats, mliis_focal_ce_workspace_floats(N, H, W));
  const int HW = H * W;
  const int nblk = part_blocks(HW);
  float* coef = ws + (size_t)N * nblk * 4;
  hipLaunchKernelGGL(focal_partial_k, dim3(nblk, N), dim3(256), 0, stream, logits, labels, img_idx, HW, label_smoothing, gamma, fg_weight, ws);
  MLIIS_CHECK_LAUNCH("focal_ce_partial");
  const bool merged = !dice && dlogits;   // (without the dice term the gradient does not depend on the fold)
  if (!merged) {
    hipLaunchKernelGGL(focal_finalize_k, dim3(1), dim3(256), 0, stream, ws, nblk, N, HW, dice, extra_loss, out, coef);
    MLIIS_CHECK_LAUNCH("focal_ce_finalize");
  }
  if (dlogits) {
    hipLaunchKernelGGL(focal_grad_k, dim3(ceil_div(HW, 256), N), dim3(256), 0, stream, logits, labels, img_idx, HW, label_smoothing, gamma,
                       fg_weight, 1.0f / ((float)N * (float)HW), coef, dlogits, merged ? ws : nullptr, nblk, N, extra_loss, out, coef);
    MLIIS_CHECK_LAUNCH("focal_ce_grad");
  }
  return MLIIS_OK;
}

int mliis_head_focal_fused_supported(int Hd, int Wd, int H, int W) { return head_fused_supported(Hd, Wd, H, W); }

size_t mliis_head_focal_fused_workspace_floats(int N, int Hd, int Wd) { return head_fused_workspace_floats(N, Hd, Wd); }

// include/mliis_loss.h.  ws = [N][tiles][4] partials, then coef [N][2] (the fold writes it; unused without a dice term).
int mliis_head_focal_fused(const float* small, const float* labels, const int* img_idx, int N, int Hd, int Wd, int H, int W,
                           float label_smoothing, float gamma, float fg_weight, float extra_loss, float* dsmall, float* out, float* ws,
                           size_t ws_floats, hipStream_t stream) {
  MLIIS_REQUIRE(small && labels && dsmall && out && ws, MLIIS_ERR_ARG, "head_focal_fused: null pointer");
  MLIIS_REQUIRE(N > 0 && Hd > 1 && Wd > 1 && H > 1 && W > 1 && N <= 65535 && (long long)H * W <= (1LL << 29) && Hd <= 32768 && Wd <= 32768,
                MLIIS_ERR_ARG, "head_focal_fused: bad shape (both maps must be larger than 1x1)");
  const int rc = check_scalars("head_focal_fused", label_smoothing, gamma, fg_weight);
  if (rc) return rc;
  MLIIS_REQUIRE(mliis_head_focal_fused_supported(Hd, Wd, H, W), MLIIS_ERR_UNSUPPORTED,
                "head_focal_fused: up-sampling factor too large for the tile footprint (mliis_head_focal_fused_supported)");
  MLIIS_REQUIRE(aligned8(small) && aligned8(labels) && aligned8(dsmall), MLIIS_ERR_ALIGN, "head_focal_fused: tensors must be 8-byte aligned");
  MLIIS_REQUIRE(ws_floats >= mliis_head_focal_fused_workspace_floats(N, Hd, Wd) && aligned16(ws), MLIIS_ERR_WORKSPACE,
                "head_focal_fused: workspace too small or unaligned (%zu floats given, %zu needed)", ws_floats,
                mliis_head_focal_fused_workspace_floats(N, Hd, Wd));
  const int tx = head_tiles(Wd), nblk = head_tiles(Hd) * tx;
  float* coef = ws + (size_t)N * nblk * 4;
  const float sh = (float)(Hd - 1) / (float)(H - 1), sw = (float)(Wd - 1) / (float)(W - 1);
  hipLaunchKernelGGL(head_focal_fused_k, dim3(nblk, N), dim3(256), 0, stream, small, labels, img_idx, N, Hd, Wd, H, W, sh, sw, label_smoothing,
                     gamma, fg_weight, 1.0f / ((float)N * (float)H * (float)W), dsmall, ws, tx);
  MLIIS_CHECK_LAUNCH("head_focal_fused");
  hipLaunchKernelGGL(focal_finalize_k, dim3(1), dim3(256), 0, stream, ws, nblk, N, H * W, 0, extra_loss, out, coef);
  MLIIS_CHECK_LAUNCH("head_focal_fused_finalize");
  return MLIIS_OK;
}
}
