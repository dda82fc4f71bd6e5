// libmliis_loss.so: the focal, foreground-weighted pixel loss of the inner loop (include/mliis_loss.h) -- the counterparts of head.hip's
// softmax cross-entropy (ce_partial_k / ce_finalize / ce_grad_k) and of its fused head (head_ce_fused_k) for a learner built with
// focal_gamma != 0 or fg_weight != 1.  A library of its own beside libmliis_hip.so, which (with its header) is not touched by it; it shares
// the resize geometry with head.hip through common.hpp / head_math.hpp, and the per-pixel loss arithmetic of its own kernels through
// focal_math.hpp.
#include "../../include/mliis_loss.h"
#include "common.hpp"
#include "head_math.hpp"
#include "focal_math.hpp"

namespace mliis {

// (this library's own error slot: common.hpp's MLIIS_REQUIRE / MLIIS_CHECK_LAUNCH report through set_error of the library they are linked into)
MLIIS_DEFINE_ERROR_SLOT(g_loss_err)

constexpr int kPartPixels = 256 * 8;   // image pixels per partial block (ce_partial_k's grid)
constexpr int kPartMaxBlocks = 256;    // at most this many partial blocks per image: the kernel grid-strides past it

// The four sums of a workgroup -> part[slot][0..3] = {sum l, sum p1 y1, sum p1, sum y1} (ce_partial_k's layout and order of addition).
__device__ __forceinline__ void store_partials(float l, float I, float Sp, float St, float (*sm)[4], float* __restrict__ dst) {
  l = wave_sum(l);
  I = wave_sum(I);
  Sp = wave_sum(Sp);
  St = wave_sum(St);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sm[wave][0] = l;
    sm[wave][1] = I;
    sm[wave][2] = Sp;
    sm[wave][3] = St;
  }
  __syncthreads();
  if (threadIdx.x < 4) dst[threadIdx.x] = sm[0][threadIdx.x] + sm[1][threadIdx.x] + sm[2][threadIdx.x] + sm[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void focal_partial_k(const float* __restrict__ logits, const float* __restrict__ labels,
                                                       const int* __restrict__ idx, int HW, float ls, float gamma, float fgw,
                                                       float* __restrict__ part) {
  __shared__ float sm[4][4];
  const int n = blockIdx.y;
  const int src = idx ? idx[n] : n;
  const float* z = logits + (long long)n * HW * 2;
  const float* t = labels + (long long)src * HW * 2;
  float l = 0.f, I = 0.f, Sp = 0.f, St = 0.f;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const float2 zz = *reinterpret_cast<const float2*>(z + (long long)p * 2);
    const float2 tt = *reinterpret_cast<const float2*>(t + (long long)p * 2);
    const FocalPixel px = focal_pixel(zz, tt, ls, gamma, fgw, 0.f);
    const float y1 = lone(tt.y);
    l += px.loss;
    I += px.p1 * y1;
    Sp += px.p1;
    St += y1;
  }
  store_partials(l, I, Sp, St, sm, part + ((long long)n * gridDim.x + blockIdx.x) * 4);
}

// out: [0] loss, [1] L_pix, [2] iou ; coef[n] = {A_n, B_n} for the dice gradient (0 when dice off).  head.hip's ce_finalize, restated for
// this library (that one is local to libmliis_hip.so): one block, 8 images at a time, 32 lanes per image fold that image's partial blocks
// in double precision, a lane butterfly finishes the image, thread 0 adds the images up in index order -- a fixed order: deterministic.
__device__ __forceinline__ void focal_finalize(const float* __restrict__ part, int nblk, int N, int HW, int dice, float extra_loss,
                                               float* __restrict__ out, float* __restrict__ coef) {
  __shared__ double s_l[8], s_iou[8];
  double l = 0.0, iou = 0.0;
  const double eps = 1e-7;
  const int g = threadIdx.x >> 5, lane = threadIdx.x & 31;
  for (int n0 = 0; n0 < N; n0 += 8) {
    const int n = n0 + g;
    double v[4] = {0, 0, 0, 0};
    if (n < N)
      for (int b = lane; b < nblk; b += 32) {
        const float4 q = ld4(part + ((long long)n * nblk + b) * 4);
        v[0] += q.x;
        v[1] += q.y;
        v[2] += q.z;
        v[3] += q.w;
      }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) v[k] += __shfl_xor(v[k], off);
    if (lane == 0 && n < N) {
      const double I = v[1], Sp = v[2], St = v[3];
      const double U = Sp + St - I;
      s_l[g] = v[0];
      s_iou[g] = (I + eps) / (U + eps);
      coef[2 * n + 0] = (float)(1.0 / (U + eps));
      coef[2 * n + 1] = (float)((I + eps) / ((U + eps) * (U + eps)));
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int j = 0; j < 8 && n0 + j < N; ++j) {
        l += s_l[j];
        iou += s_iou[j];
      }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  l /= (double)N * HW;
  iou /= N;
  double loss = l + extra_loss;
  double dLdiou = 0.0;
  if (dice) {
    loss -= log(2.0 * iou / (iou + 1.0));
    dLdiou = -1.0 / (iou * (iou + 1.0));
  }
  for (int n = 0; n < N; ++n) {
    coef[2 * n + 0] = (float)(coef[2 * n + 0] * dLdiou / N);
    coef[2 * n + 1] = (float)(coef[2 * n + 1] * dLdiou / N);
  }
  out[0] = (float)loss;
  out[1] = (float)l;
  out[2] = (float)iou;
}

__global__ __launch_bounds__(256) void focal_finalize_k(const float* __restrict__ part, int nblk, int N, int HW, int dice, float extra_loss,
                                                        float* __restrict__ out, float* __restrict__ coef) {
  focal_finalize(part, nblk, N, HW, dice, extra_loss, out, coef);
}

// fin_part != nullptr (no dice term: the gradient needs nothing from the fold): workgroup (0, 0) also folds the loss partials into out[]
// before its share of the gradient, as ce_grad_k does -- one launch fewer.  One pixel per thread.
__global__ __launch_bounds__(256) void focal_grad_k(const float* __restrict__ logits, const float* __restrict__ labels,
                                                    const int* __restrict__ idx, int HW, float ls, float gamma, float fgw, float inv_rows,
                                                    const float* __restrict__ coef, float* __restrict__ dlogits,
                                                    const float* __restrict__ fin_part, int fin_nblk, int N, float extra_loss,
                                                    float* __restrict__ fin_out, float* __restrict__ fin_coef) {
  if (fin_part != nullptr && blockIdx.x == 0 && blockIdx.y == 0) focal_finalize(fin_part, fin_nblk, N, HW, 0, extra_loss, fin_out, fin_coef);   // (uniform)
  const int n = blockIdx.y;
  const int src = idx ? idx[n] : n;
  const float* z = logits + (long long)n * HW * 2;
  const float* t = labels + (long long)src * HW * 2;
  const float An = fin_part != nullptr ? 0.f : coef[2 * n], Bn = fin_part != nullptr ? 0.f : coef[2 * n + 1];
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const float2 zz = *reinterpret_cast<const float2*>(z + (long long)p * 2);
    const float2 tt = *reinterpret_cast<const float2*>(t + (long long)p * 2);
    const FocalPixel px = focal_pixel(zz, tt, ls, gamma, fgw, inv_rows);
    const float y1 = lone(tt.y);
    const float d1 = px.d1 + (An * y1 - Bn * (1.f - y1)) * px.p1 * (1.f - px.p1);   // (the dice term's gradient, ce_grad_k's form)
    *reinterpret_cast<float2*>(dlogits + ((long long)n * HW + p) * 2) = make_float2(-d1, d1);
  }
}

// ------------------------------------------------------------------------------------------------ resize -> focal loss -> resize^T, one pass
// head.hip's head_ce_fused_k with focal_pixel() in place of the cross-entropy's arithmetic: the same 8 x 8 tiles of decoder pixels, the
// same footprint buffer (<= kHeadFoot^2 image pixels, 18 KB of LDS), the same owner rule for the loss terms (the tile that holds an image
// pixel's top-left source pixel), the same candidate walk in phase 2.  Loss partials per workgroup [n][tile][4], folded by focal_finalize_k.
constexpr int kHeadTile = 8, kHeadFoot = 48;
__device__ __forceinline__ int head_lo(int i, float s) {
  const int v = (int)floorf((float)(i - 1) / s) - 1;
  return v < 0 ? 0 : v;
}
__device__ __forceinline__ int head_hi(int i, float s, int n) {
  const int v = (int)ceilf((float)(i + 1) / s) + 1;
  return v > n - 1 ? n - 1 : v;
}
__global__ __launch_bounds__(256) void head_focal_fused_k(const float* __restrict__ small, const float* __restrict__ labels,
                                                          const int* __restrict__ idx, int N, int Hi, int Wi, int Ho, int Wo, float sh, float sw,
                                                          float ls, float gamma, float fgw, float inv_rows, float* __restrict__ dsmall,
                                                          float* __restrict__ part, int tiles_x) {
  __shared__ float2 gl[kHeadFoot * kHeadFoot];
  __shared__ float sm[4][4];
  const int t = threadIdx.x;
  const int n = blockIdx.y;
  const int src = idx ? idx[n] : n;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int hi0 = ty * kHeadTile, wi0 = tx * kHeadTile;
  const int hi1 = hi0 + kHeadTile - 1 < Hi - 1 ? hi0 + kHeadTile - 1 : Hi - 1;
  const int wi1 = wi0 + kHeadTile - 1 < Wi - 1 ? wi0 + kHeadTile - 1 : Wi - 1;
  const int fo0 = head_lo(hi0, sh), fo1 = head_hi(hi1, sh, Ho), fw0 = head_lo(wi0, sw), fw1 = head_hi(wi1, sw, Wo);
  const int FH = fo1 - fo0 + 1, FW = fw1 - fw0 + 1;   // (host: <= kHeadFoot)
  const float* zb = small + (long long)n * Hi * Wi * 2;
  const float* tb = labels + (long long)src * Ho * Wo * 2;
  float l = 0.f, I = 0.f, Sp = 0.f, St = 0.f;
  for (int p = t; p < FH * FW; p += 256) {
    const int fr = p / FW, fc = p - fr * FW;
    const int ho = fo0 + fr, wo = fw0 + fc;
    int y0, y1, x0, x1;
    float ly, lx;
    src_coord(ho, sh, Hi, y0, y1, ly);
    src_coord(wo, sw, Wi, x0, x1, lx);
    const float2 zz = bilinear_sample<float2>(zb, Wi, 2, y0, y1, x0, x1, ly, lx);   // (resize_fwd_k's arithmetic)
    const float2 tt = *reinterpret_cast<const float2*>(tb + ((long long)ho * Wo + wo) * 2);
    const FocalPixel px = focal_pixel(zz, tt, ls, gamma, fgw, inv_rows);
    gl[fr * kHeadFoot + fc] = make_float2(-px.d1, px.d1);
    if (y0 >= hi0 && y0 <= hi1 && x0 >= wi0 && x0 <= wi1) {   // this tile owns the image pixel's loss terms
      const float yy = lone(tt.y);
      l += px.loss;
      I += px.p1 * yy;
      Sp += px.p1;
      St += yy;
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int pg = (t >> 3) + 32 * it, rl = t & 7;
    const int hi = hi0 + pg / kHeadTile, wi = wi0 + pg % kHeadTile;
    const bool live = hi <= hi1 && wi <= wi1;
    const int hc = live ? hi : hi0, wc = live ? wi : wi0;
    const int ho_lo = head_lo(hc, sh), ho_hi = head_hi(hc, sh, Ho), wo_lo = head_lo(wc, sw), wo_hi = head_hi(wc, sw, Wo);
    float2 acc = make_float2(0.f, 0.f);
    for (int ho = ho_lo + rl; ho <= ho_hi; ho += 8) {
      int y0, y1;
      float ly;
      src_coord(ho, sh, Hi, y0, y1, ly);
      const float wy = (y0 == hc ? 1.f - ly : 0.f) + (y1 == hc ? ly : 0.f);
      if (wy == 0.f) continue;
      const float2* row = gl + (ho - fo0) * kHeadFoot - fw0;
      for (int wo = wo_lo; wo <= wo_hi; ++wo) {
        int x0, x1;
        float lx;
        src_coord(wo, sw, Wi, x0, x1, lx);
        const float wx = (x0 == wc ? 1.f - lx : 0.f) + (x1 == wc ? lx : 0.f);
        acc = vfma(wy * wx, row[wo], acc);
      }
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {
      acc.x += __shfl_xor(acc.x, off);
      acc.y += __shfl_xor(acc.y, off);
    }
    if (live && rl == 0) *reinterpret_cast<float2*>(dsmall + ((long long)n * Hi * Wi + (long long)hi * Wi + wi) * 2) = acc;
  }
  store_partials(l, I, Sp, St, sm, part + ((long long)n * gridDim.x + blockIdx.x) * 4);
}

static inline int head_tiles(int n) { return (n + kHeadTile - 1) / kHeadTile; }
static inline int part_blocks(long long HW) {
  const int nblk = ceil_div(HW, kPartPixels);
  return nblk > kPartMaxBlocks ? kPartMaxBlocks : nblk;
}
static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

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

size_t mliis_focal_ce_workspace_floats(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * part_blocks((long long)H * W) * 4 + 2 * (size_t)N + 8;
}

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

// (mliis_head_ce_fused_supported's predicate: the image-side footprint of an 8 x 8 tile of the decoder's map fits the LDS buffer)
int mliis_head_focal_fused_supported(int Hd, int Wd, int H, int W) {
  if (Hd <= 1 || Wd <= 1 || H <= 1 || W <= 1) return 0;
  const float sh = (float)(Hd - 1) / (float)(H - 1), sw = (float)(Wd - 1) / (float)(W - 1);
  const int fh = (int)ceilf((float)(kHeadTile + 1) / sh) + 5, fw = (int)ceilf((float)(kHeadTile + 1) / sw) + 5;
  return fh <= kHeadFoot && fw <= kHeadFoot;
}

size_t mliis_head_focal_fused_workspace_floats(int N, int Hd, int Wd) {
  if (N <= 0 || Hd <= 0 || Wd <= 0) return 0;
  return (size_t)N * head_tiles(Hd) * head_tiles(Wd) * 4 + 2 * (size_t)N + 8;
}

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
