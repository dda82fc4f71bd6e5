// The pixel-loss kernels of the decoder tail, once for every loss: the geometry of the partial-sum grid and of the fused head's tiles, the
// workspace sizes, the fold of the loss partials, and the three kernel bodies -- partial sums, gradient, fused head tile -- as templates
// over a per-pixel policy.  head.hip (softmax cross-entropy: CePixel, libmliis_hip.so) and focal.hip (the focal, foreground-weighted loss:
// FocalPixel of focal_math.hpp, libmliis_loss.so) instantiate them behind their own __global__ kernels and entry points.  tversky.hip (the
// Tversky region term, libmliis_region.so) runs the same bodies through their hooks: a region term for the fold (JaccardRegion is the
// default: the soft IoU's dice term), a region gradient for the gradient pass and the fused head's tiles (JaccardGrad / NoRegion), and a
// logits source for the partial-sum pass (LoadedLogits).
//
// A policy is a small struct of the loss's scalars, passed by value.  Per pixel, from the two logits zz and the two stored labels tt:
//   auto a = px.at(zz, tt);             what the pixel's gradient and loss terms share, with the softmax pair a.p0, a.p1
//   float2 g = px.grad(a);              d(loss / (N H W)) / d(z0, z1) without the dice term
//   g = px.with_dice(g, dp1);           the dice term's d / dz1 added to that pair (the gradient pass only; dp1 is 0 without the term)
//   px.terms(a, l, I, Sp, St);          adds the pixel's {loss term, p1 y1, p1, y1} to the four sums
#pragma once
#include <type_traits>

#include "common.hpp"
#include "head_math.hpp"

namespace mliis {

// ------------------------------------------------------------------------------------------------ geometry (host and device)
constexpr int kPartPixels = 256 * 8;   // image pixels per partial block of the partial-sum pass
constexpr int kPartMaxBlocks = 256;    // at most this many partial blocks per image: the kernel grid-strides past it
static inline int part_blocks(long long HW) {
  int nblk = ceil_div(HW, kPartPixels);
  if (nblk > kPartMaxBlocks) nblk = kPartMaxBlocks;
  return nblk;
}
// the fused head: 8 x 8 tiles of decoder pixels, an LDS buffer of kHeadFoot^2 image pixels for a tile's footprint; head_lo / head_hi are
// the conservative candidate range of image rows (columns) that can touch decoder row (column) i -- resize_bwd_k's
constexpr int kHeadTile = 8, kHeadFoot = 48;
__device__ __forceinline__ int head_lo(int i, float s) {
  const int v = (int)floorf((float)(i - 1) / s) - 1;
  return v < 0 ? 0 : v;
}
__device__ __forceinline__ int head_hi(int i, float s, int n) {
  const int v = (int)ceilf((float)(i + 1) / s) + 1;
  return v > n - 1 ? n - 1 : v;
}
static inline int head_tiles(int n) { return (n + kHeadTile - 1) / kHeadTile; }
static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// 1 when the fused head takes this pair of maps: the image-side footprint of an 8 x 8 tile of the decoder's map fits the LDS buffer
// (up-sampling factors up to ~4.5).  This bound is what keeps phase 1 of head_fused_tile inside gl[].
static inline int head_fused_supported(int Hd, int Wd, int H, int W) {
  if (Hd <= 1 || Wd <= 1 || H <= 1 || W <= 1) return 0;
  const float sh = (float)(Hd - 1) / (float)(H - 1), sw = (float)(Wd - 1) / (float)(W - 1);
  const int fh = (int)ceilf((float)(kHeadTile + 1) / sh) + 5, fw = (int)ceilf((float)(kHeadTile + 1) / sw) + 5;
  return fh <= kHeadFoot && fw <= kHeadFoot;
}
// workspaces: [N][nblk][4] partials, then coef [N][2], and 8 floats of slack
static inline size_t loss_workspace_floats(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  const int nblk = part_blocks((long long)H * W);
  return (size_t)N * nblk * 4 + 2 * (size_t)N + 8;
}
static inline size_t head_fused_workspace_floats(int N, int Hd, int Wd) {
  if (N <= 0 || Hd <= 0 || Wd <= 0) return 0;
  return (size_t)N * head_tiles(Hd) * head_tiles(Wd) * 4 + 2 * (size_t)N + 8;
}

// ------------------------------------------------------------------------------------------------ partials and their fold
// The four sums of a workgroup -> dst[0..3] = {sum loss term, sum p1 y1, sum p1, sum y1}: lanes, then the four waves in index order.
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

// The region term of the fold.  image(): from an image's three sums, its index T_n (returned: the term is -ln(2 T / (T + 1)) on the batch
// mean T) and, into coef[n], the pair {1 / D_n, (I + eps) / D_n^2} of its denominator that the fold scales by (dL/dT) / N into coef[n].  kIndices = 1: T_n is the
// soft IoU that out[2] reports anyway; 2: the fold keeps the two means apart.  JaccardRegion is the dice term of the reference.
struct JaccardRegion {
  static constexpr int kIndices = 1;
  int on;
  __device__ __forceinline__ double image(double I, double Sp, double St, double iou_n, float* __restrict__ coef, int n) const {
    const double eps = 1e-7;
    const double U = Sp + St - I;
    coef[2 * n + 0] = (float)(1.0 / (U + eps));
    coef[2 * n + 1] = (float)((I + eps) / ((U + eps) * (U + eps)));
    return iou_n;
  }
};

// out: [0] loss, [1] pixel loss, [2] iou ; coef[n] = {A_n, B_n} for the region gradient (0 when the term is off).  One block: 8 images at
// a time, 32 lanes per image fold that image's partial blocks (double precision), a lane butterfly finishes the image, thread 0 adds the
// images up in index order (fixed order: deterministic).
template <class Region>
__device__ __forceinline__ void loss_fold_with(Region rg, const float* __restrict__ part, int nblk, int N, int HW, float extra_loss,
                                               float* __restrict__ out, float* __restrict__ coef) {
  __shared__ double s_l[8], s_iou[8 * Region::kIndices];
  double l = 0.0, iou = 0.0, tv = 0.0;
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
      const double T = rg.image(I, Sp, St, (I + eps) / (U + eps), coef, n);
      if constexpr (Region::kIndices == 2) s_iou[8 + g] = T;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int j = 0; j < 8 && n0 + j < N; ++j) {
        l += s_l[j];
        iou += s_iou[j];
        if constexpr (Region::kIndices == 2) tv += s_iou[8 + j];
      }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  l /= (double)N * HW;
  iou /= N;
  const double T = Region::kIndices == 2 ? tv / N : iou;
  double loss = l + extra_loss;
  double dLdT = 0.0;
  if (rg.on) {
    loss -= log(2.0 * T / (T + 1.0));
    dLdT = -1.0 / (T * (T + 1.0));
  }
  for (int n = 0; n < N; ++n) {
    coef[2 * n + 0] = (float)(coef[2 * n + 0] * dLdT / N);
    coef[2 * n + 1] = (float)(coef[2 * n + 1] * dLdT / N);
  }
  out[0] = (float)loss;
  out[1] = (float)l;
  out[2] = (float)iou;
}
__device__ __forceinline__ void loss_fold(const float* __restrict__ part, int nblk, int N, int HW, int dice, float extra_loss,
                                          float* __restrict__ out, float* __restrict__ coef) {
  loss_fold_with(JaccardRegion{dice}, part, nblk, N, HW, extra_loss, out, coef);
}

// ------------------------------------------------------------------------------------------------ the chain: partial sums, gradient
// part layout [n][blk][4] (store_partials); grid (part_blocks(HW), N).  The logits of image n's pixel p come from a source: LoadedLogits reads
// them, a caller's own source may form them (tversky.hip rebuilds them from the decoder's map).
struct LoadedLogits {
  const float* logits;   // [N][HW][2]
  int HW;
  struct Image {
    const float* z;
    __device__ __forceinline__ float2 operator()(int p) const { return *reinterpret_cast<const float2*>(z + (long long)p * 2); }
  };
  __device__ __forceinline__ Image image(int n) const { return Image{logits + (long long)n * HW * 2}; }
};
template <class Pixel, class Logits>
__device__ __forceinline__ void loss_partial_from(Pixel px, Logits zsrc, const float* __restrict__ labels, const int* __restrict__ idx, int HW,
                                                  float* __restrict__ part) {
  __shared__ float sm[4][4];
  const int n = blockIdx.y;
  const int src = idx ? idx[n] : n;
  const auto z = zsrc.image(n);
  const float* t = labels + (long long)src * HW * 2;
  const unsigned nblk = gridDim.x;
  float l = 0.f, I = 0.f, Sp = 0.f, St = 0.f;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += nblk * 256) {
    const float2 zz = z(p);
    const float2 tt = *reinterpret_cast<const float2*>(t + (long long)p * 2);
    px.terms(px.at(zz, tt), l, I, Sp, St);
  }
  store_partials(l, I, Sp, St, sm, part + ((long long)n * nblk + blockIdx.x) * 4);
}
template <class Pixel>
__device__ __forceinline__ void loss_partial(Pixel px, const float* __restrict__ logits, const float* __restrict__ labels,
                                             const int* __restrict__ idx, int HW, float* __restrict__ part) {
  loss_partial_from(px, LoadedLogits{logits, HW}, labels, idx, HW, part);
}

// The region term's d / dz1 at a pixel from the image's pair coef[n] = {An, Bn} (the fold's), the stored foreground label and p1.
// A functor float(An, Bn, y1, p1).  JaccardGrad names the dice term's, which loss_grad spells itself (through a functor the compiler
// schedules focal_grad_k's instructions in another order); NoRegion marks a fused head without a region term (its tiles add the loss
// terms instead).
struct JaccardGrad {};
struct NoRegion {};

// dlogits (nullable) = the pixel's gradient with the dice term's (coef, from the fold); pred (nullable) = (softmax > 0.5) as float.
// fin_part != nullptr (no dice term: the gradient needs nothing from the fold): workgroup (0, 0) also folds the loss partials into
// fin_out[] before its share of the gradient -- one launch fewer than partial -> fold -> gradient.  One pixel per thread.
template <class Pixel, class RegionGrad = JaccardGrad>
__device__ __forceinline__ void loss_grad(Pixel px, const float* __restrict__ logits, const float* __restrict__ labels,
                                          const int* __restrict__ idx, int HW, const float* __restrict__ coef, float* __restrict__ dlogits,
                                          float* __restrict__ pred, const float* __restrict__ fin_part, int fin_nblk, int N, float extra_loss,
                                          float* __restrict__ fin_out, float* __restrict__ fin_coef, RegionGrad region = RegionGrad{}) {
  if (fin_part != nullptr && blockIdx.x == 0 && blockIdx.y == 0) loss_fold(fin_part, fin_nblk, N, HW, 0, extra_loss, fin_out, fin_coef);   // (uniform)
  const int n = blockIdx.y;
  const int src = idx ? idx[n] : n;
  const float* z = logits + (long long)n * HW * 2;
  const float* t = labels + (long long)src * HW * 2;
  const float An = fin_part != nullptr ? 0.f : coef[2 * n], Bn = fin_part != nullptr ? 0.f : coef[2 * n + 1];
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const float2 zz = *reinterpret_cast<const float2*>(z + (long long)p * 2);
    const float2 tt = *reinterpret_cast<const float2*>(t + (long long)p * 2);
    const auto a = px.at(zz, tt);
    float dp1;
    if constexpr (std::is_same<RegionGrad, JaccardGrad>::value)
      dp1 = (An * tt.y - Bn * (1.f - tt.y)) * a.p1 * (1.f - a.p1);
    else
      dp1 = region(An, Bn, tt.y, a.p1);
    const float2 g = px.with_dice(px.grad(a), dp1);
    if (dlogits) *reinterpret_cast<float2*>(dlogits + ((long long)n * HW + p) * 2) = g;
    if (pred) *reinterpret_cast<float2*>(pred + ((long long)n * HW + p) * 2) = make_float2(a.p0 > 0.5f ? 1.f : 0.f, a.p1 > 0.5f ? 1.f : 0.f);
  }
}

// ------------------------------------------------------------------------------------------------ resize -> pixel loss -> resize^T, one pass
// The tail of a training step without the dice term: logits = resize(small) (models/efficientlab.py:166-173), the per-pixel loss
// (:294-303), its gradient / (N H W) -- which needs no global sum -- and the transpose of the resize back to the decoder's map.
// A workgroup owns an 8 x 8 tile of DECODER pixels:
//   phase 1: every image pixel that a pixel of the tile reaches (the tile's footprint, <= kHeadFoot^2 pixels) gets its logits rebuilt
//            from the four decoder pixels around it (resize_fwd_k's arithmetic) and its gradient formed (the gradient pass's arithmetic)
//            into LDS; the loss terms of an image pixel are added by the tile that holds its top-left source pixel (one owner each);
//   phase 2: the 8 lanes of a decoder pixel walk its candidates exactly as resize_bwd_k does, reading the gradients from LDS.
// The full-resolution logits / gradient tensors are never written (four launches and 4 x 3.2 MB of traffic at 224x224, N = 8, become
// two).  Loss partials per workgroup [n][tile][4] as the partial-sum pass's, folded by loss_fold -- a launch of its own (or a ride in
// the final conv's backward-data launch): a last-arriver fold inside this kernel needs device-scope fences, which on this eight-L2 part
// write back and invalidate a whole L2 each (measured: 39 us for the launch, more than the four it replaces).  (A first form without
// the LDS phase -- every decoder pixel rebuilding its ~100 candidates itself -- took 69 us: one dependent load chain per candidate.)
// grid (head_tiles(Hi) * tiles_x, N); the host admits only maps with head_fused_supported(Hi, Wi, Ho, Wo).
// With a region gradient (Region != NoRegion: the second pass of a two-pass head, after the sums and their fold) phase 1 adds the region
// term's d / dz1 from coef[n] to the entry and no loss terms are formed; part is not written.
template <class Pixel, class Region = NoRegion>
__device__ __forceinline__ void head_fused_tile(Pixel px, const float* __restrict__ small, const float* __restrict__ labels,
                                                const int* __restrict__ idx, int Hi, int Wi, int Ho, int Wo, float sh, float sw,
                                                float* __restrict__ dsmall, float* __restrict__ part, int tiles_x,
                                                const float* __restrict__ coef = nullptr, Region region = Region{}) {
  constexpr bool kRegion = !std::is_same<Region, NoRegion>::value;
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
    const auto a = px.at(zz, tt);
    if constexpr (kRegion) {
      gl[fr * kHeadFoot + fc] = px.with_dice(px.grad(a), region(coef[2 * n], coef[2 * n + 1], tt.y, a.p1));
    } else {
      gl[fr * kHeadFoot + fc] = px.grad(a);
      if (y0 >= hi0 && y0 <= hi1 && x0 >= wi0 && x0 <= wi1) px.terms(a, l, I, Sp, St);   // this tile owns the image pixel's loss terms
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
  if constexpr (!kRegion) store_partials(l, I, Sp, St, sm, part + ((long long)n * gridDim.x + blockIdx.x) * 4);
}

}  // namespace mliis
