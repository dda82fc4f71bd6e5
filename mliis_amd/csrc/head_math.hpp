// Per-pixel arithmetic of the decoder tail shared between translation units: the bilinear sample of head.hip's resize kernels and the
// two-class softmax of its loss kernels.  score.hip (libmliis_score.so) forms its prediction mask with these very functions, so the
// mask it counts is bit for bit the one head.hip's kernels write.
#pragma once
#include "common.hpp"

namespace mliis {

template <int V>
struct Vec;
template <>
struct Vec<4> {
  typedef float4 T;
};
template <>
struct Vec<2> {
  typedef float2 T;
};
__device__ __forceinline__ float4 vfma(float s, float4 a, float4 c) {
  return make_float4(fmaf(s, a.x, c.x), fmaf(s, a.y, c.y), fmaf(s, a.z, c.z), fmaf(s, a.w, c.w));
}
__device__ __forceinline__ float2 vfma(float s, float2 a, float2 c) { return make_float2(fmaf(s, a.x, c.x), fmaf(s, a.y, c.y)); }
template <class T>
__device__ __forceinline__ T vzero();
template <>
__device__ __forceinline__ float4 vzero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
template <>
__device__ __forceinline__ float2 vzero<float2>() { return make_float2(0.f, 0.f); }

// one output element of the resize: the four source elements around it (base = the image's channel window, row stride ldx) under the
// corner weights, accumulated in the order tl, tr, bl, br.  resize_fwd_k and mask_iou_counts_k share it: the mask the scoring kernel
// counts is bit for bit the one the resize launch followed by ce_grad_k writes.
template <class T>
__device__ __forceinline__ T bilinear_sample(const float* __restrict__ base, int Wi, int ldx, int y0, int y1, int x0, int x1, float ly, float lx) {
  const T tl = *reinterpret_cast<const T*>(base + ((long long)y0 * Wi + x0) * ldx);
  const T tr = *reinterpret_cast<const T*>(base + ((long long)y0 * Wi + x1) * ldx);
  const T bl = *reinterpret_cast<const T*>(base + ((long long)y1 * Wi + x0) * ldx);
  const T br = *reinterpret_cast<const T*>(base + ((long long)y1 * Wi + x1) * ldx);
  // top = tl + (tr - tl) * lx ; bottom likewise ; out = top + (bottom - top) * ly   (TF ResizeBilinear form)
  T o = vzero<T>();
  float wtl, wtr, wbl, wbr;
  bilinear_weights(ly, lx, wtl, wtr, wbl, wbr);
  o = vfma(wtl, tl, o);
  o = vfma(wtr, tr, o);
  o = vfma(wbl, bl, o);
  o = vfma(wbr, br, o);
  return o;
}
// the two class probabilities of one pixel as ce_grad_k forms them (its prediction mask is p > 0.5f of these): shared with
// mask_iou_counts_k
__device__ __forceinline__ void softmax2(float2 zz, float& p0, float& p1) {
  const float m = fmaxf(zz.x, zz.y);
  const float e0 = expf(zz.x - m), e1 = expf(zz.y - m);
  const float inv = 1.f / (e0 + e1);
  p0 = e0 * inv;
  p1 = e1 * inv;
}

}  // namespace mliis
