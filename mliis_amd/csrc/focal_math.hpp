// Per-pixel arithmetic of the focal, foreground-weighted pixel loss (include/mliis_loss.h): the loss term and its gradient from the two
// logits and the two stored labels, and FocalPixel, the policy that hands them to the kernel bodies of loss_kernels.hpp.  focal.hip's
// chain kernels (focal_partial_k, focal_grad_k) and its fused head (head_focal_fused_k) all reach this one function through it, so the
// fused head and the chain form the same values per pixel.
#pragma once
#include "common.hpp"

namespace mliis {

struct FocalTerms {
  float loss;     // l: the pixel's loss term, NOT yet divided by N H W (the fold divides the sum in double)
  float d1;       // d(l * inv_rows) / dz1; the gradient w.r.t. z0 is -d1
  float p0, p1;   // the softmax pair (p1: the soft IoU's sums, the dice gradient)
  float y1;       // the stored foreground label, alone (the soft IoU's sums)
};

// z = (z0, z1), y = (y0, y1); t_c = y_c (1 - ls) + ls / 2; w = 1 + (fgw - 1) y1; (l0, l1) = log_softmax(z) through m + logf(e0 + e1) as
// ce_partial_k forms it.  (1 - p_c)^gamma = exp(gamma * l_other): no powf, no 1 - p, no log(p) -- at |z0 - z1| ~ 180 every factor is a
// finite number times an exponential that has gone to zero.  exp((gamma + 1) l) is the product exp(gamma l) * p of two values the pixel
// has already.  Contraction is off inside: the products and sums below are the same roundings wherever the function is inlined.
// The halves of the two float2 operands pass through lone() (common.hpp): each is used alone from here on.
__device__ __forceinline__ FocalTerms focal_pixel(float2 zz, float2 tt, float ls, float gamma, float fgw, float inv_rows) {
#pragma clang fp contract(off)
  const float z0 = lone(zz.x), z1 = lone(zz.y), y0 = lone(tt.x), y1 = lone(tt.y);
  const float m = fmaxf(z0, z1);
  const float e0 = expf(z0 - m), e1 = expf(z1 - m);
  const float s = e0 + e1;
  const float lse = m + logf(s);
  const float l0 = z0 - lse, l1 = z1 - lse;
  const float inv = 1.f / s;
  const float p0 = e0 * inv, p1 = e1 * inv;
  const float t0 = y0 * (1.f - ls) + 0.5f * ls, t1 = y1 * (1.f - ls) + 0.5f * ls;
  const float w = 1.f + (fgw - 1.f) * y1;
  const float f0 = expf(gamma * l1), f1 = expf(gamma * l0);   // class 0 is modulated by p1^gamma, class 1 by p0^gamma
  FocalTerms r;
  r.loss = -w * (t0 * (f0 * l0) + t1 * (f1 * l1));
  const float g1 = t1 * (gamma * (f1 * l1) * p1 - f1 * p0);
  const float g0 = t0 * (gamma * (f0 * l0) * p0 - f0 * p1);
  r.d1 = w * (g1 - g0) * inv_rows;
  r.p0 = p0;
  r.p1 = p1;
  r.y1 = y1;
  return r;
}

// the per-pixel policy of loss_kernels.hpp's kernel bodies (a partial-sum pass, which asks for no gradient, builds it with inv_rows = 0)
struct FocalPixel {
  float ls, gamma, fgw, inv_rows;
  __device__ __forceinline__ FocalTerms at(float2 zz, float2 tt) const { return focal_pixel(zz, tt, ls, gamma, fgw, inv_rows); }
  __device__ __forceinline__ float2 grad(const FocalTerms& a) const { return make_float2(-a.d1, a.d1); }
  __device__ __forceinline__ float2 with_dice(float2 g, float dp1) const {   // (the pair stays (-d1, d1), a zero's sign included)
    const float d1 = g.y + dp1;
    return make_float2(-d1, d1);
  }
  __device__ __forceinline__ void terms(const FocalTerms& a, float& l, float& I, float& Sp, float& St) const {
    l += a.loss;
    I += a.p1 * a.y1;
    Sp += a.p1;
    St += a.y1;
  }
};

}  // namespace mliis
