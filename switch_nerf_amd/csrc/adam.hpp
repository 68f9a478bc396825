// The per-element arithmetic of the optimiser kernels: ONE expression for swn_adam_step (elementwise.hip) and swn_adam_accum_step
// (accum.hip), so the two compile the same operations and agree bit for bit on the same inputs.
#pragma once
#include "common.hpp"

namespace swn {

// torch.optim.Adam on one element: g * gscale is the gradient, m / v the moments (updated in place); returns the new parameter.
// The three fused multiply-adds are written out and contraction is off inside, so the roundings do not depend on what the compiler
// fuses in the surrounding kernel (scalar loop or 4-wide body): they are the ones swn_adam_step has always made.
__device__ __forceinline__ float adam_update(float g, float gscale, float p, float& m, float& v, float lr, float b1, float b2, float eps,
                                             float bc1, float bc2s) {
#pragma clang fp contract(off)
  const float gi = g * gscale;
  const float mi = fmaf(b1, m, (1.f - b1) * gi);           // b1 m + (1 - b1) g
  const float vi = fmaf(b2, v, ((1.f - b2) * gi) * gi);    // b2 v + (1 - b2) g^2
  m = mi;
  v = vi;
  const float denom = sqrtf(vi) / bc2s + eps;  // torch.optim.Adam: (sqrt(v) / sqrt(bias_correction2)) + eps
  return fmaf(-(lr / bc1), mi / denom, p);                 // p - (lr / bias_correction1) m / denom
}

// acc + g * scale as two separately rounded fp32 operations (no FMA): the value is defined bit for bit, the same whether the sum is
// stored by swn_grad_accum or formed in registers by swn_adam_accum_step.
__device__ __forceinline__ float accum_add(float acc, float g, float scale) {
#pragma clang fp contract(off)
  const float prod = g * scale;
  return acc + prod;
}

}  // namespace swn
