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

// The loop of swn_adam_step over [0, n), one element per thread and pass - the body of the unguarded kernel (elementwise.hip) and of
// the guarded one (finite_guard.hip): ONE text, so the two cannot drift apart.
template <typename T>
__device__ __forceinline__ void adam_range(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                           T* __restrict__ shadow, long n, float lr, float b1, float b2, float eps, float bc1, float bc2s,
                                           float gscale) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float mi = m[i], vi = v[i];
    const float pi = adam_update(g[i], gscale, p[i], mi, vi, lr, b1, b2, eps, bc1, bc2s);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
    if (shadow) ElemIO<T>::st(shadow + i, pi);
  }
}

// acc + g * scale as two separately rounded fp32 operations (no FMA): the value is defined bit for bit, the same whether the sum is
// stored by swn_grad_accum or formed in registers by swn_adam_accum_step.
__device__ __forceinline__ float accum_add(float acc, float g, float scale) {
#pragma clang fp contract(off)
  const float prod = g * scale;
  return acc + prod;
}

// ---- the finite guard's side of an optimiser launch (finite_guard.hip, accum.hip: the *_guarded entry points) ----
// A guarded launch reads the step's flag ok[0] (swn_finite_guard) and, because a skipped step must not advance Adam's bias correction,
// takes the step count from the device: state[0] = optimizer steps taken so far, state[1] = workgroups of the running launch that have
// finished (0 between launches).  The bias corrections of step t come from a table the host filled with swn_adam_step's own
// expressions (swn_adam_bias_table): the same bits as the unguarded launch, which the device's powf would not give.
struct GuardArgs {
  const int* ok;         // [1]
  int* state;            // [2]
  const float* table;    // [table_n][2] = {bc1, bc2s} of step 1 .. table_n; the last row holds for every later step
  long table_n;
};

// Once per workgroup: thread 0 reads the flag, the step count and the step's bias corrections, LDS hands them to the others.
// -> ok; t = the step this launch takes.  ok is the same for every workgroup of the launch.
__device__ __forceinline__ bool guard_begin(const GuardArgs& ga, float& bc1, float& bc2s, int& t) {
  __shared__ int s_ok, s_t;
  __shared__ float s_bc[2];
  if (threadIdx.x == 0) {
    const int ok = ga.ok[0];
    s_ok = ok;
    if (ok) {
      const int step = ga.state[0] + 1;
      long row = ((long)step < ga.table_n ? (long)step : ga.table_n) - 1;
      if (row < 0) row = 0;              // (a count below 0 cannot come from these launches; never index in front of the table)
      s_t = step;
      s_bc[0] = ga.table[2 * row];
      s_bc[1] = ga.table[2 * row + 1];
    }
  }
  __syncthreads();
  if (!s_ok) return false;
  bc1 = s_bc[0];
  bc2s = s_bc[1];
  t = s_t;
  return true;
}

// Behind a workgroup's last element of a step that was taken: the workgroup that finishes last stores the new step count and puts the
// counter back to 0 for the next launch.  No fence: no workgroup reads another's data.  The one order needed - every workgroup's read
// of the old count in front of the last one's store - holds because thread 0 has consumed that read (it went through LDS in
// guard_begin) before it issues its atomic, and the store waits for the value the last atomic returns.  (A device-scope release here
// would be an L2 write-back per workgroup, 4096 per launch.)
__device__ __forceinline__ void guard_end(const GuardArgs& ga, int t) {
  __syncthreads();
  if (threadIdx.x == 0) {
    if (atomicAdd(ga.state + 1, 1) == (int)gridDim.x - 1) {
      ga.state[0] = t;
      ga.state[1] = 0;
    }
  }
}

}  // namespace swn
