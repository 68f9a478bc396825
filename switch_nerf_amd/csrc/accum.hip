// Gradient accumulation (the reference's --accumulation_steps, runner.py:677-690): the add of one micro-step's gradient into the
// window's fp32 buffer, and the window's last micro-step fused with the Adam update.  Both are streaming kernels: 256 threads,
// grid-stride over 16-byte pieces of the aligned body, the few elements before and after it one by one; no atomics, no LDS.
#include "adam.hpp"

namespace swn {

// Where the 16-byte body of n floats begins (head elements before it) and how many 4-float pieces it has.  Every buffer of a call is
// walked with the same element index, so the body is 16-byte aligned in all of them only when they share their offset inside a 16-byte
// line (the flat buffers of a model sliced at the same element do); otherwise the whole range goes one element at a time.
struct AccumSplit {
  long head, nvec;
};
static AccumSplit accum_split(long n, const void* const* f32, int n_f32, const void* shadow, int shadow_esz) {
  const long head = (long)(((16 - (uintptr_t)f32[0] % 16) % 16) / 4);
  bool ok = n >= head + 4;
  for (int i = 0; i < n_f32 && ok; ++i) ok = f32[i] == nullptr || ((uintptr_t)f32[i] + head * 4) % 16 == 0;
  if (ok && shadow) ok = ((uintptr_t)shadow + head * shadow_esz) % (4 * shadow_esz) == 0;
  if (!ok) return {0, 0};
  return {head, (n - head) / 4};
}
static int accum_blocks(long n, const AccumSplit& s) {
  const long edge = n - 4 * s.nvec, items = s.nvec > edge ? s.nvec : edge;
  int blocks = cdiv(items, 256);
  return blocks > 4096 ? 4096 : blocks;   // (the cap of swn_adam_step)
}
// element index of edge item j: the head first, then what follows the body
__device__ __forceinline__ long edge_index(long j, long head, long nvec) { return j < head ? j : j + 4 * nvec; }

__device__ __forceinline__ void store4(float* p, const float4& v) { *(float4*)p = v; }
__device__ __forceinline__ void store4(bf16_t* p, const float4& v) { *(uint2*)p = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)); }

__global__ __launch_bounds__(256) void grad_accum_kernel(float* __restrict__ acc, const float* __restrict__ g, long n, long head, long nvec,
                                                         float scale) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  for (long i = tid; i < nvec; i += stride) {
    const long e = head + 4 * i;
    const float4 a = *(const float4*)(acc + e), b = *(const float4*)(g + e);
    *(float4*)(acc + e) = make_float4(accum_add(a.x, b.x, scale), accum_add(a.y, b.y, scale), accum_add(a.z, b.z, scale),
                                      accum_add(a.w, b.w, scale));
  }
  for (long j = tid; j < n - 4 * nvec; j += stride) {
    const long e = edge_index(j, head, nvec);
    acc[e] = accum_add(acc[e], g[e], scale);
  }
}

// swn_grad_accum under the finite guard: a flagged micro-step contributes nothing and clears the window's partial sums (zero_grad)
__global__ __launch_bounds__(256) void grad_accum_guarded_kernel(float* __restrict__ acc, const float* __restrict__ g, long n, long head,
                                                                 long nvec, float scale, const int* __restrict__ ok) {
  __shared__ int s_ok;
  if (threadIdx.x == 0) s_ok = ok[0];
  __syncthreads();
  const bool add = s_ok != 0;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  for (long i = tid; i < nvec; i += stride) {
    const long e = head + 4 * i;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (add) {
      const float4 a = *(const float4*)(acc + e), b = *(const float4*)(g + e);
      r = make_float4(accum_add(a.x, b.x, scale), accum_add(a.y, b.y, scale), accum_add(a.z, b.z, scale), accum_add(a.w, b.w, scale));
    }
    *(float4*)(acc + e) = r;
  }
  for (long j = tid; j < n - 4 * nvec; j += stride) {
    const long e = edge_index(j, head, nvec);
    acc[e] = add ? accum_add(acc[e], g[e], scale) : 0.f;
  }
}

struct AdamArgs {
  float lr, b1, b2, eps, bc1, bc2s, gscale, ascale;
};

// one element of the fused last micro-step: the window's total, the Adam update on it, the buffer cleared
template <bool HAS_GRAD>
__device__ __forceinline__ float adam_accum_one(float a, float g, float p, float& m, float& v, const AdamArgs& c) {
  const float total = HAS_GRAD ? accum_add(a, g, c.ascale) : a;
  return adam_update(total, c.gscale, p, m, v, c.lr, c.b1, c.b2, c.eps, c.bc1, c.bc2s);
}

// The fused last micro-step over [0, n): 16-byte pieces on the aligned body, single elements around it.  The body of the unguarded
// kernel and of the guarded one below: ONE text for both.
template <typename T, bool HAS_GRAD>
__device__ __forceinline__ void adam_accum_range(float* __restrict__ p, float* __restrict__ acc, const float* __restrict__ g,
                                                 float* __restrict__ m, float* __restrict__ v, T* __restrict__ shadow, long n, long head,
                                                 long nvec, const AdamArgs& c) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  for (long i = tid; i < nvec; i += stride) {
    const long e = head + 4 * i;
    const float4 a = *(const float4*)(acc + e), pi = *(const float4*)(p + e);
    float4 mi = *(const float4*)(m + e), vi = *(const float4*)(v + e), gi = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (HAS_GRAD) gi = *(const float4*)(g + e);
    float4 po;
    po.x = adam_accum_one<HAS_GRAD>(a.x, gi.x, pi.x, mi.x, vi.x, c);
    po.y = adam_accum_one<HAS_GRAD>(a.y, gi.y, pi.y, mi.y, vi.y, c);
    po.z = adam_accum_one<HAS_GRAD>(a.z, gi.z, pi.z, mi.z, vi.z, c);
    po.w = adam_accum_one<HAS_GRAD>(a.w, gi.w, pi.w, mi.w, vi.w, c);
    *(float4*)(m + e) = mi;
    *(float4*)(v + e) = vi;
    *(float4*)(p + e) = po;
    *(float4*)(acc + e) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (shadow) store4(shadow + e, po);
  }
  for (long j = tid; j < n - 4 * nvec; j += stride) {
    const long e = edge_index(j, head, nvec);
    float mi = m[e], vi = v[e];
    const float po = adam_accum_one<HAS_GRAD>(acc[e], HAS_GRAD ? g[e] : 0.f, p[e], mi, vi, c);
    m[e] = mi;
    v[e] = vi;
    p[e] = po;
    acc[e] = 0.f;
    if (shadow) ElemIO<T>::st(shadow + e, po);
  }
}

template <typename T, bool HAS_GRAD>
__global__ __launch_bounds__(256) void adam_accum_kernel(float* __restrict__ p, float* __restrict__ acc, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, T* __restrict__ shadow, long n,
                                                         long head, long nvec, AdamArgs c) {
  adam_accum_range<T, HAS_GRAD>(p, acc, g, m, v, shadow, n, head, nvec, c);
}

// adam_accum_kernel under the finite guard.  ok: the same loops with the step count and bias corrections read on the device.  A
// skipped step is a store-only pass that clears acc - what a taken step leaves behind - and touches nothing else.
template <typename T, bool HAS_GRAD>
__global__ __launch_bounds__(256) void adam_accum_guarded_kernel(float* __restrict__ p, float* __restrict__ acc, const float* __restrict__ g,
                                                                 float* __restrict__ m, float* __restrict__ v, T* __restrict__ shadow, long n,
                                                                 long head, long nvec, AdamArgs c, GuardArgs ga) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  int t;
  if (!guard_begin(ga, c.bc1, c.bc2s, t)) {
    for (long i = tid; i < nvec; i += stride) *(float4*)(acc + head + 4 * i) = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long j = tid; j < n - 4 * nvec; j += stride) acc[edge_index(j, head, nvec)] = 0.f;
    return;
  }
  adam_accum_range<T, HAS_GRAD>(p, acc, g, m, v, shadow, n, head, nvec, c);
  guard_end(ga, t);
}

}  // namespace swn

using namespace swn;

extern "C" int swn_grad_accum(float* acc, const float* grad, long n, float scale, void* stream) {
  SWN_CHECK(acc && grad && n >= 1, "swn_grad_accum: bad arguments");
  SWN_CHECK((uintptr_t)acc % 4 == 0 && (uintptr_t)grad % 4 == 0, "swn_grad_accum: pointers must be 4-byte aligned");
  const void* ptrs[2] = {acc, grad};
  const AccumSplit s = accum_split(n, ptrs, 2, nullptr, 0);
  hipLaunchKernelGGL(grad_accum_kernel, dim3(accum_blocks(n, s)), dim3(256), 0, as_stream(stream), acc, grad, n, s.head, s.nvec, scale);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_adam_accum_step(float* param, float* acc, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow,
                                   int dtype, long n, float lr, float beta1, float beta2, float eps, int step, float accum_scale,
                                   float grad_scale, void* stream) {
  SWN_CHECK(param && acc && exp_avg && exp_avg_sq && step >= 1 && n >= 1, "swn_adam_accum_step: bad arguments");
  const bool half = shadow && dtype == SWN_HALF;
  const void* ptrs[5] = {param, acc, grad, exp_avg, exp_avg_sq};
  for (const void* q : ptrs) SWN_CHECK((uintptr_t)q % 4 == 0, "swn_adam_accum_step: pointers must be 4-byte aligned");
  SWN_CHECK(!shadow || (uintptr_t)shadow % (half ? 2 : 4) == 0, "swn_adam_accum_step: misaligned shadow");
  const AccumSplit s = accum_split(n, ptrs, 5, shadow, half ? 2 : 4);
  const AdamArgs c = {lr, beta1, beta2, eps, 1.f - powf(beta1, (float)step), sqrtf(1.f - powf(beta2, (float)step)), grad_scale,
                      accum_scale};
  const dim3 grid(accum_blocks(n, s)), block(256);
#define SWN_ADAM_ACCUM(T, G) \
  hipLaunchKernelGGL((adam_accum_kernel<T, G>), grid, block, 0, as_stream(stream), param, acc, grad, exp_avg, exp_avg_sq, (T*)shadow, n, s.head, s.nvec, c)
  if (half) {
    if (grad) SWN_ADAM_ACCUM(bf16_t, true); else SWN_ADAM_ACCUM(bf16_t, false);
  } else {
    if (grad) SWN_ADAM_ACCUM(float, true); else SWN_ADAM_ACCUM(float, false);
  }
#undef SWN_ADAM_ACCUM
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_grad_accum_guarded(float* acc, const float* grad, long n, float scale, const int* ok, void* stream) {
  SWN_CHECK(acc && grad && ok && n >= 1, "swn_grad_accum_guarded: bad arguments");
  SWN_CHECK((uintptr_t)acc % 4 == 0 && (uintptr_t)grad % 4 == 0 && (uintptr_t)ok % 4 == 0,
            "swn_grad_accum_guarded: pointers must be 4-byte aligned");
  const void* ptrs[2] = {acc, grad};
  const AccumSplit s = accum_split(n, ptrs, 2, nullptr, 0);
  hipLaunchKernelGGL(grad_accum_guarded_kernel, dim3(accum_blocks(n, s)), dim3(256), 0, as_stream(stream), acc, grad, n, s.head, s.nvec,
                     scale, ok);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_adam_accum_step_guarded(float* param, float* acc, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow,
                                           int dtype, long n, float lr, float beta1, float beta2, float eps, const float* bias_table,
                                           long table_rows, int* step_state, float accum_scale, float grad_scale, const int* ok,
                                           void* stream) {
  SWN_CHECK(param && acc && exp_avg && exp_avg_sq && n >= 1, "swn_adam_accum_step_guarded: bad arguments");
  SWN_CHECK(bias_table && table_rows >= 1 && step_state && ok, "swn_adam_accum_step_guarded: bias table, step state and flag are required");
  SWN_CHECK((uintptr_t)bias_table % 4 == 0 && (uintptr_t)step_state % 4 == 0 && (uintptr_t)ok % 4 == 0,
            "swn_adam_accum_step_guarded: misaligned pointer");
  const bool half = shadow && dtype == SWN_HALF;
  const void* ptrs[5] = {param, acc, grad, exp_avg, exp_avg_sq};
  for (const void* q : ptrs) SWN_CHECK((uintptr_t)q % 4 == 0, "swn_adam_accum_step_guarded: pointers must be 4-byte aligned");
  SWN_CHECK(!shadow || (uintptr_t)shadow % (half ? 2 : 4) == 0, "swn_adam_accum_step_guarded: misaligned shadow");
  const AccumSplit s = accum_split(n, ptrs, 5, shadow, half ? 2 : 4);
  const AdamArgs c = {lr, beta1, beta2, eps, 1.f, 1.f, grad_scale, accum_scale};      // (bc1, bc2s: read from the table in the kernel)
  const GuardArgs ga = {ok, step_state, bias_table, table_rows};
  const dim3 grid(accum_blocks(n, s)), block(256);
#define SWN_ADAM_ACCUM_G(T, G) \
  hipLaunchKernelGGL((adam_accum_guarded_kernel<T, G>), grid, block, 0, as_stream(stream), param, acc, grad, exp_avg, exp_avg_sq, (T*)shadow, n, s.head, s.nvec, c, ga)
  if (half) {
    if (grad) SWN_ADAM_ACCUM_G(bf16_t, true); else SWN_ADAM_ACCUM_G(bf16_t, false);
  } else {
    if (grad) SWN_ADAM_ACCUM_G(float, true); else SWN_ADAM_ACCUM_G(float, false);
  }
#undef SWN_ADAM_ACCUM_G
  SWN_LAUNCH_CHECK();
  return 0;
}
