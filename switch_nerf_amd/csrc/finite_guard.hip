// The finite guard (the reference's check_finite, runner.py:620-673, on by default there): a training step whose scalar metrics are
// not all finite is dropped - no Adam step, gradients cleared - and counted.  The reference decides with an .item() on the host; here
// the decision is a device flag that the optimiser launches read, so a guarded step reads nothing on the host and can be captured.
//   swn_finite_guard        metrics of the step (the loss kernels' out4 / out5) -> ok[0], skipped[0] += 1 - ok
//   swn_adam_step_guarded   swn_adam_step under the flag, the step count on the device (adam.hpp: guard_begin / guard_end)
//   swn_adam_bias_table     the host-side table of bias corrections the guarded launches index with that step count
// (the guarded forms of the accumulation kernels live with their unguarded ones in accum.hip)
#include "adam.hpp"

namespace swn {

// One wave.  Lane i < n tests slot i: finite, or +inf in the psnr slot (a perfect reproduction: photo = 0, psnr = +inf, which the
// reference lets through).  -inf and NaN fail everywhere.
__global__ __launch_bounds__(64) void finite_guard_kernel(const float* __restrict__ metrics, int n, int psnr_slot, int* __restrict__ ok,
                                                          long long* __restrict__ skipped) {
  const int lane = threadIdx.x;
  bool good = true;
  if (lane < n) {
    const uint32_t bits = __float_as_uint(metrics[lane]);      // on the bits: no compiler flag can fold the test away
    good = (bits & 0x7f800000u) != 0x7f800000u || (lane == psnr_slot && bits == 0x7f800000u);
  }
  const bool all = __ballot(!good) == 0ull;
  if (lane == 0) {
    ok[0] = all ? 1 : 0;
    if (skipped && !all) skipped[0] += 1;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, T* __restrict__ shadow, long n, float lr, float b1,
                                                           float b2, float eps, float gscale, GuardArgs ga) {
  float bc1, bc2s;
  int t;
  if (!guard_begin(ga, bc1, bc2s, t)) return;      // a skipped step: parameters, moments, copies and the step count stay as they are
  adam_range(p, g, m, v, shadow, n, lr, b1, b2, eps, bc1, bc2s, gscale);      // (adam_kernel's loop)
  guard_end(ga, t);
}

}  // namespace swn

using namespace swn;

extern "C" int swn_finite_guard(const float* metrics, int n, int psnr_slot, int* ok, long long* skipped, void* stream) {
  SWN_CHECK(metrics && ok, "swn_finite_guard: null pointer");
  SWN_CHECK(n >= 1 && n <= 64, "swn_finite_guard: 1 to 64 metrics, got %d", n);
  SWN_CHECK(psnr_slot >= -1 && psnr_slot < n, "swn_finite_guard: psnr slot %d outside the %d metrics (-1: none)", psnr_slot, n);
  SWN_CHECK((uintptr_t)metrics % 4 == 0 && (uintptr_t)ok % 4 == 0 && (uintptr_t)skipped % 8 == 0, "swn_finite_guard: misaligned pointer");
  hipLaunchKernelGGL(finite_guard_kernel, dim3(1), dim3(64), 0, as_stream(stream), metrics, n, psnr_slot, ok, skipped);
  SWN_LAUNCH_CHECK();
  return 0;
}

// Host only.  Row t - 1 = {bc1, bc2s} of optimizer step t, the expressions of swn_adam_step on the same host: what the guarded
// launches read is bit for bit what the unguarded launch is handed.  The table ends where both have reached exactly 1.0f (for
// 0.9 / 0.999 after ~17.3 k steps); *rows = its length.
extern "C" int swn_adam_bias_table(float beta1, float beta2, float* table, long capacity, long* rows) {
  SWN_CHECK(table && rows && capacity >= 1, "swn_adam_bias_table: bad arguments");
  SWN_CHECK(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "swn_adam_bias_table: betas must lie in [0, 1)");
  for (long t = 1; t <= capacity; ++t) {
    const float bc1 = 1.f - powf(beta1, (float)t);
    const float bc2s = sqrtf(1.f - powf(beta2, (float)t));
    table[2 * (t - 1)] = bc1;
    table[2 * (t - 1) + 1] = bc2s;
    if (bc1 == 1.f && bc2s == 1.f) {
      *rows = t;
      return 0;
    }
  }
  return set_error("swn_adam_bias_table: the bias corrections have not reached 1 after %ld steps; pass a larger table", capacity);
}

extern "C" int swn_adam_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow, int dtype,
                                     long n, float lr, float beta1, float beta2, float eps, const float* bias_table, long table_rows,
                                     int* step_state, float grad_scale, const int* ok, void* stream) {
  SWN_CHECK(param && grad && exp_avg && exp_avg_sq && n >= 1, "swn_adam_step_guarded: bad arguments");
  SWN_CHECK(bias_table && table_rows >= 1 && step_state && ok, "swn_adam_step_guarded: bias table, step state and flag are required");
  SWN_CHECK((uintptr_t)bias_table % 4 == 0 && (uintptr_t)step_state % 4 == 0 && (uintptr_t)ok % 4 == 0,
            "swn_adam_step_guarded: misaligned pointer");
  int blocks = cdiv(n, 256);
  if (blocks > 4096) blocks = 4096;
  const GuardArgs ga = {ok, step_state, bias_table, table_rows};
  if (shadow && dtype == SWN_HALF)
    hipLaunchKernelGGL((adam_guarded_kernel<bf16_t>), dim3(blocks), dim3(256), 0, as_stream(stream), param, grad, exp_avg, exp_avg_sq,
                       (bf16_t*)shadow, n, lr, beta1, beta2, eps, grad_scale, ga);
  else
    hipLaunchKernelGGL((adam_guarded_kernel<float>), dim3(blocks), dim3(256), 0, as_stream(stream), param, grad, exp_avg, exp_avg_sq,
                       (float*)shadow, n, lr, beta1, beta2, eps, grad_scale, ga);
  SWN_LAUNCH_CHECK();
  return 0;
}
