// Seeded device-side noise (philox.hpp): the fill kernel behind every supplied-noise argument of the library, and the step counter's
// advance.  The step is READ FROM DEVICE MEMORY by the kernels, so a launch captured into a hipGraph follows it from replay to replay.
//   swn_rng_fill     out[i] = draw of element base + i of (seed, *step_dev, stream_id): uniform [0,1) or normal * scale
//   swn_rng_advance  *step_dev += 1 (one thread; the last launch of a training step)
// The fill is bandwidth-trivial (8 MB at the full batch): one Philox block = four consecutive elements per thread, one 16-byte store
// where the output's alignment allows it, and a grid small enough to be launch-bound.
#include "common.hpp"
#include "philox.hpp"

namespace swn {

// Thread t owns Philox block b0 + t, i.e. the elements 4 (b0 + t) .. + 3, i.e. out[i0 .. i0 + 3] with i0 = 4 (b0 + t) - base.
// VEC: out + i0 is 16-byte aligned for every t (decided on the host); the first / last block may be partial either way.
template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void rng_fill_kernel(float* __restrict__ out, long n, long base, long n_blocks, float scale,
                                                       uint64_t seed, const int64_t* __restrict__ step_dev, int stream_id) {
  const uint32_t step = (uint32_t)*step_dev;
  const long b0 = base >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n_blocks; t += stride) {
    const PhiloxWords v = philox_block(seed, step, stream_id, b0 + t);
    float r[4];
    if constexpr (KIND == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = philox_uniform(v.w[k]);
    } else {
      philox_normal_pair(v.w[0], v.w[1], scale, r[0], r[1]);
      philox_normal_pair(v.w[2], v.w[3], scale, r[2], r[3]);
    }
    const long i0 = 4 * (b0 + t) - base;           // in [-3, n - 1]
    if (VEC && i0 >= 0 && i0 + 4 <= n) {
      *(float4*)(out + i0) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long i = i0 + k;
        if (i >= 0 && i < n) out[i] = r[k];
      }
    }
  }
}

__global__ void rng_advance_kernel(int64_t* __restrict__ step_dev) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *step_dev += 1;
}

}  // namespace swn

using namespace swn;

extern "C" int swn_rng_fill(float* out, int64_t n, int64_t base, int kind, float scale, uint64_t seed, const int64_t* step_dev,
                            int stream_id, void* stream) {
  SWN_CHECK(n >= 0 && base >= 0, "swn_rng_fill: n and base must be >= 0");
  SWN_CHECK(base <= INT64_MAX - n, "swn_rng_fill: base + n overflows");
  SWN_CHECK(kind == 0 || kind == 1, "swn_rng_fill: kind must be 0 (uniform) or 1 (normal), got %d", kind);
  SWN_CHECK(stream_id >= 0 && stream_id < RNG_STREAMS, "swn_rng_fill: stream id %d outside 0..%d", stream_id, RNG_STREAMS - 1);
  if (n == 0) return 0;
  SWN_CHECK(out && step_dev, "swn_rng_fill: null pointer");
  SWN_CHECK(((uintptr_t)out & 3) == 0, "swn_rng_fill: out must be 4-byte aligned");
  const long n_blocks = ((base + n - 1) >> 2) - (base >> 2) + 1;
  // out + (4 b - base) is 16-byte aligned for every block b  <=>  (address / 4 - base) % 4 == 0
  const bool vec = ((((uintptr_t)out >> 2) - (uintptr_t)base) & 3) == 0;
  long blocks = (n_blocks + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  const dim3 grid((unsigned)blocks), block(256);
  hipStream_t s = as_stream(stream);
  if (kind == 0) {
    if (vec) hipLaunchKernelGGL((rng_fill_kernel<0, true>), grid, block, 0, s, out, (long)n, (long)base, n_blocks, scale, seed, step_dev, stream_id);
    else hipLaunchKernelGGL((rng_fill_kernel<0, false>), grid, block, 0, s, out, (long)n, (long)base, n_blocks, scale, seed, step_dev, stream_id);
  } else {
    if (vec) hipLaunchKernelGGL((rng_fill_kernel<1, true>), grid, block, 0, s, out, (long)n, (long)base, n_blocks, scale, seed, step_dev, stream_id);
    else hipLaunchKernelGGL((rng_fill_kernel<1, false>), grid, block, 0, s, out, (long)n, (long)base, n_blocks, scale, seed, step_dev, stream_id);
  }
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_rng_advance(int64_t* step_dev, void* stream) {
  SWN_CHECK(step_dev, "swn_rng_advance: null pointer");
  hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(1), 0, as_stream(stream), step_dev);
  SWN_LAUNCH_CHECK();
  return 0;
}
