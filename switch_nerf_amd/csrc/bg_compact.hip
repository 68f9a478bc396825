// Fixed-shape ("padded") background rows of a scene with a background model (background.py, bg_capacity): the rays that leave the
// foreground bound are compacted on the DEVICE into the first n_bg of C rows, so that no launch of the step is sized by a host read and
// the whole step can be captured into a hipGraph.
//   bg_compact_kernel    stable compaction of has_bg[N] -> idx_bg[C], n_bg, the gathered rays / image indices, benign padding rows
//   bg_blend_fwd_kernel  rgb / depth of the foreground += the background's, times the leftover transmittance (rendering.py:104-131)
//   bg_blend_bwd_kernel  its backward: dL/d bg_lambda per ray, dL/d rgb of the background rows (exactly +0 on padding rows)
// All three read n_bg from device memory.  Plain C++, fp32, fma contraction off (the products and sums round like torch's).
#include "common.hpp"

namespace swn {

struct PadRay { float v[8]; };

constexpr int COMPACT_THREADS = 1024;      // 16 waves of 64

// Geometry: ONE workgroup of 1024 threads walks has_bg in slabs of 1024 rays.  Per slab: a wave ballot gives each set lane its rank in
// its wave, the 16 wave counts go through LDS and every thread adds the counts of the waves before its own - a block scan without
// atomics, so position j always holds the j-th set ray (ascending) and the output is a pure function of the input.  A ray batch is at
// most a few 10^5 rays (8192: 8 slabs, a few microseconds): latency-sized work that a second level of scan would not shorten.
// Rows past n_bg (padding): idx 0, image index 0, the caller's benign ray.  Set rays past C are counted, not written.
template <typename I>
__global__ __launch_bounds__(COMPACT_THREADS) void bg_compact_kernel(const int32_t* __restrict__ has_bg, const float* __restrict__ rays,
                                                                     const I* __restrict__ img, PadRay pad, int N, int C,
                                                                     int64_t* __restrict__ idx_bg, int32_t* __restrict__ n_bg,
                                                                     float* __restrict__ rays_b, I* __restrict__ img_b) {
  __shared__ int wave_cnt[COMPACT_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int base = 0;                                                   // set rays before this slab (the same in every thread)
  for (int i0 = 0; i0 < N; i0 += COMPACT_THREADS) {               // (uniform trip count: every thread reaches both barriers)
    const int i = i0 + t;
    const bool set = i < N && has_bg[i] != 0;
    const unsigned long long m = __ballot(set);
    if (lane == 0) wave_cnt[w] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < COMPACT_THREADS / 64; ++k) {
      const int c = wave_cnt[k];
      before += k < w ? c : 0;
      total += c;
    }
    const int pos = base + before + __popcll(m & ((1ull << lane) - 1ull));
    if (set && pos < C) {
      idx_bg[pos] = i;
      img_b[pos] = img[i];
      const float4* src = reinterpret_cast<const float4*>(rays + (long)i * 8);
      float4* dst = reinterpret_cast<float4*>(rays_b + (long)pos * 8);
      dst[0] = src[0];
      dst[1] = src[1];
    }
    base += total;
    __syncthreads();                                              // wave_cnt is rewritten by the next slab
  }
  for (int j = base + t; j < C; j += COMPACT_THREADS) {           // padding rows (none when base >= C)
    idx_bg[j] = 0;
    img_b[j] = 0;
    float4* dst = reinterpret_cast<float4*>(rays_b + (long)j * 8);
    dst[0] = make_float4(pad.v[0], pad.v[1], pad.v[2], pad.v[3]);
    dst[1] = make_float4(pad.v[4], pad.v[5], pad.v[6], pad.v[7]);
  }
  if (t == 0) *n_bg = base;                                       // the true count, also when it exceeds C
}

// one thread per background row j; rows j >= min(n_bg, C) write nothing.  idx_bg's valid entries are distinct, so no two threads
// touch the same ray; an entry outside [0, N) (never produced by bg_compact_kernel) is skipped rather than followed.
__global__ __launch_bounds__(256) void bg_blend_fwd_kernel(const int64_t* __restrict__ idx_bg, const int32_t* __restrict__ n_bg,
                                                           const float* __restrict__ lam, const float* __restrict__ rgb_b,
                                                           const float* __restrict__ depth_b, int N, int C, float* __restrict__ rgb,
                                                           float* __restrict__ depth) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = min(*n_bg, C);
  if (j >= n) return;
  const int64_t i = idx_bg[j];
  if (i < 0 || i >= N) return;
  const float l = lam[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p = rgb_b[(long)j * 3 + c] * l;
    rgb[i * 3 + c] = rgb[i * 3 + c] + p;
  }
  const float pd = depth_b[j] * l;
  depth[i] = depth[i] + pd;
}

// d_lam is zero-filled by the launch in front of this one; one thread per background row j
__global__ __launch_bounds__(256) void bg_blend_bwd_kernel(const int64_t* __restrict__ idx_bg, const int32_t* __restrict__ n_bg,
                                                           const float* __restrict__ lam, const float* __restrict__ rgb_b,
                                                           const float* __restrict__ d_rgb, int N, int C, float* __restrict__ d_lam,
                                                           float* __restrict__ d_rgb_b) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= C) return;
  const int n = min(*n_bg, C);
  const int64_t i = j < n ? idx_bg[j] : -1;
  float out[3] = {0.f, 0.f, 0.f};                                 // padding rows: exactly +0
  if (i >= 0 && i < N) {
    const float l = lam[i];
    float g[3], p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      g[c] = d_rgb[i * 3 + c];
      p[c] = g[c] * rgb_b[(long)j * 3 + c];
      out[c] = g[c] * l;
    }
    d_lam[i] = (p[0] + p[2]) + p[1];                              // the association of torch's sum(-1) over three elements (two lanes: {0, 2}, {1})
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) d_rgb_b[(long)j * 3 + c] = out[c];
}

}  // namespace swn

using namespace swn;

extern "C" int swn_bg_compact(const int32_t* has_bg, const float* rays, const void* image_indices, int idx_is_i64,
                              const float* pad_ray_host, int n_rays, int capacity, int64_t* idx_bg, int32_t* n_bg, float* rays_b,
                              void* img_b, void* stream) {
  SWN_CHECK(has_bg && rays && image_indices && pad_ray_host && idx_bg && n_bg && rays_b && img_b, "swn_bg_compact: null pointer");
  SWN_CHECK(n_rays >= 1, "swn_bg_compact: n_rays %d < 1", n_rays);
  SWN_CHECK(capacity >= 1 && capacity <= n_rays, "swn_bg_compact: capacity %d outside [1, n_rays %d]", capacity, n_rays);
  SWN_CHECK(((uintptr_t)rays & 15) == 0 && ((uintptr_t)rays_b & 15) == 0, "swn_bg_compact: rays / rays_b must be 16-byte aligned");
  PadRay pad;
  memcpy(pad.v, pad_ray_host, sizeof(pad.v));
  if (idx_is_i64)
    hipLaunchKernelGGL(bg_compact_kernel<int64_t>, dim3(1), dim3(COMPACT_THREADS), 0, as_stream(stream), has_bg, rays,
                       (const int64_t*)image_indices, pad, n_rays, capacity, idx_bg, n_bg, rays_b, (int64_t*)img_b);
  else
    hipLaunchKernelGGL(bg_compact_kernel<int32_t>, dim3(1), dim3(COMPACT_THREADS), 0, as_stream(stream), has_bg, rays,
                       (const int32_t*)image_indices, pad, n_rays, capacity, idx_bg, n_bg, rays_b, (int32_t*)img_b);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_bg_blend_fwd(const int64_t* idx_bg, const int32_t* n_bg, const float* bg_lambda, const float* rgb_b,
                                const float* depth_b, int n_rays, int capacity, float* rgb, float* depth, void* stream) {
  SWN_CHECK(idx_bg && n_bg && bg_lambda && rgb_b && depth_b && rgb && depth, "swn_bg_blend_fwd: null pointer");
  SWN_CHECK(n_rays >= 1 && capacity >= 1 && capacity <= n_rays, "swn_bg_blend_fwd: capacity %d outside [1, n_rays %d]", capacity, n_rays);
  hipLaunchKernelGGL(bg_blend_fwd_kernel, dim3(cdiv(capacity, 256)), dim3(256), 0, as_stream(stream), idx_bg, n_bg, bg_lambda, rgb_b,
                     depth_b, n_rays, capacity, rgb, depth);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_bg_blend_bwd(const int64_t* idx_bg, const int32_t* n_bg, const float* bg_lambda, const float* rgb_b,
                                const float* d_rgb, int n_rays, int capacity, float* d_bg_lambda, float* d_rgb_b, void* stream) {
  SWN_CHECK(idx_bg && n_bg && bg_lambda && rgb_b && d_rgb && d_bg_lambda && d_rgb_b, "swn_bg_blend_bwd: null pointer");
  SWN_CHECK(n_rays >= 1 && capacity >= 1 && capacity <= n_rays, "swn_bg_blend_bwd: capacity %d outside [1, n_rays %d]", capacity, n_rays);
  const hipError_t e = fill_u32_async(d_bg_lambda, 0u, (size_t)n_rays * 4, as_stream(stream));
  SWN_CHECK(e == hipSuccess, "swn_bg_blend_bwd: fill failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(bg_blend_bwd_kernel, dim3(cdiv(capacity, 256)), dim3(256), 0, as_stream(stream), idx_bg, n_bg, bg_lambda, rgb_b,
                     d_rgb, n_rays, capacity, d_bg_lambda, d_rgb_b);
  SWN_LAUNCH_CHECK();
  return 0;
}
