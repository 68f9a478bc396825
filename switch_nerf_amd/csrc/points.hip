// Per-sample point outputs of render_rays (rendering.py:299, :413-417, :443-452) and the device side of the per-expert point-cloud
// export (Runner._run_validation_points, runner.py:2024-2142): PLY vertex bodies packed on the GPU, partitioned stably by expert.
// Nothing here runs on the training step.
#include "common.hpp"

// pts = rays_o + rays_d * z must match torch's separate mul and add bit for bit, so no contraction into FMAs in this file.
#pragma clang fp contract(off)

namespace swn {
namespace {

// ------------------------------------------------------------------------------------------------ point fields
// one wave per ray, like composite_fwd_kernel; lanes stride over the samples.
__global__ __launch_bounds__(256) void point_fields_kernel(const float* __restrict__ rays, const float* __restrict__ z_pts, int n_pts,
                                                           const float* __restrict__ z, const float* __restrict__ raw, int N, int T,
                                                           float last_delta, const float* __restrict__ last_delta_ray,
                                                           const int32_t* __restrict__ order, float* __restrict__ pts,
                                                           float* __restrict__ alpha, float* __restrict__ pts_alpha) {
  const int lane = threadIdx.x & 63;
  const long ray = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (ray >= N) return;
  if (pts) {
    const float* rr = rays + ray * 8;
    const float ox = rr[0], oy = rr[1], oz = rr[2], dx = rr[3], dy = rr[4], dz = rr[5];
    const float* zp = z_pts + ray * n_pts;
    float* out = pts + ray * n_pts * 3;
    for (int s = lane; s < n_pts; s += 64) {
      const float t = zp[s];
      out[s * 3 + 0] = ox + dx * t;          // rendering.py:90, :103
      out[s * 3 + 1] = oy + dy * t;
      out[s * 3 + 2] = oz + dz * t;
    }
  }
  if (!alpha && !pts_alpha) return;
  if (last_delta_ray) last_delta = last_delta_ray[ray];
  const float* zr = z + ray * T;
  const float4* rw = (const float4*)(raw + ray * T * 4);
  for (int s = lane; s < T; s += 64) {
    const float zs = zr[s];
    const float dl = (s + 1 < T) ? (zr[s + 1] - zs) : last_delta;      // the compositing kernel's delta (rendering.py:436-442)
    const float a = 1.f - expf(-dl * rw[s].w);
    if (alpha) alpha[ray * T + s] = a;
    if (pts_alpha) {
      if (order) {                                                       // scatter back to the source order (:446-452)
        const int src = order[ray * T + s];
        if (src < n_pts) pts_alpha[ray * n_pts + src] = a;
      } else {
        pts_alpha[ray * T + s] = a;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ PLY vertex bodies
constexpr int PK_THREADS = 256;
constexpr int PK_ROUNDS = 8;                              // records per thread per block
constexpr int PK_CHUNK = PK_THREADS * PK_ROUNDS;          // records per block
constexpr int PK_MAX_E = 64;

struct PackArgs {
  const float* pts;            // [R, S, 3]
  const float* rgb;            // [R, S, rgb_stride] (first 3 channels)
  const float* alpha;          // [R, S]
  const int32_t* idx;          // [R * S] or NULL
  const float* pixel;          // [R, 3] (SEG_RGB)
  const uint8_t* palette;      // [E, 3]
  int rgb_stride, R, S, skip, Sk, E, mode;
  long n;                      // R * Sk kept records
};

__device__ __forceinline__ uint32_t q8(float x) {             // (x * 255).to(torch.uint8): fp32 product, truncation
  return (uint32_t)(int)(x * 255.f) & 0xFFu;
}

__device__ __forceinline__ int rec_expert(const PackArgs& a, long i) {
  const long r = (uint32_t)i / (uint32_t)a.Sk;                 // (n < 2^31: the host checks)
  const int j = (int)(i - r * a.Sk);
  const int e = a.idx[r * a.S + (long)j * a.skip];
  return (e >= 0 && e < a.E) ? e : -1;
}

// the record of kept point i as four words (the 15-byte SEG_RGB record uses the first 15 bytes)
__device__ __forceinline__ uint4 make_record(const PackArgs& a, long i) {
  const long r = (uint32_t)i / (uint32_t)a.Sk;
  const int j = (int)(i - r * a.Sk);
  const long p = r * a.S + (long)j * a.skip;
  const float* q = a.pts + p * 3;
  uint4 w;
  w.x = __float_as_uint(q[0]); w.y = __float_as_uint(q[1]); w.z = __float_as_uint(q[2]);
  uint32_t c0, c1, c2, c3 = 0;
  if (a.mode == SWN_PLY_RGBA) {
    const float* c = a.rgb + p * a.rgb_stride;
    c0 = q8(c[0]); c1 = q8(c[1]); c2 = q8(c[2]); c3 = q8(a.alpha[p]);
  } else {
    const int e = a.idx[p];
    c0 = c1 = c2 = 0;                                            // (an index outside [0, E) keeps the zero colour, runner.py:2084)
    if (e >= 0 && e < a.E) { c0 = a.palette[e * 3]; c1 = a.palette[e * 3 + 1]; c2 = a.palette[e * 3 + 2]; }
    if (a.mode == SWN_PLY_SEG_ALPHA) {
      c3 = q8(a.alpha[p]);
    } else if (j == a.Sk - 1) {                                  // the last kept sample carries the pixel colour (:2124)
      c0 = q8(a.pixel[r * 3]); c1 = q8(a.pixel[r * 3 + 1]); c2 = q8(a.pixel[r * 3 + 2]);
    }
  }
  w.w = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
  return w;
}

__device__ __forceinline__ void store_record(uint8_t* base, long pos, int rec_bytes, const uint4& w) {
  if (rec_bytes == 16) {
    *(uint4*)(base + pos * 16) = w;
  } else {                                                       // 15 bytes: x y z + red green blue
    uint8_t* d = base + pos * 15;
    const uint32_t v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int b = 0; b < 15; ++b) d[b] = (uint8_t)(v[b >> 2] >> (8 * (b & 3)));
  }
}

// pass 1: records of each expert in each block's chunk -> bc[block * E + e]
__global__ __launch_bounds__(PK_THREADS) void pack_count_kernel(PackArgs a, int32_t* __restrict__ bc) {
  __shared__ int hist[PK_MAX_E];
  for (int e = threadIdx.x; e < a.E; e += PK_THREADS) hist[e] = 0;
  __syncthreads();
  const long base = (long)blockIdx.x * PK_CHUNK;
  for (int k = 0; k < PK_ROUNDS; ++k) {
    const long i = base + k * PK_THREADS + threadIdx.x;
    if (i < a.n) {
      const int e = rec_expert(a, i);
      if (e >= 0) atomicAdd(&hist[e], 1);            // (integer counts: order-free, so deterministic)
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < a.E; e += PK_THREADS) bc[(long)blockIdx.x * a.E + e] = hist[e];
}

// pass 2: one workgroup per expert: exclusive scan of its column over the blocks (in place) and its total -> counts[e]
__global__ __launch_bounds__(1024) void pack_scan_kernel(int32_t* __restrict__ bc, int n_blocks, int E, int32_t* __restrict__ counts) {
  __shared__ int wsum[16];
  __shared__ int carry_s;
  const int e = blockIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int b0 = 0; b0 < n_blocks; b0 += 1024) {
    const int b = b0 + threadIdx.x;
    const int v = b < n_blocks ? bc[(long)b * E + e] : 0;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    int before = carry_s;
    for (int w = 0; w < wid; ++w) before += wsum[w];
    if (b < n_blocks) bc[(long)b * E + e] = before + incl - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = before + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[e] = carry_s;
}

// pass 3: build every record once; write it to the "all" body at its own index and to the per-expert body at
// base(e) + (records of e in earlier blocks) + (records of e earlier in this block): in-wave ranks from a 64-bit ballot, wave
// offsets in LDS.  Stable, and the same bytes on every run.
__global__ __launch_bounds__(PK_THREADS) void pack_scatter_kernel(PackArgs a, const int32_t* __restrict__ bc,
                                                                  const int32_t* __restrict__ counts, uint8_t* __restrict__ out_all,
                                                                  uint8_t* __restrict__ out_exp, int rec_bytes) {
  __shared__ long cursor[PK_MAX_E];
  __shared__ int wcnt[PK_THREADS / 64][PK_MAX_E];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool part = out_exp != nullptr;             // (the host checks that idx is given then)
  if (part) {
    for (int e = threadIdx.x; e < a.E; e += PK_THREADS) {
      long b = 0;
      for (int f = 0; f < e; ++f) b += counts[f];
      cursor[e] = b + bc[(long)blockIdx.x * a.E + e];
    }
  }
  const long base = (long)blockIdx.x * PK_CHUNK;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (int k = 0; k < PK_ROUNDS; ++k) {
    const long i = base + k * PK_THREADS + threadIdx.x;
    const bool ok = i < a.n;
    uint4 w = make_uint4(0, 0, 0, 0);
    if (ok) {
      w = make_record(a, i);
      if (out_all) store_record(out_all, i, rec_bytes, w);
    }
    if (!part) continue;
    const int my_e = ok ? rec_expert(a, i) : -1;
    int rank = 0;
    for (int e = 0; e < a.E; ++e) {
      const uint64_t m = __ballot(my_e == e);
      if (my_e == e) rank = __popcll(m & lt);
      if (lane == 0) wcnt[wid][e] = __popcll(m);
    }
    __syncthreads();                                   // (also orders the cursor initialisation before the first round)
    if (my_e >= 0) {
      long pos = cursor[my_e] + rank;
      for (int v = 0; v < wid; ++v) pos += wcnt[v][my_e];
      store_record(out_exp, pos, rec_bytes, w);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < a.E; e += PK_THREADS) {
      int s = 0;
#pragma unroll
      for (int v = 0; v < PK_THREADS / 64; ++v) s += wcnt[v][e];
      cursor[e] += s;
    }
    __syncthreads();
  }
}

}  // namespace
}  // namespace swn

using namespace swn;

extern "C" int swn_point_fields(const float* rays, const float* z_pts, int n_pts, const float* z, const float* raw, int n_rays,
                                int n_samples, float last_delta, const float* last_delta_ray, const int32_t* order, float* pts,
                                float* alpha, float* pts_alpha, void* stream) {
  SWN_CHECK(n_rays >= 0 && n_samples >= 1 && n_pts >= 1, "swn_point_fields: bad sizes");
  SWN_CHECK(!pts || (rays && (z_pts || z)), "swn_point_fields: pts needs rays and depths");
  SWN_CHECK(!(alpha || pts_alpha) || (z && raw), "swn_point_fields: alpha needs z and raw");
  SWN_CHECK(order || n_pts == n_samples || !pts_alpha, "swn_point_fields: without order, n_pts must equal n_samples");
  SWN_CHECK(order || z_pts || n_pts == n_samples || !pts, "swn_point_fields: pts from z needs n_pts == n_samples");
  if (n_rays == 0) return 0;
  hipLaunchKernelGGL(point_fields_kernel, dim3(cdiv(n_rays, 4)), dim3(256), 0, as_stream(stream), rays, z_pts ? z_pts : z, n_pts,
                     z, raw, n_rays, n_samples, last_delta, last_delta_ray, order, pts, alpha, pts_alpha);
  SWN_LAUNCH_CHECK();
  return 0;
}

static size_t pack_workspace_bytes(int n_rays, int n_samples, int skip, int n_experts) {
  const long n = (long)n_rays * ((n_samples + skip - 1) / skip);
  return (size_t)((n + PK_CHUNK - 1) / PK_CHUNK) * n_experts * sizeof(int32_t);
}

extern "C" int swn_points_pack(const float* pts, const float* rgb, int rgb_stride, const float* alpha, const int32_t* idx,
                               const float* pixel_rgb, const uint8_t* palette, int n_rays, int n_samples, int skip, int n_experts,
                               int mode, void* out_all, void* out_experts, int32_t* counts, void* workspace, size_t workspace_bytes,
                               void* stream) {
  SWN_CHECK(mode == SWN_PLY_RGBA || mode == SWN_PLY_SEG_ALPHA || mode == SWN_PLY_SEG_RGB, "swn_points_pack: bad mode %d", mode);
  SWN_CHECK(n_rays >= 0 && n_samples >= 1 && skip >= 1, "swn_points_pack: bad sizes");
  SWN_CHECK(pts, "swn_points_pack: null pts");
  SWN_CHECK(n_experts >= 1 && n_experts <= PK_MAX_E, "swn_points_pack: 1..%d experts", PK_MAX_E);
  SWN_CHECK(mode != SWN_PLY_RGBA || (rgb && (rgb_stride == 3 || rgb_stride == 4)), "swn_points_pack: RGBA needs rgb (stride 3 or 4)");
  SWN_CHECK(mode == SWN_PLY_SEG_RGB || alpha, "swn_points_pack: null alpha");
  SWN_CHECK(mode == SWN_PLY_RGBA || (idx && palette), "swn_points_pack: segmentation modes need idx and palette");
  SWN_CHECK(mode != SWN_PLY_SEG_RGB || pixel_rgb, "swn_points_pack: SEG_RGB needs pixel_rgb");
  SWN_CHECK(!out_experts || (idx && counts), "swn_points_pack: per-expert bodies need idx and counts");
  if (n_rays == 0) {
    if (counts) (void)hipMemsetAsync(counts, 0, n_experts * sizeof(int32_t), as_stream(stream));
    return 0;
  }
  PackArgs a;
  a.pts = pts; a.rgb = rgb; a.alpha = alpha; a.idx = idx; a.pixel = pixel_rgb; a.palette = palette;
  a.rgb_stride = rgb_stride; a.R = n_rays; a.S = n_samples; a.skip = skip; a.Sk = (n_samples + skip - 1) / skip; a.E = n_experts;
  a.mode = mode; a.n = (long)n_rays * a.Sk;
  const long blocks = (a.n + PK_CHUNK - 1) / PK_CHUNK;
  SWN_CHECK(a.n < (1L << 31), "swn_points_pack: %ld records is too many (< 2^31 per call)", a.n);
  const int rec_bytes = mode == SWN_PLY_SEG_RGB ? 15 : 16;
  hipStream_t s = as_stream(stream);
  int32_t* bc = (int32_t*)workspace;
  const bool part = out_experts != nullptr;
  if (part) {
    SWN_CHECK(workspace && workspace_bytes >= pack_workspace_bytes(n_rays, n_samples, skip, n_experts),
              "swn_points_pack: workspace too small (4 E ceil(records / 2048) bytes)");
    hipLaunchKernelGGL(pack_count_kernel, dim3((unsigned)blocks), dim3(PK_THREADS), 0, s, a, bc);
    SWN_LAUNCH_CHECK();
    hipLaunchKernelGGL(pack_scan_kernel, dim3(n_experts), dim3(1024), 0, s, bc, (int)blocks, n_experts, counts);
    SWN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pack_scatter_kernel, dim3((unsigned)blocks), dim3(PK_THREADS), 0, s, a, bc, counts, (uint8_t*)out_all,
                     (uint8_t*)out_experts, rec_bytes);
  SWN_LAUNCH_CHECK();
  return 0;
}
