// Rays from cameras on the device: the reference's ray_utils.py (get_ray_directions :6-19, get_rays :22-32, get_rays_batch :35-44,
// _get_rays_inner :47-66, _truncate_with_plane_intersection :69-90) in fp32, one thread per ray, outside any autocast.
//   rays_from_camera_kernel       one camera by value: pixel -> camera direction -> world direction -> bounds -> rays[n, 8] (and the
//                                 camera's image index per ray); the directions never reach memory
//   ray_directions_kernel         get_ray_directions: [H, W, 3]
//   rays_from_directions_kernel   get_rays / get_rays_batch: directions [n, 3] x poses [n_cam, 3, 4] -> rays [n_cam, n, 8]
//   rays_from_pixels_kernel       the gather form of a training batch: (camera index, pixel index) per ray, cameras from a table
// Every kernel goes through the SAME three helpers (pixel_direction, rotate_direction, ray_bounds), contraction off inside them,
// IEEE division and square root, the three squares of a norm added as (x^2 + y^2) + z^2: the same pixel of the same camera gives the
// same bits through every entry.  No LDS, no atomics; each ray is written as two 16-byte stores.
#include "common.hpp"

namespace swn {

constexpr int RAY_THREADS = 256;

struct RayVec { float x, y, z; };
struct RayPose { float m[12]; };            // c2w [3][4] row-major: columns 0..2 the rotation, column 3 the camera origin
struct RayBounds {                          // near / far of _get_rays_inner; has_alt 0: the altitude planes are not applied
  float near, far, alt_near, alt_far;
  int has_alt;
};

__device__ __forceinline__ float ray_norm(float x, float y, float z) {
#pragma clang fp contract(off)
  const float xx = x * x, yy = y * y, zz = z * z;
  return sqrtf((xx + yy) + zz);
}

// get_ray_directions for the pixel (col, row): ((i - cx) / fx, -(j - cy) / fy, -1) / its norm; i, j the pixel's corner, or its centre.
__device__ __forceinline__ RayVec pixel_direction(int col, int row, float fx, float fy, float cx, float cy, int center_pixels) {
#pragma clang fp contract(off)
  float i = (float)col, j = (float)row;
  if (center_pixels) {
    i = i + 0.5f;
    j = j + 0.5f;
  }
  const float x = (i - cx) / fx;
  const float y = -(j - cy) / fy;
  const float z = -1.f;
  const float n = ray_norm(x, y, z);
  return {x / n, y / n, z / n};
}

// get_rays: directions @ c2w[:, :3].T, each dot product as (d0 r0 + d1 r1) + d2 r2, then divided by its norm.
__device__ __forceinline__ RayVec rotate_direction(RayVec d, const RayPose& c) {
#pragma clang fp contract(off)
  const float x = (d.x * c.m[0] + d.y * c.m[1]) + d.z * c.m[2];
  const float y = (d.x * c.m[4] + d.y * c.m[5]) + d.z * c.m[6];
  const float z = (d.x * c.m[8] + d.y * c.m[9]) + d.z * c.m[10];
  const float n = ray_norm(x, y, z);
  return {x / n, y / n, z / n};
}

// _truncate_with_plane_intersection for one ray: the distance from o to where the ray meets the plane x = alt, step by step as the
// reference computes it (plane normal n = (-1, 0, 0)); `bound` is left alone unless the ray starts before the plane and goes down.
__device__ __forceinline__ float plane_bound(RayVec o, RayVec d, float alt, float bound) {
#pragma clang fp contract(off)
  if (!(o.x < alt && d.x > 0.f)) return bound;
  const float ndotu = -d.x;                                   // d . n
  const float wx = o.x - alt, wy = o.y, wz = o.z;             // w = o - (alt, 0, 0)
  const float si = -(-wx) / ndotu;                            // -(w . n) / (d . n)
  const float px = (wx + si * d.x) + alt;                     // p = w + si d + (alt, 0, 0)
  const float py = wy + si * d.y;
  const float pz = wz + si * d.z;
  return ray_norm(o.x - px, o.y - py, o.z - pz);
}

// _get_rays_inner: near / far, truncated by the two altitude planes and clamped.
__device__ __forceinline__ void ray_bounds(RayVec o, RayVec d, const RayBounds& b, float& near, float& far) {
  near = b.near;
  far = b.far;
  if (b.has_alt) {
    near = fmaxf(plane_bound(o, d, b.alt_near, near), b.near);
    far = fminf(plane_bound(o, d, b.alt_far, far), b.far);
    far = fmaxf(near, far);
  }
}

__device__ __forceinline__ void store_ray(float* __restrict__ rays, size_t r, RayVec o, RayVec d, float near, float far) {
  float4* p = reinterpret_cast<float4*>(rays + r * 8);
  p[0] = make_float4(o.x, o.y, o.z, d.x);
  p[1] = make_float4(d.y, d.z, near, far);
}

__device__ __forceinline__ void world_ray(RayVec dir, const RayPose& c, const RayBounds& b, float* __restrict__ rays, size_t r) {
  const RayVec o = {c.m[3], c.m[7], c.m[11]};
  const RayVec d = rotate_direction(dir, c);
  float near, far;
  ray_bounds(o, d, b, near, far);
  store_ray(rays, r, o, d, near, far);
}

struct RayCamera {
  RayPose pose;
  float fx, fy, cx, cy;
  int W, center_pixels;
};

__global__ __launch_bounds__(RAY_THREADS) void rays_from_camera_kernel(RayCamera cam, RayBounds b, long pixel_begin, long n,
                                                                      long image_index, float* __restrict__ rays,
                                                                      int64_t* __restrict__ image_indices) {
  const long i = (long)blockIdx.x * RAY_THREADS + threadIdx.x;
  if (i >= n) return;
  const long p = pixel_begin + i;
  const RayVec dir = pixel_direction((int)(p % cam.W), (int)(p / cam.W), cam.fx, cam.fy, cam.cx, cam.cy, cam.center_pixels);
  world_ray(dir, cam.pose, b, rays, (size_t)i);
  if (image_indices) image_indices[i] = image_index;
}

__global__ __launch_bounds__(RAY_THREADS) void ray_directions_kernel(int W, long n, float fx, float fy, float cx, float cy,
                                                                    int center_pixels, float* __restrict__ dirs) {
  const long i = (long)blockIdx.x * RAY_THREADS + threadIdx.x;
  if (i >= n) return;
  const RayVec d = pixel_direction((int)(i % W), (int)(i / W), fx, fy, cx, cy, center_pixels);
  float* o = dirs + (size_t)i * 3;
  o[0] = d.x;
  o[1] = d.y;
  o[2] = d.z;
}

__device__ __forceinline__ RayPose load_pose(const float* __restrict__ c2w) {      // 12 floats, 16-byte aligned
  const float4* q = reinterpret_cast<const float4*>(c2w);
  const float4 a = q[0], b = q[1], c = q[2];
  return {{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w}};
}

// blockIdx.y = the camera; rays[cam][i] from dirs[i]
__global__ __launch_bounds__(RAY_THREADS) void rays_from_directions_kernel(const float* __restrict__ dirs, const float* __restrict__ c2w,
                                                                          RayBounds b, long n, float* __restrict__ rays) {
  const long i = (long)blockIdx.x * RAY_THREADS + threadIdx.x;
  if (i >= n) return;
  const RayPose pose = load_pose(c2w + (size_t)blockIdx.y * 12);
  const float* s = dirs + (size_t)i * 3;
  world_ray({s[0], s[1], s[2]}, pose, b, rays, (size_t)blockIdx.y * n + i);
}

template <typename I>
__global__ __launch_bounds__(RAY_THREADS) void rays_from_pixels_kernel(const float* __restrict__ table, const I* __restrict__ cam_idx,
                                                                      const I* __restrict__ pix_idx, long n, int W, int center_pixels,
                                                                      RayBounds b, float* __restrict__ rays) {
  const long i = (long)blockIdx.x * RAY_THREADS + threadIdx.x;
  if (i >= n) return;
  const float* row = table + (size_t)cam_idx[i] * 16;        // c2w [3][4], then fx, fy, cx, cy
  const RayPose pose = load_pose(row);
  const float4 k = reinterpret_cast<const float4*>(row)[3];
  const long p = (long)pix_idx[i];
  const RayVec dir = pixel_direction((int)(p % W), (int)(p / W), k.x, k.y, k.z, k.w, center_pixels);
  world_ray(dir, pose, b, rays, (size_t)i);
}

// The checks every entry shares; -1 with the error text on a refusal.  altitude_range: two floats in HOST memory, or NULL.
static int ray_bounds_arg(const char* who, float near, float far, const float* altitude_range, RayBounds* b) {
  if (!(near <= far)) {
    set_error("%s: near %g > far %g", who, (double)near, (double)far);
    return -1;
  }
  *b = {near, far, 0.f, 0.f, 0};
  if (altitude_range) {
    if (!(altitude_range[0] < altitude_range[1])) {
      set_error("%s: the altitude pair must be ascending, got (%g, %g)", who, (double)altitude_range[0], (double)altitude_range[1]);
      return -1;
    }
    b->alt_near = altitude_range[0];
    b->alt_far = altitude_range[1];
    b->has_alt = 1;
  }
  return 0;
}

#define SWN_RAY_CHECK(cond, ...)  \
  do {                            \
    if (!(cond)) {                \
      swn::set_error(__VA_ARGS__); \
      return -1;                  \
    }                             \
  } while (0)

constexpr long RAY_MAX_N = 0x7fffffffL * RAY_THREADS;       // gridDim.x

}  // namespace swn

using namespace swn;

extern "C" int swn_rays_from_camera(const swn_camera* camera, float near, float far, const float* altitude_range, long pixel_begin,
                                    long n, float* rays, int64_t* image_indices, void* stream) {
  SWN_RAY_CHECK(camera && rays, "swn_rays_from_camera: null pointer");
  SWN_RAY_CHECK(n > 0 && n <= RAY_MAX_N, "swn_rays_from_camera: n must be positive, got %ld", n);
  SWN_RAY_CHECK(camera->W >= 1 && camera->H >= 1, "swn_rays_from_camera: bad image size (W %d, H %d)", camera->W, camera->H);
  const long pixels = (long)camera->W * camera->H;
  SWN_RAY_CHECK(pixel_begin >= 0 && pixel_begin < pixels && n <= pixels - pixel_begin,
                "swn_rays_from_camera: pixel range [%ld, %ld) outside the image's %ld pixels", pixel_begin, pixel_begin + n, pixels);
  SWN_RAY_CHECK((uintptr_t)rays % 16 == 0 && (uintptr_t)image_indices % 8 == 0, "swn_rays_from_camera: misaligned pointer");
  RayBounds b;
  if (ray_bounds_arg("swn_rays_from_camera", near, far, altitude_range, &b)) return -1;
  RayCamera cam;
  for (int k = 0; k < 12; ++k) cam.pose.m[k] = camera->c2w[k];
  cam.fx = camera->fx, cam.fy = camera->fy, cam.cx = camera->cx, cam.cy = camera->cy;
  cam.W = camera->W, cam.center_pixels = camera->center_pixels;
  hipLaunchKernelGGL(rays_from_camera_kernel, dim3(cdiv(n, RAY_THREADS)), dim3(RAY_THREADS), 0, as_stream(stream), cam, b, pixel_begin, n,
                     (long)camera->image_index, rays, image_indices);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_ray_directions(int W, int H, float fx, float fy, float cx, float cy, int center_pixels, float* directions,
                                  void* stream) {
  SWN_RAY_CHECK(directions, "swn_ray_directions: null pointer");
  SWN_RAY_CHECK(W >= 1 && H >= 1, "swn_ray_directions: bad image size (W %d, H %d)", W, H);
  SWN_RAY_CHECK((uintptr_t)directions % 4 == 0, "swn_ray_directions: misaligned pointer");
  const long n = (long)W * H;
  SWN_RAY_CHECK(n <= RAY_MAX_N, "swn_ray_directions: too many pixels");
  hipLaunchKernelGGL(ray_directions_kernel, dim3(cdiv(n, RAY_THREADS)), dim3(RAY_THREADS), 0, as_stream(stream), W, n, fx, fy, cx, cy,
                     center_pixels, directions);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_rays_from_directions(const float* directions, const float* c2w, int n_cameras, long n, float near, float far,
                                        const float* altitude_range, float* rays, void* stream) {
  SWN_RAY_CHECK(directions && c2w && rays, "swn_rays_from_directions: null pointer");
  SWN_RAY_CHECK(n > 0 && n <= RAY_MAX_N, "swn_rays_from_directions: n must be positive, got %ld", n);
  SWN_RAY_CHECK(n_cameras >= 1 && n_cameras <= 65535, "swn_rays_from_directions: 1 to 65535 cameras, got %d", n_cameras);
  SWN_RAY_CHECK((uintptr_t)rays % 16 == 0 && (uintptr_t)c2w % 16 == 0 && (uintptr_t)directions % 4 == 0,
                "swn_rays_from_directions: misaligned pointer");
  RayBounds b;
  if (ray_bounds_arg("swn_rays_from_directions", near, far, altitude_range, &b)) return -1;
  hipLaunchKernelGGL(rays_from_directions_kernel, dim3(cdiv(n, RAY_THREADS), n_cameras), dim3(RAY_THREADS), 0, as_stream(stream),
                     directions, c2w, b, n, rays);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_rays_from_pixels(const float* camera_table, int n_cameras, const void* cam_idx, const void* pix_idx, int idx_is_i64,
                                    long n, int W, int H, int center_pixels, float near, float far, const float* altitude_range,
                                    float* rays, void* stream) {
  SWN_RAY_CHECK(camera_table && cam_idx && pix_idx && rays, "swn_rays_from_pixels: null pointer");
  SWN_RAY_CHECK(n > 0 && n <= RAY_MAX_N, "swn_rays_from_pixels: n must be positive, got %ld", n);
  SWN_RAY_CHECK(n_cameras >= 1 && W >= 1 && H >= 1, "swn_rays_from_pixels: bad sizes (cameras %d, W %d, H %d)", n_cameras, W, H);
  SWN_RAY_CHECK(idx_is_i64 || (long)W * H <= 0x7fffffffL, "swn_rays_from_pixels: pixel range of %ld pixels outside int32 indices",
                (long)W * H);
  const uintptr_t idx_align = idx_is_i64 ? 8 : 4;
  SWN_RAY_CHECK((uintptr_t)rays % 16 == 0 && (uintptr_t)camera_table % 16 == 0 && (uintptr_t)cam_idx % idx_align == 0 &&
                    (uintptr_t)pix_idx % idx_align == 0,
                "swn_rays_from_pixels: misaligned pointer");
  RayBounds b;
  if (ray_bounds_arg("swn_rays_from_pixels", near, far, altitude_range, &b)) return -1;
  const dim3 grid(cdiv(n, RAY_THREADS)), block(RAY_THREADS);
  if (idx_is_i64)
    hipLaunchKernelGGL(rays_from_pixels_kernel<int64_t>, grid, block, 0, as_stream(stream), camera_table, (const int64_t*)cam_idx,
                       (const int64_t*)pix_idx, n, W, center_pixels, b, rays);
  else
    hipLaunchKernelGGL(rays_from_pixels_kernel<int32_t>, grid, block, 0, as_stream(stream), camera_table, (const int32_t*)cam_idx,
                       (const int32_t*)pix_idx, n, W, center_pixels, b, rays);
  SWN_LAUNCH_CHECK();
  return 0;
}
