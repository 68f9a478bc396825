// Rays the NeRF-dataset way on the device: the reference's datasets/nerf_data (ray_utils.get_rays :14-24, ndc_rays :27-46,
// nerf_loader.py :155-177, load_bungee.get_bungee_nearfar_radii :44-90) in fp32, one thread per pixel, outside any autocast.
//   nerf_rays_from_camera_kernel   one camera by value: pixel -> camera direction -> world direction -> mode -> rays[n, 8] (and radii[n]
//                                  in the bungee modes); no [H, W, 3] directions reach memory
//   nerf_rays_from_pixels_kernel   the gather form of a training batch: (camera index, pixel index) per ray, cameras from a table
//   nerf_rays_dirs_kernel          get_rays as the reference's first step: raw rays_o / rays_d [H, W, 3]
//   nerf_ndc_kernel                ndc_rays over [n, 3] origins and directions
// Every kernel goes through the SAME helpers (nerf_world_dir, nerf_normalize, nerf_ndc, nerf_flat, nerf_sphere, nerf_radius), contraction
// off inside them, IEEE division and square root: the same pixel of the same camera gives the same bits through every entry.  The one
// fused operation is written out: torch.norm's CPU kernel accumulates acc + v * v as ONE fused multiply-add per element, so the norm of
// the NORMALIZED directions is sqrt(fma(z, z, fma(y, y, x * x))) - explicit fmaf, not a contraction the compiler may or may not make.
// The pixel's corner is used (no + 0.5) and the camera direction is not normalised, unlike raygen.hip's Mega-NeRF convention.
// The sphere form's distance along the ray subtracts squares of the order of the scaled earth radius: it is formed in fp64 from the fp32
// origin, direction and globe centre (a few operations per ray) and rounded to fp32 once.  No LDS, no atomics.
#include <cmath>

#include "common.hpp"

namespace swn {

constexpr int NERF_RAY_THREADS = 256;

struct NerfVec { float x, y, z; };
struct NerfCam {                            // c2w [3][4] row-major (columns 0..2 the rotation, column 3 the origin), then K's used entries
  float m[12];
  float fx, fy, cx, cy;
};
struct NerfParams {
  int mode, W, H;
  float near, far;                          // columns 6, 7 of RAW / NORMALIZED / NDC
  float cw, ch, near_ndc, near2;            // NDC: -1 / (W / (2 focal)), -1 / (H / (2 focal)), near, 2 near (host doubles, rounded once)
  float scale, p_near;                      // flat: the plane normal's z (= the scale) and the upper plane's z (250 * scale)
  float gx, gy, gz;                         // sphere: the globe centre, fp32 as the reference rounds it
  double r2_near, r2_far;                   // sphere: the squared radii (earth + 250 m, earth), scaled
};

// get_rays for the pixel (col, row): c = ((i - cx) / fx, -(j - cy) / fy, -1), each world component (c0 r0 + c1 r1) + c2 r2.
__device__ __forceinline__ NerfVec nerf_world_dir(int col, int row, const NerfCam& c) {
#pragma clang fp contract(off)
  const float x = ((float)col - c.cx) / c.fx;
  const float y = -((float)row - c.cy) / c.fy;
  const float z = -1.f;
  return {(x * c.m[0] + y * c.m[1]) + z * c.m[2], (x * c.m[4] + y * c.m[5]) + z * c.m[6], (x * c.m[8] + y * c.m[9]) + z * c.m[10]};
}

// rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
__device__ __forceinline__ NerfVec nerf_normalize(NerfVec d) {
#pragma clang fp contract(off)
  const float xx = d.x * d.x;
  const float n = sqrtf(fmaf(d.z, d.z, fmaf(d.y, d.y, xx)));
  return {d.x / n, d.y / n, d.z / n};
}

__device__ __forceinline__ float nerf_plain_norm(float x, float y, float z) {
#pragma clang fp contract(off)
  const float xx = x * x, yy = y * y, zz = z * z;
  return sqrtf((xx + yy) + zz);
}

// ndc_rays, statement by statement
__device__ __forceinline__ void nerf_ndc(NerfVec& o, NerfVec& d, const NerfParams& p) {
#pragma clang fp contract(off)
  const float t = -(p.near_ndc + o.z) / d.z;
  const float tx = t * d.x, ty = t * d.y, tz = t * d.z;
  const float ox = o.x + tx, oy = o.y + ty, oz = o.z + tz;
  const float o0 = (p.cw * ox) / oz;
  const float o1 = (p.ch * oy) / oz;
  const float o2 = 1.f + p.near2 / oz;
  const float d0 = p.cw * (d.x / d.z - ox / oz);
  const float d1 = p.ch * (d.y / d.z - oy / oz);
  const float d2 = -p.near2 / oz;
  o = {o0, o1, o2};
  d = {d0, d1, d2};
}

// 'flat': the two planes z = 250 * scale and z = 0 with the normal (0, 0, scale); the x and y terms of the reference's sums are zeros
__device__ __forceinline__ void nerf_flat(NerfVec o, NerfVec d, const NerfParams& p, float& near, float& far) {
#pragma clang fp contract(off)
  const float den = d.z * p.scale;
  const float oz = o.z * p.scale;
  near = fmaxf((p.p_near - oz) / den, 1e-6f);
  far = (0.f - oz) / den;
}

// 'sphere': |o - (o + dist d)| with dist the nearer intersection of the ray and the sphere of squared radius r2 about the globe centre
__device__ __forceinline__ float nerf_sphere(NerfVec o, NerfVec d, const NerfParams& p, double r2) {
#pragma clang fp contract(off)
  const double dx = (double)d.x, dy = (double)d.y, dz = (double)d.z;
  const double cx = (double)o.x - (double)p.gx, cy = (double)o.y - (double)p.gy, cz = (double)o.z - (double)p.gz;
  const double b = 2.0 * ((cx * dx + cy * dy) + cz * dz);
  const double n2 = (dx * dx + dy * dy) + dz * dz;
  const double c2 = (cx * cx + cy * cy) + cz * cz;
  const double delta = b * b - (4.0 * n2) * (c2 - r2);
  const float dist = (float)((-b - sqrt(delta)) / (2.0 * n2));
  const float sx = dist * d.x, sy = dist * d.y, sz = dist * d.z;
  const float px = o.x + sx, py = o.y + sy, pz = o.z + sz;
  return nerf_plain_norm(o.x - px, o.y - py, o.z - pz);
}

// radii: dx(row) = |d(row) - d(row + 1)| for row < H - 1; the last row takes dx(H - 3), the reference's cat([dx, dx[:, -2:-1]]) over
// dx's H - 1 rows (H == 2: dx(0), the only one).  The neighbours' directions are recomputed, so a pixel range may start anywhere.
__device__ __forceinline__ float nerf_radius(int col, int row, NerfVec self, const NerfCam& c, int H) {
#pragma clang fp contract(off)
  const int k = row < H - 1 ? row : (H >= 3 ? H - 3 : 0);
  const NerfVec a = k == row ? self : nerf_normalize(nerf_world_dir(col, k, c));
  const NerfVec b = k + 1 == row ? self : nerf_normalize(nerf_world_dir(col, k + 1, c));
  const float dx = nerf_plain_norm(a.x - b.x, a.y - b.y, a.z - b.z);
  return (dx * 2.f) / (float)3.4641016151377544;          // 2 / np.sqrt(12): the product, then the division by fp32(sqrt(12))
}

enum { NERF_RAW = 0, NERF_NORMALIZED = 1, NERF_NDC = 2, NERF_BUNGEE_SPHERE = 3, NERF_BUNGEE_FLAT = 4 };

__device__ __forceinline__ void nerf_pixel(const NerfCam& c, const NerfParams& p, long pix, float* __restrict__ rays,
                                           float* __restrict__ radii, size_t i) {
#pragma clang fp contract(off)
  const int col = (int)(pix % p.W), row = (int)(pix / p.W);
  NerfVec o = {c.m[3], c.m[7], c.m[11]};
  NerfVec d = nerf_world_dir(col, row, c);
  float near = p.near, far = p.far;
  if (p.mode == NERF_NDC) {
    nerf_ndc(o, d, p);
  } else if (p.mode != NERF_RAW) {
    d = nerf_normalize(d);
    if (p.mode == NERF_BUNGEE_SPHERE) {
      near = nerf_sphere(o, d, p, p.r2_near) * 0.9f;
      far = nerf_sphere(o, d, p, p.r2_far) * 1.1f;
    } else if (p.mode == NERF_BUNGEE_FLAT) {
      nerf_flat(o, d, p, near, far);
    }
    if (p.mode != NERF_NORMALIZED) radii[i] = nerf_radius(col, row, d, c, p.H);
  }
  float4* q = reinterpret_cast<float4*>(rays + i * 8);
  q[0] = make_float4(o.x, o.y, o.z, d.x);
  q[1] = make_float4(d.y, d.z, near, far);
}

__device__ __forceinline__ NerfCam nerf_load_cam(const float* __restrict__ row) {      // 16 floats, 16-byte aligned
  const float4* q = reinterpret_cast<const float4*>(row);
  const float4 a = q[0], b = q[1], c = q[2], k = q[3];
  return {{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w}, k.x, k.y, k.z, k.w};
}

__global__ __launch_bounds__(NERF_RAY_THREADS) void nerf_rays_from_camera_kernel(NerfCam cam, NerfParams p, long pixel_begin, long n,
                                                                                float* __restrict__ rays, float* __restrict__ radii) {
  const long i = (long)blockIdx.x * NERF_RAY_THREADS + threadIdx.x;
  if (i >= n) return;
  nerf_pixel(cam, p, pixel_begin + i, rays, radii, (size_t)i);
}

template <typename I>
__global__ __launch_bounds__(NERF_RAY_THREADS) void nerf_rays_from_pixels_kernel(const float* __restrict__ table,
                                                                                const I* __restrict__ cam_idx,
                                                                                const I* __restrict__ pix_idx, long n, NerfParams p,
                                                                                float* __restrict__ rays, float* __restrict__ radii) {
  const long i = (long)blockIdx.x * NERF_RAY_THREADS + threadIdx.x;
  if (i >= n) return;
  const NerfCam cam = nerf_load_cam(table + (size_t)cam_idx[i] * 16);
  nerf_pixel(cam, p, (long)pix_idx[i], rays, radii, (size_t)i);
}

__global__ __launch_bounds__(NERF_RAY_THREADS) void nerf_rays_dirs_kernel(const float* __restrict__ camera_row, int W, long n,
                                                                         float* __restrict__ rays_o, float* __restrict__ rays_d) {
  const long i = (long)blockIdx.x * NERF_RAY_THREADS + threadIdx.x;
  if (i >= n) return;
  const NerfCam cam = nerf_load_cam(camera_row);
  const NerfVec d = nerf_world_dir((int)(i % W), (int)(i / W), cam);
  float* o = rays_o + (size_t)i * 3;
  float* q = rays_d + (size_t)i * 3;
  o[0] = cam.m[3], o[1] = cam.m[7], o[2] = cam.m[11];
  q[0] = d.x, q[1] = d.y, q[2] = d.z;
}

__global__ __launch_bounds__(NERF_RAY_THREADS) void nerf_ndc_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                                   long n, NerfParams p, float* __restrict__ out_o,
                                                                   float* __restrict__ out_d) {
  const long i = (long)blockIdx.x * NERF_RAY_THREADS + threadIdx.x;
  if (i >= n) return;
  const float* so = rays_o + (size_t)i * 3;
  const float* sd = rays_d + (size_t)i * 3;
  NerfVec o = {so[0], so[1], so[2]}, d = {sd[0], sd[1], sd[2]};
  nerf_ndc(o, d, p);
  float* qo = out_o + (size_t)i * 3;
  float* qd = out_d + (size_t)i * 3;
  qo[0] = o.x, qo[1] = o.y, qo[2] = o.z;
  qd[0] = d.x, qd[1] = d.y, qd[2] = d.z;
}

#define SWN_NERF_CHECK(cond, ...)  \
  do {                             \
    if (!(cond)) {                 \
      swn::set_error(__VA_ARGS__); \
      return -1;                   \
    }                              \
  } while (0)

constexpr long NERF_RAY_MAX_N = 0x7fffffffL * NERF_RAY_THREADS;       // gridDim.x

// The host half of ndc_rays: the reference forms -1. / (W / (2. * focal)) and 2. * near in Python doubles; a tensor operand rounds each
// to fp32 once.
static int nerf_ndc_params(const char* who, int W, int H, double focal, double near_ndc, NerfParams* p) {
  if (!(focal > 0.0) || !std::isfinite(focal) || !std::isfinite(near_ndc)) {
    set_error("%s: NDC needs a positive finite focal and a finite near, got focal %g near %g", who, focal, near_ndc);
    return -1;
  }
  p->cw = (float)(-1. / (W / (2. * focal)));
  p->ch = (float)(-1. / (H / (2. * focal)));
  p->near_ndc = (float)near_ndc;
  p->near2 = (float)(2. * near_ndc);
  return 0;
}

// The host half of get_bungee_nearfar_radii: the globe centre (scene_origin * scale, rounded to fp32 as .float() does), the two scaled
// radii squared (doubles), the flat form's plane constants in fp32.
static int nerf_bungee_params(const char* who, int H, double scale, const double* scene_origin, int ray_nearfar, NerfParams* p) {
  if (H < 2) {
    set_error("%s: the bungee radii need two image rows, got H %d", who, H);
    return -1;
  }
  if (ray_nearfar != SWN_NERF_SPHERE && ray_nearfar != SWN_NERF_FLAT) {
    set_error("%s: ray_nearfar must be SWN_NERF_SPHERE or SWN_NERF_FLAT, got %d", who, ray_nearfar);
    return -1;
  }
  if (!(scale > 0.0) || !std::isfinite(scale)) {
    set_error("%s: scene_scaling_factor must be positive and finite, got %g", who, scale);
    return -1;
  }
  if (ray_nearfar == SWN_NERF_SPHERE) {
    if (!scene_origin) {
      set_error("%s: null pointer (scene_origin)", who);
      return -1;
    }
    p->gx = (float)(scene_origin[0] * scale), p->gy = (float)(scene_origin[1] * scale), p->gz = (float)(scene_origin[2] * scale);
    const double r_far = 6371011 * scale, r_near = (6371011 + 250) * scale;
    p->r2_near = r_near * r_near;
    p->r2_far = r_far * r_far;
    p->mode = NERF_BUNGEE_SPHERE;
  } else {
    p->scale = (float)scale;
    p->p_near = 250.f * p->scale;
    p->mode = NERF_BUNGEE_FLAT;
  }
  return 0;
}

// mode (and what it needs) -> params; -1 with the error text on a refusal
static int nerf_mode_params(const char* who, int mode, int W, int H, float near, float far, double focal, double near_ndc, double scale,
                            const double* scene_origin, NerfParams* p) {
  *p = NerfParams{};
  p->W = W, p->H = H, p->near = near, p->far = far;
  switch (mode) {
    case SWN_NERF_RAW: p->mode = NERF_RAW; break;
    case SWN_NERF_NORMALIZED: p->mode = NERF_NORMALIZED; break;
    case SWN_NERF_NDC:
      p->mode = NERF_NDC;
      if (nerf_ndc_params(who, W, H, focal, near_ndc, p)) return -1;
      break;
    case SWN_NERF_BUNGEE_SPHERE: return nerf_bungee_params(who, H, scale, scene_origin, SWN_NERF_SPHERE, p);
    case SWN_NERF_BUNGEE_FLAT: return nerf_bungee_params(who, H, scale, scene_origin, SWN_NERF_FLAT, p);
    default: set_error("%s: unknown mode %d", who, mode); return -1;
  }
  if (!(near <= far)) {
    set_error("%s: near %g > far %g", who, (double)near, (double)far);
    return -1;
  }
  return 0;
}

static NerfCam nerf_cam(const swn_nerf_camera* camera) {
  NerfCam c;
  for (int k = 0; k < 12; ++k) c.m[k] = camera->c2w[k];
  c.fx = camera->fx, c.fy = camera->fy, c.cx = camera->cx, c.cy = camera->cy;
  return c;
}

// the checks the two by-value entries share
static int nerf_camera_range(const char* who, const swn_nerf_camera* camera, long pixel_begin, long n, const float* rays) {
  if (!camera || !rays) {
    set_error("%s: null pointer", who);
    return -1;
  }
  if (!(n > 0 && n <= NERF_RAY_MAX_N)) {
    set_error("%s: n must be positive, got %ld", who, n);
    return -1;
  }
  if (!(camera->W >= 1 && camera->H >= 1)) {
    set_error("%s: bad image size (W %d, H %d)", who, camera->W, camera->H);
    return -1;
  }
  const long pixels = (long)camera->W * camera->H;
  if (!(pixel_begin >= 0 && pixel_begin < pixels && n <= pixels - pixel_begin)) {
    set_error("%s: pixel range [%ld, %ld) outside the image's %ld pixels", who, pixel_begin, pixel_begin + n, pixels);
    return -1;
  }
  if ((uintptr_t)rays % 16) {
    set_error("%s: misaligned pointer", who);
    return -1;
  }
  return 0;
}

}  // namespace swn

using namespace swn;

extern "C" int swn_nerf_rays_from_camera(const swn_nerf_camera* camera, int mode, float near, float far, double focal, double near_ndc,
                                         long pixel_begin, long n, float* rays, void* stream) {
  const char* who = "swn_nerf_rays_from_camera";
  if (nerf_camera_range(who, camera, pixel_begin, n, rays)) return -1;
  SWN_NERF_CHECK(mode == SWN_NERF_RAW || mode == SWN_NERF_NORMALIZED || mode == SWN_NERF_NDC,
                 "%s: mode must be SWN_NERF_RAW, SWN_NERF_NORMALIZED or SWN_NERF_NDC, got %d", who, mode);
  NerfParams p;
  if (nerf_mode_params(who, mode, camera->W, camera->H, near, far, focal, near_ndc, 0.0, nullptr, &p)) return -1;
  hipLaunchKernelGGL(nerf_rays_from_camera_kernel, dim3(cdiv(n, NERF_RAY_THREADS)), dim3(NERF_RAY_THREADS), 0, as_stream(stream),
                     nerf_cam(camera), p, pixel_begin, n, rays, (float*)nullptr);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_nerf_rays_bungee(const swn_nerf_camera* camera, double scene_scaling_factor, const double* scene_origin,
                                    int ray_nearfar, long pixel_begin, long n, float* rays, float* radii, void* stream) {
  const char* who = "swn_nerf_rays_bungee";
  if (nerf_camera_range(who, camera, pixel_begin, n, rays)) return -1;
  SWN_NERF_CHECK(radii, "%s: null pointer", who);
  SWN_NERF_CHECK((uintptr_t)radii % 4 == 0, "%s: misaligned pointer", who);
  NerfParams p = NerfParams{};
  p.W = camera->W, p.H = camera->H;
  if (nerf_bungee_params(who, camera->H, scene_scaling_factor, scene_origin, ray_nearfar, &p)) return -1;
  hipLaunchKernelGGL(nerf_rays_from_camera_kernel, dim3(cdiv(n, NERF_RAY_THREADS)), dim3(NERF_RAY_THREADS), 0, as_stream(stream),
                     nerf_cam(camera), p, pixel_begin, n, rays, radii);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_nerf_rays_from_pixels(const float* camera_table, int n_cameras, const void* cam_idx, const void* pix_idx, int idx_is_i64,
                                         long n, int W, int H, int mode, float near, float far, double focal, double near_ndc,
                                         double scene_scaling_factor, const double* scene_origin, float* rays, float* radii,
                                         void* stream) {
  const char* who = "swn_nerf_rays_from_pixels";
  SWN_NERF_CHECK(camera_table && cam_idx && pix_idx && rays, "%s: null pointer", who);
  SWN_NERF_CHECK(n > 0 && n <= NERF_RAY_MAX_N, "%s: n must be positive, got %ld", who, n);
  SWN_NERF_CHECK(n_cameras >= 1 && W >= 1 && H >= 1, "%s: bad sizes (cameras %d, W %d, H %d)", who, n_cameras, W, H);
  SWN_NERF_CHECK(idx_is_i64 || (long)W * H <= 0x7fffffffL, "%s: pixel range of %ld pixels outside int32 indices", who, (long)W * H);
  const bool bungee = mode == SWN_NERF_BUNGEE_SPHERE || mode == SWN_NERF_BUNGEE_FLAT;
  SWN_NERF_CHECK(!bungee || radii, "%s: null pointer (the bungee modes write radii)", who);
  const uintptr_t idx_align = idx_is_i64 ? 8 : 4;
  SWN_NERF_CHECK((uintptr_t)rays % 16 == 0 && (uintptr_t)camera_table % 16 == 0 && (uintptr_t)cam_idx % idx_align == 0 &&
                     (uintptr_t)pix_idx % idx_align == 0 && (uintptr_t)radii % 4 == 0,
                 "%s: misaligned pointer", who);
  NerfParams p;
  if (nerf_mode_params(who, mode, W, H, near, far, focal, near_ndc, scene_scaling_factor, scene_origin, &p)) return -1;
  const dim3 grid(cdiv(n, NERF_RAY_THREADS)), block(NERF_RAY_THREADS);
  float* rad = bungee ? radii : nullptr;
  if (idx_is_i64)
    hipLaunchKernelGGL(nerf_rays_from_pixels_kernel<int64_t>, grid, block, 0, as_stream(stream), camera_table, (const int64_t*)cam_idx,
                       (const int64_t*)pix_idx, n, p, rays, rad);
  else
    hipLaunchKernelGGL(nerf_rays_from_pixels_kernel<int32_t>, grid, block, 0, as_stream(stream), camera_table, (const int32_t*)cam_idx,
                       (const int32_t*)pix_idx, n, p, rays, rad);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_nerf_rays_dirs(const float* camera_row, int W, int H, float* rays_o, float* rays_d, void* stream) {
  const char* who = "swn_nerf_rays_dirs";
  SWN_NERF_CHECK(camera_row && rays_o && rays_d, "%s: null pointer", who);
  SWN_NERF_CHECK(W >= 1 && H >= 1, "%s: bad image size (W %d, H %d)", who, W, H);
  SWN_NERF_CHECK((uintptr_t)camera_row % 16 == 0 && (uintptr_t)rays_o % 4 == 0 && (uintptr_t)rays_d % 4 == 0, "%s: misaligned pointer", who);
  const long n = (long)W * H;
  SWN_NERF_CHECK(n <= NERF_RAY_MAX_N, "%s: too many pixels", who);
  hipLaunchKernelGGL(nerf_rays_dirs_kernel, dim3(cdiv(n, NERF_RAY_THREADS)), dim3(NERF_RAY_THREADS), 0, as_stream(stream), camera_row, W, n,
                     rays_o, rays_d);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_nerf_ndc(const float* rays_o, const float* rays_d, long n, int W, int H, double focal, double near, float* out_o,
                            float* out_d, void* stream) {
  const char* who = "swn_nerf_ndc";
  SWN_NERF_CHECK(rays_o && rays_d && out_o && out_d, "%s: null pointer", who);
  SWN_NERF_CHECK(n > 0 && n <= NERF_RAY_MAX_N, "%s: n must be positive, got %ld", who, n);
  SWN_NERF_CHECK(W >= 1 && H >= 1, "%s: bad image size (W %d, H %d)", who, W, H);
  SWN_NERF_CHECK((uintptr_t)rays_o % 4 == 0 && (uintptr_t)rays_d % 4 == 0 && (uintptr_t)out_o % 4 == 0 && (uintptr_t)out_d % 4 == 0,
                 "%s: misaligned pointer", who);
  NerfParams p = NerfParams{};
  p.W = W, p.H = H, p.mode = NERF_NDC;
  if (nerf_ndc_params(who, W, H, focal, near, &p)) return -1;
  hipLaunchKernelGGL(nerf_ndc_kernel, dim3(cdiv(n, NERF_RAY_THREADS)), dim3(NERF_RAY_THREADS), 0, as_stream(stream), rays_o, rays_d, n, p,
                     out_o, out_d);
  SWN_LAUNCH_CHECK();
  return 0;
}
