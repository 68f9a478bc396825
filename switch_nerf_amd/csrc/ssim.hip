// Image metrics of the validation loop on the device (the reference's metrics.py: psnr :8-10, ssim :51-121, psnr_mask / ssim_mask
// :124-208): SSIM with a separable Gaussian window over zero-padded images, and the squared error next to it, in one pass over the
// two images.
//   ssim_tile_kernel     one workgroup per image and tile of SWN_SSIM_TILE^2 output pixels; channel by channel: tile + halo of both
//                        images into LDS (zeros outside the image), the pass along the last spatial axis of x, y, x^2, y^2, xy into
//                        LDS, the pass along the first axis out of LDS into registers, the per-pixel formula, the tile's five sums to
//                        its own slot.  The blurred fields never leave the CU.
//   ssim_reduce_kernel   one workgroup per image: the tiles' sums in ascending tile order in a fixed association -> the four means.
// No atomics: every slot has one writer, every sum a fixed order, so the result is the same bits on every run.
#include "common.hpp"

namespace swn {

constexpr int SSIM_TILE = SWN_SSIM_TILE;      // output pixels per tile edge
constexpr int SSIM_THREADS = 256;
constexpr int SSIM_RUN = 4;        // consecutive outputs one thread carries along the axis of a pass (register sliding window)
constexpr int SSIM_MAX_TAPS = 15;
static_assert(SSIM_THREADS / SSIM_TILE * SSIM_RUN == SSIM_TILE, "the second pass gives every thread one column and SSIM_RUN rows");

struct SsimTaps { float w[SSIM_MAX_TAPS]; };

// The reference's per-pixel expression, each product and sum rounded on its own as torch's elementwise ops round them.
__device__ __forceinline__ float ssim_pixel(float mu0, float mu1, float exx, float eyy, float exy, float c1, float c2) {
#pragma clang fp contract(off)
  const float mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
  const float s00 = fmaxf(exx - mu00, 0.f), s11 = fmaxf(eyy - mu11, 0.f);
  float s01 = exy - mu01;
  const float lim = fminf(sqrtf(s00 * s11), fabsf(s01));
  s01 = s01 > 0.f ? lim : (s01 < 0.f ? -lim : 0.f);      // sign(s01) * lim; sign(0) = 0
  const float numer = (2.f * mu01 + c1) * (2.f * s01 + c2);
  const float denom = (mu00 + mu11 + c1) * (s00 + s11 + c2);
  return numer / denom;
}

// FS taps (odd), HW = FS / 2.  LDS: the two input tiles [NR][SI] and the five row-blurred fields [NR][SH]; SI and SH are odd, so
// that lanes along rows (the first pass) land on distinct banks; the second pass has its lanes along columns.
template <int FS>
__global__ __launch_bounds__(SSIM_THREADS) void ssim_tile_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                const uint8_t* __restrict__ mask, int A, int B, int C, SsimTaps taps,
                                                                float c1, float c2, float* __restrict__ map_out,
                                                                float4* __restrict__ part, int* __restrict__ part_cnt) {
  constexpr int T = SSIM_TILE, HW = FS / 2, NR = T + 2 * HW, SI = NR | 1, SH = T + 1, R = SSIM_RUN, WIN = R + FS - 1;
  __shared__ float sx[NR * SI];
  __shared__ float sy[NR * SI];
  __shared__ float sh[5][NR * SH];
  __shared__ float red[SSIM_THREADS / 64][4];
  __shared__ int red_cnt[SSIM_THREADS / 64];

  const int tid = threadIdx.x;
  const int a0 = blockIdx.y * T, b0 = blockIdx.x * T;
  const int n_tiles = gridDim.x * gridDim.y, tile = blockIdx.y * gridDim.x + blockIdx.x;
  const size_t img_off = (size_t)blockIdx.z * A * B;           // in pixels
  const float* __restrict__ px = pred + img_off * C;
  const float* __restrict__ py = target + img_off * C;

  // this thread's outputs of the second pass: column oc, rows or0 .. or0 + R - 1 of the tile
  const int oc = tid % T, or0 = (tid / T) * R;
  const int gb = b0 + oc;
  float s_map = 0.f, s_se = 0.f, s_map_m = 0.f, s_se_m = 0.f;
  int cnt_m = 0;
  bool live[R], sel[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int ga = a0 + or0 + i;
    live[i] = ga < A && gb < B;
    sel[i] = live[i] && mask != nullptr && mask[img_off + (size_t)ga * B + gb] != 0;
    cnt_m += sel[i] ? 1 : 0;
  }

  for (int c = 0; c < C; ++c) {
    if (c) __syncthreads();                                    // the previous channel's reads of sx / sy / sh are done
    for (int i = tid; i < NR * NR; i += SSIM_THREADS) {
      const int r = i / NR, q = i % NR;
      const int ga = a0 - HW + r, gq = b0 - HW + q;
      float vx = 0.f, vy = 0.f;                                // zero padding outside the image
      if (ga >= 0 && ga < A && gq >= 0 && gq < B) {
        const size_t o = ((size_t)ga * B + gq) * C + c;
        vx = px[o];
        vy = py[o];
      }
      sx[r * SI + q] = vx;
      sy[r * SI + q] = vy;
    }
    __syncthreads();
    // the pass along the last spatial axis: item = (run of R columns, row), rows on the lanes
    for (int i = tid; i < (T / R) * NR; i += SSIM_THREADS) {
      const int r = i % NR, q0 = (i / NR) * R;
      float wx[WIN], wy[WIN];
#pragma unroll
      for (int k = 0; k < WIN; ++k) {
        wx[k] = sx[r * SI + q0 + k];
        wy[k] = sy[r * SI + q0 + k];
      }
#pragma unroll
      for (int j = 0; j < R; ++j) {
        float f0 = 0.f, f1 = 0.f, f2 = 0.f, f3 = 0.f, f4 = 0.f;
#pragma unroll
        for (int k = 0; k < FS; ++k) {
          const float w = taps.w[k], x = wx[j + k], y = wy[j + k];
          f0 = fmaf(w, x, f0);
          f1 = fmaf(w, y, f1);
          f2 = fmaf(w, x * x, f2);
          f3 = fmaf(w, y * y, f3);
          f4 = fmaf(w, x * y, f4);
        }
        const int o = r * SH + q0 + j;
        sh[0][o] = f0;
        sh[1][o] = f1;
        sh[2][o] = f2;
        sh[3][o] = f3;
        sh[4][o] = f4;
      }
    }
    __syncthreads();
    // the pass along the first axis: one column and R rows per thread, columns on the lanes
    float acc[5][R];
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      float win[WIN];
#pragma unroll
      for (int k = 0; k < WIN; ++k) win[k] = sh[f][(or0 + k) * SH + oc];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < FS; ++k) a = fmaf(taps.w[k], win[j + k], a);
        acc[f][j] = a;
      }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      if (!live[j]) continue;
      const float v = ssim_pixel(acc[0][j], acc[1][j], acc[2][j], acc[3][j], acc[4][j], c1, c2);
      const int ci = (or0 + j + HW) * SI + oc + HW;
      const float d = sx[ci] - sy[ci];
      const float se = d * d;
      s_map += v;
      s_se += se;
      if (sel[j]) {
        s_map_m += v;
        s_se_m += se;
      }
      if (map_out) map_out[(img_off + (size_t)(a0 + or0 + j) * B + gb) * C + c] = v;
    }
  }

  // the tile's sums: lanes by a fixed butterfly, the four waves in ascending order
  s_map = wave_sum(s_map);
  s_se = wave_sum(s_se);
  s_map_m = wave_sum(s_map_m);
  s_se_m = wave_sum(s_se_m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt_m += __shfl_xor(cnt_m, o, 64);
  const int wave = tid / 64;
  if (tid % 64 == 0) {
    red[wave][0] = s_map;
    red[wave][1] = s_se;
    red[wave][2] = s_map_m;
    red[wave][3] = s_se_m;
    red_cnt[wave] = cnt_m;
  }
  __syncthreads();
  if (tid == 0) {
    float4 p = {red[0][0], red[0][1], red[0][2], red[0][3]};
    int n = red_cnt[0];
#pragma unroll
    for (int w = 1; w < SSIM_THREADS / 64; ++w) {
      p.x += red[w][0];
      p.y += red[w][1];
      p.z += red[w][2];
      p.w += red[w][3];
      n += red_cnt[w];
    }
    const size_t slot = (size_t)blockIdx.z * n_tiles + tile;
    part[slot] = p;
    part_cnt[slot] = n;
  }
}

// out[img] = (mean map, mean squared error, the two means over the masked pixels; nan for an empty mask).  Thread t adds the tiles
// [t * run, (t + 1) * run) in ascending order, then the 256 run sums are added in ascending order in two levels of 16; the
// accumulators are fp64 (a validation image is some thousand tiles, and the adds are free next to the loads).
__global__ __launch_bounds__(256) void ssim_reduce_kernel(const float4* __restrict__ part, const int* __restrict__ part_cnt, int n_tiles,
                                                          double n_pixels, int C, float* __restrict__ out) {
  __shared__ double acc[256][5];
  const int t = threadIdx.x;
  const int run = (n_tiles + 255) / 256;
  const int i0 = t * run, i1 = n_tiles < i0 + run ? n_tiles : i0 + run;
  const float4* __restrict__ p = part + (size_t)blockIdx.x * n_tiles;
  const int* __restrict__ pc = part_cnt + (size_t)blockIdx.x * n_tiles;
  double s[5] = {0., 0., 0., 0., 0.};
  for (int i = i0; i < i1; ++i) {
    const float4 v = p[i];
    s[0] += v.x;
    s[1] += v.y;
    s[2] += v.z;
    s[3] += v.w;
    s[4] += (double)pc[i];                                     // exact: an integer below 2^53
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) acc[t][k] = s[k];
  __syncthreads();
  if (t < 16) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      double a = acc[t * 16][k];
      for (int j = 1; j < 16; ++j) a += acc[t * 16 + j][k];
      s[k] = a;
    }
  }
  __syncthreads();
  if (t < 16) {
#pragma unroll
    for (int k = 0; k < 5; ++k) acc[t][k] = s[k];
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      double a = acc[0][k];
      for (int j = 1; j < 16; ++j) a += acc[j][k];
      s[k] = a;
    }
    const double n_all = n_pixels * C, n_sel = s[4] * C;
    float* o = out + (size_t)blockIdx.x * 4;
    o[0] = (float)(s[0] / n_all);
    o[1] = (float)(s[1] / n_all);
    const float qnan = __uint_as_float(0x7fc00000u);
    o[2] = s[4] > 0. ? (float)(s[2] / n_sel) : qnan;
    o[3] = s[4] > 0. ? (float)(s[3] / n_sel) : qnan;
  }
}

template <int FS>
static void ssim_launch(dim3 grid, hipStream_t s, const float* pred, const float* target, const uint8_t* mask, int A, int B, int C,
                        const SsimTaps& taps, float c1, float c2, float* map_out, float4* part, int* part_cnt) {
  hipLaunchKernelGGL((ssim_tile_kernel<FS>), grid, dim3(SSIM_THREADS), 0, s, pred, target, mask, A, B, C, taps, c1, c2, map_out, part,
                     part_cnt);
}

static inline long ssim_tiles(int A, int B) { return (long)cdiv(A, SSIM_TILE) * cdiv(B, SSIM_TILE); }

}  // namespace swn

using namespace swn;

extern "C" int swn_ssim_workspace_bytes(int n_img, int A, int B, size_t* bytes) {
  SWN_CHECK(bytes, "swn_ssim_workspace_bytes: null pointer");
  SWN_CHECK(n_img >= 1 && A >= 1 && B >= 1, "swn_ssim_workspace_bytes: bad sizes (n_img %d, A %d, B %d)", n_img, A, B);
  *bytes = (size_t)n_img * ssim_tiles(A, B) * (sizeof(float4) + sizeof(int));
  return 0;
}

extern "C" int swn_ssim_fwd(const float* pred, const float* target, const uint8_t* mask, int n_img, int A, int B, int C, const float* taps,
                            int filter_size, float c1, float c2, float* map_out, void* workspace, size_t workspace_bytes, float* out,
                            void* stream) {
  if (filter_size < 1 || filter_size > SSIM_MAX_TAPS || filter_size % 2 == 0) {
    set_error("swn_ssim_fwd: filter_size must be odd and in 1..%d, got %d", SSIM_MAX_TAPS, filter_size);
    return -1;
  }
  SWN_CHECK(pred && target && taps && workspace && out, "swn_ssim_fwd: null pointer");
  SWN_CHECK(n_img >= 1 && A >= 1 && B >= 1, "swn_ssim_fwd: bad sizes (n_img %d, A %d, B %d)", n_img, A, B);
  SWN_CHECK(C >= 1 && C <= 4, "swn_ssim_fwd: 1 to 4 channels, got %d", C);
  const int ta = cdiv(A, SSIM_TILE), tb = cdiv(B, SSIM_TILE);
  SWN_CHECK(n_img <= 65535 && ta <= 65535, "swn_ssim_fwd: at most 65535 images and 65535 tiles along the first axis");
  SWN_CHECK((long)ta * tb <= 0x7fffffffL, "swn_ssim_fwd: too many tiles per image");
  const size_t n_slots = (size_t)n_img * ta * tb;
  SWN_CHECK(workspace_bytes >= n_slots * (sizeof(float4) + sizeof(int)), "swn_ssim_fwd: workspace of %zu bytes, need %zu", workspace_bytes,
            n_slots * (sizeof(float4) + sizeof(int)));
  SWN_CHECK((uintptr_t)workspace % 16 == 0 && (uintptr_t)pred % 4 == 0 && (uintptr_t)target % 4 == 0 && (uintptr_t)out % 4 == 0 &&
                (uintptr_t)map_out % 4 == 0,
            "swn_ssim_fwd: misaligned pointer");
  SsimTaps tp;
  for (int k = 0; k < SSIM_MAX_TAPS; ++k) tp.w[k] = k < filter_size ? taps[k] : 0.f;
  float4* part = (float4*)workspace;
  int* part_cnt = (int*)(part + n_slots);
  const dim3 grid(tb, ta, n_img);
  hipStream_t s = as_stream(stream);
  switch (filter_size) {
#define SWN_SSIM_CASE(FS) \
  case FS: ssim_launch<FS>(grid, s, pred, target, mask, A, B, C, tp, c1, c2, map_out, part, part_cnt); break;
    SWN_SSIM_CASE(1) SWN_SSIM_CASE(3) SWN_SSIM_CASE(5) SWN_SSIM_CASE(7) SWN_SSIM_CASE(9) SWN_SSIM_CASE(11) SWN_SSIM_CASE(13)
    SWN_SSIM_CASE(15)
#undef SWN_SSIM_CASE
  }
  SWN_LAUNCH_CHECK();
  hipLaunchKernelGGL(ssim_reduce_kernel, dim3(n_img), dim3(256), 0, s, (const float4*)part, (const int*)part_cnt, ta * tb,
                     (double)A * (double)B, C, out);
  SWN_LAUNCH_CHECK();
  return 0;
}
