// The per-image affine colour transform (--affine_appearance, opts.py:55; models/nerf_moe.py:153-161, 426-438): the appearance embedding
// does not feed layer "2"; a Linear(appearance_dim, 12) turns each image's embedding into a 3 x 4 matrix T = [A | t] and the colour head's
// linear output goes through it before the sigmoid:
//     T[n]   = affine(embedding_a(image_index[n]))                 per ray (a ray belongs to one image)
//     rgb[i] = sigmoid(A[ray(i)] color(h2[i]) + t[ray(i)])         per point
// Four entry points: the per-ray matrix (forward / backward) and the sigma / colour heads with the transform (forward / backward - the
// siblings of swn_heads_fwd / swn_heads_bwd in elementwise.hip, same row layout, same ordered reductions).  All arithmetic is fp32.
#include "common.hpp"
#include "row16.hpp"

namespace swn {

// T[n][r] = b_a[r] + sum_k emb[idx[n]][k] w_a[r][k]      (w_a [12, app_dim]: nn.Linear's layout).  One thread per (ray, r).
__global__ __launch_bounds__(256) void affine_ray_fwd_kernel(const float* __restrict__ emb, int app_dim, const void* __restrict__ image_indices,
                                                             int idx64, const float* __restrict__ w_a, const float* __restrict__ b_a, int n_rays,
                                                             float* __restrict__ T) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)n_rays * 12) return;
  const int n = (int)(t / 12), r = (int)(t - (long)n * 12);
  const long img = idx64 ? (long)((const long long*)image_indices)[n] : (long)((const int32_t*)image_indices)[n];
  const float* e = emb + img * app_dim;
  const float* w = w_a + (long)r * app_dim;
  float acc = b_a[r];
  for (int k = 0; k < app_dim; ++k) acc = fmaf(e[k], w[k], acc);
  T[t] = acc;
}

// Backward of the per-ray matrix over ARB rays per block: partial[b] = [sum_n dT[n][r] emb[idx[n]][k] (12 x app_dim) | sum_n dT[n][r] (12)]
// with the block's rays in ascending order (ordered_reduce_kernel then adds the blocks in order), and d_feat[n][k] = sum_r dT[n][r] w_a[r][k],
// the per-ray embedding gradient (handed to swn_emb_grad).
constexpr int ARB = 64;
__global__ __launch_bounds__(256) void affine_ray_bwd_kernel(const float* __restrict__ dT, const float* __restrict__ emb, int app_dim,
                                                             const void* __restrict__ image_indices, int idx64, const float* __restrict__ w_a,
                                                             int n_rays, float* __restrict__ partial, float* __restrict__ d_feat) {
  __shared__ float dts[ARB][12];
  __shared__ long imgs[ARB];
  const int b = blockIdx.x, r0 = b * ARB, nr = min(ARB, n_rays - r0);
  for (int i = threadIdx.x; i < ARB * 12; i += 256) dts[i / 12][i % 12] = i < nr * 12 ? dT[(long)r0 * 12 + i] : 0.f;
  for (int i = threadIdx.x; i < ARB; i += 256)
    imgs[i] = i < nr ? (idx64 ? (long)((const long long*)image_indices)[r0 + i] : (long)((const int32_t*)image_indices)[r0 + i]) : 0;
  __syncthreads();
  const int np = 12 * app_dim + 12;
  float* part = partial + (size_t)b * np;
  for (int t = threadIdx.x; t < np; t += 256) {
    float acc = 0.f;
    if (t < 12 * app_dim) {
      const int r = t / app_dim, k = t - r * app_dim;
      for (int n = 0; n < nr; ++n) acc = fmaf(dts[n][r], emb[imgs[n] * app_dim + k], acc);
    } else {
      const int r = t - 12 * app_dim;
      for (int n = 0; n < nr; ++n) acc += dts[n][r];
    }
    part[t] = acc;
  }
  for (int i = threadIdx.x; i < nr * app_dim; i += 256) {
    const int n = i / app_dim, k = i - n * app_dim;
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < 12; ++r) acc = fmaf(dts[n][r], w_a[(long)r * app_dim + k], acc);
    d_feat[(long)(r0 + n) * app_dim + k] = acc;
  }
}

// raw[i] = (sigmoid(A lin + t), softplus(y . ws + bs + noise - 1)), lin = h2 Wc^T + bc, [A | t] = T[i / rows_per_group].
// A 16-lane group walks a CONTIGUOUS run of rows: the ray's matrix stays in lane 0's registers until the run crosses into the next ray.
template <typename T_, int M, int H2>
__global__ __launch_bounds__(256) void heads_affine_fwd_kernel(const T_* __restrict__ y, const T_* __restrict__ h2,
                                                               const float* __restrict__ ws, const float* __restrict__ bs,
                                                               const float* __restrict__ wc, const float* __restrict__ bc,
                                                               const float* __restrict__ noise, const float* __restrict__ T,
                                                               int rows_per_group, long P, long run, float* __restrict__ raw) {
  using RY = Row16<T_, M>;
  using RH = Row16<T_, H2>;
  const int j = threadIdx.x & 15;
  float wsv[RY::VPL], wcv[3][RH::VPL];
  RY::loadf(ws, j, wsv);
#pragma unroll
  for (int c = 0; c < 3; ++c) RH::loadf(wc + c * H2, j, wcv[c]);
  const float b_s = bs[0], b0 = bc[0], b1 = bc[1], b2 = bc[2];
  const long gid = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
  const long i0 = gid * run, i1 = i0 + run < P ? i0 + run : P;
  long cur = -1;
  float4 t0 = make_float4(0, 0, 0, 0), t1 = t0, t2 = t0;       // the rows of [A | t]
  for (long i = i0; i < i1; ++i) {
    float yv[RY::VPL], hv[RH::VPL];
    RY::load(y + i * M, j, yv);
    RH::load(h2 + i * H2, j, hv);
    float s = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int v = 0; v < RY::VPL; ++v) s += yv[v] * wsv[v];
#pragma unroll
    for (int v = 0; v < RH::VPL; ++v) { c0 += hv[v] * wcv[0][v]; c1 += hv[v] * wcv[1][v]; c2 += hv[v] * wcv[2][v]; }
    s = sum16(s); c0 = sum16(c0); c1 = sum16(c1); c2 = sum16(c2);
    if (j == 0) {
      const long ray = i / rows_per_group;
      if (ray != cur) {
        const float4* tp = (const float4*)(T + ray * 12);
        t0 = tp[0]; t1 = tp[1]; t2 = tp[2];
        cur = ray;
      }
      const float l0 = c0 + b0, l1 = c1 + b1, l2 = c2 + b2;
      const float u = s + b_s + (noise ? noise[i] : 0.f) - 1.f;  // ShiftedSoftplus, models/nerf.py:68-69
      float4 o;
      o.x = 1.f / (1.f + expf(-(t0.x * l0 + t0.y * l1 + t0.z * l2 + t0.w)));
      o.y = 1.f / (1.f + expf(-(t1.x * l0 + t1.y * l1 + t1.z * l2 + t1.w)));
      o.z = 1.f / (1.f + expf(-(t2.x * l0 + t2.y * l1 + t2.z * l2 + t2.w)));
      o.w = u > 20.f ? u : log1pf(expf(u));
      *(float4*)(raw + i * 4) = o;
    }
  }
}

// swn_heads_bwd's kernel with the transform.  A block walks whole rays (units of rows_per_group rows; its 16-lane groups the unit's rows
// q, q + 16, ...) with the ray's matrix in registers; per row it recomputes lin = color(h2), forms d_pre = d_raw_c rgb (1 - rgb),
// d_lin = A^T d_pre (which takes the place of swn_heads_bwd's dc in dh2, d_w_color, d_b_color) and adds [d_pre (x) lin | d_pre] to the
// ray's dT: the 16 row stripes meet in LDS in a fixed order.  Block partial sums for the four parameter gradients -> partial[block].
template <typename T_, int M, int H2, bool HASY>
__global__ __launch_bounds__(256) void heads_affine_bwd_kernel(const T_* __restrict__ y, const T_* __restrict__ h2,
                                                               const float* __restrict__ wc, const float* __restrict__ bc,
                                                               const float* __restrict__ T, const float* __restrict__ raw,
                                                               const float* __restrict__ d_raw, long P, T_* __restrict__ dh2,
                                                               float* __restrict__ dsig, float* __restrict__ partial, int rows_per_group,
                                                               float* __restrict__ rowsum, float* __restrict__ dT) {
  using RY = Row16<T_, M>;
  using RH = Row16<T_, H2>;
  const int j = threadIdx.x & 15, grp = threadIdx.x >> 4;
  float aws[RY::VPL], awc[3][RH::VPL], abs_ = 0.f, abc[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int v = 0; v < RH::VPL; ++v) awc[c][v] = 0.f;
  }
#pragma unroll
  for (int v = 0; v < RY::VPL; ++v) aws[v] = 0.f;
  // the colour weights in LDS, read per row (in registers they cost a wave of occupancy: see heads_bwd_kernel)
  __shared__ float wc_lds[3][16][RH::VPL];
  __shared__ float cs_lds[16][H2];
  __shared__ float dt_lds[16][12];
  if (threadIdx.x < 16) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float t_[RH::VPL];
      RH::loadf(wc + c * H2, threadIdx.x, t_);
#pragma unroll
      for (int v = 0; v < RH::VPL; ++v) wc_lds[c][threadIdx.x][v] = t_[v];
    }
  }
  __syncthreads();
  const float b0 = bc[0], b1 = bc[1], b2 = bc[2];
  const long rows = rows_per_group, n_units = P / rows_per_group;
  for (long u = blockIdx.x; u < n_units; u += gridDim.x) {
    const float4* tp = (const float4*)(T + u * 12);             // (block-uniform: scalar loads)
    const float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
    float cs[RH::VPL], dt[12];
#pragma unroll
    for (int v = 0; v < RH::VPL; ++v) cs[v] = 0.f;
#pragma unroll
    for (int q = 0; q < 12; ++q) dt[q] = 0.f;
    for (long r = grp; r < rows; r += 16) {
      const long i = u * rows + r;
      const float4 rr = *(const float4*)(raw + i * 4);
      const float4 d = *(const float4*)(d_raw + i * 4);
      uint4 yr[RY::NCH], hr[RH::NCH];
      if constexpr (HASY) RY::load_raw(y + i * M, j, yr);       // (y == NULL: d_w_sigma stays untouched, like swn_heads_bwd)
      RH::load_raw(h2 + i * H2, j, hr);
      const float p0 = d.x * rr.x * (1.f - rr.x), p1 = d.y * rr.y * (1.f - rr.y), p2 = d.z * rr.z * (1.f - rr.z);      // d_pre
      const float dl0 = t0.x * p0 + t1.x * p1 + t2.x * p2, dl1 = t0.y * p0 + t1.y * p1 + t2.y * p2,
                  dl2 = t0.z * p0 + t1.z * p1 + t2.z * p2;                                                            // d_lin = A^T d_pre
      const float dsp = d.w * -expm1f(-rr.w);      // softplus'(u) = 1 - exp(-softplus(u))
      if (j == 0) {
        dsig[i] = dsp;
        abs_ += dsp; abc[0] += dl0; abc[1] += dl1; abc[2] += dl2;
      }
      asm volatile("" ::: "memory");        // (keeps the LDS reads of the colour weights inside the row loop)
      if constexpr (HASY) {
        float yv[RY::VPL];
        RY::unpack(yr, yv);
#pragma unroll
        for (int v = 0; v < RY::VPL; ++v) aws[v] += dsp * yv[v];
      }
      float hv[RH::VPL], o[RH::VPL];
      RH::unpack(hr, hv);
      float c0 = 0.f, c1 = 0.f, c2 = 0.f;
#pragma unroll
      for (int v = 0; v < RH::VPL; ++v) {
        const float w0 = wc_lds[0][j][v], w1 = wc_lds[1][j][v], w2 = wc_lds[2][j][v];
        c0 += hv[v] * w0; c1 += hv[v] * w1; c2 += hv[v] * w2;
        awc[0][v] += dl0 * hv[v]; awc[1][v] += dl1 * hv[v]; awc[2][v] += dl2 * hv[v];
        const float gg = dl0 * w0 + dl1 * w1 + dl2 * w2;
        o[v] = hv[v] > 0.f ? gg : 0.f;
      }
      RH::store(dh2 + i * H2, j, o);
      const float l0 = sum16(c0) + b0, l1 = sum16(c1) + b1, l2 = sum16(c2) + b2;      // lin, recomputed
      dt[0] += p0 * l0; dt[1] += p0 * l1; dt[2] += p0 * l2; dt[3] += p0;
      dt[4] += p1 * l0; dt[5] += p1 * l1; dt[6] += p1 * l2; dt[7] += p1;
      dt[8] += p2 * l0; dt[9] += p2 * l1; dt[10] += p2 * l2; dt[11] += p2;
      if constexpr (sizeof(T_) == 2) {
#pragma unroll
        for (int v = 0; v < RH::VPL; v += 2) {           // what the store kept: the values rounded to T_
          const uint32_t pk = pack_bf16x2(o[v], o[v + 1]);
          cs[v] += bf16_to_f32((bf16_t)(pk & 0xFFFF));
          cs[v + 1] += bf16_to_f32((bf16_t)(pk >> 16));
        }
      } else {
#pragma unroll
        for (int v = 0; v < RH::VPL; ++v) cs[v] += o[v];
      }
    }
#pragma unroll
    for (int v = 0; v < RH::VPL; ++v) cs_lds[grp][RH::col(j, v)] = cs[v];
    if (j == 0) {
#pragma unroll
      for (int q = 0; q < 12; ++q) dt_lds[grp][q] = dt[q];
    }
    __syncthreads();
    if (rowsum) {
      for (int c = threadIdx.x; c < H2; c += 256) {
        float s_ = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) s_ += cs_lds[q][c];   // the 16 row stripes in a fixed order
        rowsum[u * H2 + c] = s_;
      }
    }
    if (threadIdx.x < 12) {
      float s_ = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) s_ += dt_lds[q][threadIdx.x];
      dT[u * 12 + threadIdx.x] = s_;
    }
    __syncthreads();
  }
  // block-level reduction in LDS, the 16 row groups one after the other (fixed order); ordered_reduce_kernel adds the blocks in order
  __shared__ float red[M + 3 * H2 + 4];
  for (int t = threadIdx.x; t < M + 3 * H2 + 4; t += 256) red[t] = 0.f;
  __syncthreads();
  for (int gq = 0; gq < 16; ++gq) {
    if (grp == gq) {
#pragma unroll
      for (int v = 0; v < RY::VPL; ++v) red[RY::col(j, v)] += aws[v];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int v = 0; v < RH::VPL; ++v) red[M + c * H2 + RH::col(j, v)] += awc[c][v];
      if (j == 0) {
        red[M + 3 * H2 + 0] += abs_;
        red[M + 3 * H2 + 1] += abc[0];
        red[M + 3 * H2 + 2] += abc[1];
        red[M + 3 * H2 + 3] += abc[2];
      }
    }
    __syncthreads();
  }
  float* part = partial + (size_t)blockIdx.x * (M + 3 * H2 + 4);     // [M | 3 H2 | b_sigma | b_color(3)]
  for (int t = threadIdx.x; t < M + 3 * H2 + 4; t += 256) part[t] = red[t];
}

static int affine_bwd_blocks(long n_points, int rows_per_group) {
  long b = n_points / rows_per_group;
  if (b > 1024) b = 1024;
  return b < 1 ? 1 : (int)b;
}

}  // namespace swn

using namespace swn;

extern "C" int swn_affine_ray_fwd(const float* emb, int app_dim, const void* image_indices, int indices_are_int64, const float* w_affine,
                                  const float* b_affine, int n_rays, float* T, void* stream) {
  SWN_CHECK(emb && image_indices && w_affine && b_affine && T, "swn_affine_ray_fwd: null pointer");
  SWN_CHECK(n_rays >= 0 && app_dim > 0 && app_dim <= 256, "swn_affine_ray_fwd: bad sizes (rays %d, width %d)", n_rays, app_dim);
  if (n_rays == 0) return 0;
  hipLaunchKernelGGL(affine_ray_fwd_kernel, dim3(cdiv((long)n_rays * 12, 256)), dim3(256), 0, as_stream(stream), emb, app_dim, image_indices,
                     indices_are_int64, w_affine, b_affine, n_rays, T);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_affine_ray_bwd_workspace_bytes(int n_rays, int app_dim, size_t* bytes) {
  SWN_CHECK(bytes && n_rays >= 0 && app_dim > 0, "swn_affine_ray_bwd_workspace_bytes: bad arguments");
  *bytes = (size_t)cdiv(n_rays > 0 ? n_rays : 1, ARB) * (size_t)(12 * app_dim + 12) * sizeof(float);
  return 0;
}

extern "C" int swn_affine_ray_bwd(const float* dT, const float* emb, int app_dim, const void* image_indices, int indices_are_int64,
                                  const float* w_affine, int n_rays, float* d_w_affine, float* d_b_affine, float* d_feat, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  SWN_CHECK(dT && emb && image_indices && w_affine && d_w_affine && d_b_affine && d_feat && workspace, "swn_affine_ray_bwd: null pointer");
  SWN_CHECK(n_rays >= 0 && app_dim > 0 && app_dim <= 256, "swn_affine_ray_bwd: bad sizes (rays %d, width %d)", n_rays, app_dim);
  size_t need = 0;
  swn_affine_ray_bwd_workspace_bytes(n_rays, app_dim, &need);
  SWN_CHECK(workspace_bytes >= need, "swn_affine_ray_bwd: workspace of %zu bytes, need %zu", workspace_bytes, need);
  if (n_rays == 0) return 0;
  const int nb = cdiv(n_rays, ARB);
  hipLaunchKernelGGL(affine_ray_bwd_kernel, dim3(nb), dim3(256), 0, as_stream(stream), dT, emb, app_dim, image_indices, indices_are_int64,
                     w_affine, n_rays, (float*)workspace, d_feat);
  OrdDst od{{d_w_affine, d_b_affine, nullptr, nullptr}, {12 * app_dim, 12, 0, 0}};
  ordered_reduce_async((const float*)workspace, nb, 12 * app_dim + 12, od, true, as_stream(stream));
  SWN_LAUNCH_CHECK();
  return 0;
}

#define SWN_AFF_DISPATCH(MACRO)                                                                                                   \
  do {                                                                                                                            \
    if (dtype == SWN_HALF) {                                                                                                      \
      if (model_dim == 256 && h2_dim == 128) MACRO(bf16_t, 256, 128); else if (model_dim == 512 && h2_dim == 256) MACRO(bf16_t, 512, 256); \
      else if (model_dim == 256) MACRO(bf16_t, 256, 256); else MACRO(bf16_t, 512, 128);                                           \
    } else {                                                                                                                      \
      if (model_dim == 256 && h2_dim == 128) MACRO(float, 256, 128); else if (model_dim == 512 && h2_dim == 256) MACRO(float, 512, 256); \
      else if (model_dim == 256) MACRO(float, 256, 256); else MACRO(float, 512, 128);                                             \
    }                                                                                                                             \
  } while (0)

extern "C" int swn_heads_affine_fwd(const void* y, const void* h2, int dtype, const float* w_sigma, const float* b_sigma,
                                    const float* w_color, const float* b_color, const float* sigma_noise, const float* T,
                                    int rows_per_group, int n_points, int model_dim, int h2_dim, float* raw, void* stream) {
  SWN_CHECK(dtype == SWN_F32 || dtype == SWN_HALF, "swn_heads_affine_fwd: bad dtype");
  SWN_CHECK(y && h2 && w_sigma && b_sigma && w_color && b_color && T && raw, "swn_heads_affine_fwd: null pointer");
  SWN_CHECK((model_dim == 256 || model_dim == 512) && (h2_dim == 128 || h2_dim == 256),
            "swn_heads_affine_fwd: model_dim in {256,512}, h2_dim in {128,256}");
  SWN_CHECK(n_points >= 0 && rows_per_group > 0 && n_points % rows_per_group == 0,
            "swn_heads_affine_fwd: rows_per_group %d must be positive and divide n_points %d", rows_per_group, n_points);
  if (n_points == 0) return 0;
  // 16-lane groups take contiguous runs of rows: at most 4096 blocks x 16 groups, a run of at least one row
  long blocks = ((long)n_points + 15) / 16;
  if (blocks > 4096) blocks = 4096;
  const long run = ((long)n_points + blocks * 16 - 1) / (blocks * 16);
#define SWN_HAF(T_, M_, H_) hipLaunchKernelGGL((heads_affine_fwd_kernel<T_, M_, H_>), dim3((int)blocks), dim3(256), 0, as_stream(stream), \
                                               (const T_*)y, (const T_*)h2, w_sigma, b_sigma, w_color, b_color, sigma_noise, T,        \
                                               rows_per_group, (long)n_points, run, raw)
  SWN_AFF_DISPATCH(SWN_HAF);
#undef SWN_HAF
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_heads_affine_bwd_workspace_bytes(int n_points, int model_dim, int h2_dim, int rows_per_group, size_t* bytes) {
  SWN_CHECK(bytes && n_points >= 0 && rows_per_group > 0, "swn_heads_affine_bwd_workspace_bytes: bad arguments");
  *bytes = (size_t)affine_bwd_blocks(n_points, rows_per_group) * (size_t)(model_dim + 3 * h2_dim + 4) * sizeof(float);
  return 0;
}

extern "C" int swn_heads_affine_bwd(const void* y, const void* h2, int dtype, const float* w_color, const float* b_color, const float* T,
                                    const float* raw, const float* d_raw, int n_points, int model_dim, int h2_dim, int rows_per_group,
                                    void* dh2, float* dsig, float* d_w_sigma, float* d_b_sigma, float* d_w_color, float* d_b_color,
                                    float* group_colsum, float* dT, void* workspace, size_t workspace_bytes, void* stream) {
  SWN_CHECK(dtype == SWN_F32 || dtype == SWN_HALF, "swn_heads_affine_bwd: bad dtype");
  SWN_CHECK(h2 && w_color && b_color && T && raw && d_raw && dh2 && dsig && d_w_sigma && d_b_sigma && d_w_color && d_b_color && dT && workspace,
            "swn_heads_affine_bwd: null pointer");      // (y may be NULL: d_w_sigma is left as it is; group_colsum may be NULL)
  SWN_CHECK((model_dim == 256 || model_dim == 512) && (h2_dim == 128 || h2_dim == 256),
            "swn_heads_affine_bwd: model_dim in {256,512}, h2_dim in {128,256}");
  SWN_CHECK(n_points >= 0 && rows_per_group > 0 && n_points % rows_per_group == 0,
            "swn_heads_affine_bwd: rows_per_group %d must be positive and divide n_points %d", rows_per_group, n_points);
  size_t need = 0;
  swn_heads_affine_bwd_workspace_bytes(n_points, model_dim, h2_dim, rows_per_group, &need);
  SWN_CHECK(workspace_bytes >= need, "swn_heads_affine_bwd: workspace of %zu bytes, need %zu", workspace_bytes, need);
  if (n_points == 0) return 0;
  const int blocks = affine_bwd_blocks(n_points, rows_per_group);
  float* partial = (float*)workspace;
#define SWN_HAB1(T_, M_, H_, Y_) hipLaunchKernelGGL((heads_affine_bwd_kernel<T_, M_, H_, Y_>), dim3(blocks), dim3(256), 0, as_stream(stream), \
                                                    (const T_*)y, (const T_*)h2, w_color, b_color, T, raw, d_raw, (long)n_points, (T_*)dh2,    \
                                                    dsig, partial, rows_per_group, group_colsum, dT)
#define SWN_HAB(T_, M_, H_) do { if (y) SWN_HAB1(T_, M_, H_, true); else SWN_HAB1(T_, M_, H_, false); } while (0)
  SWN_AFF_DISPATCH(SWN_HAB);
#undef SWN_HAB
#undef SWN_HAB1
  OrdDst od{{d_w_sigma, d_w_color, d_b_sigma, d_b_color}, {model_dim, 3 * h2_dim, 1, 3}};
  ordered_reduce_async(partial, blocks, model_dim + 3 * h2_dim + 4, od, true, as_stream(stream));
  SWN_LAUNCH_CHECK();
  return 0;
}
