// Spherical-harmonics colour (--sh_deg d, opts.py:69; models/nerf.py:137-143 + rendering.py:317-349): the colour head emits 3 B
// coefficients per point, B = (d + 1)^2, row c B + b of the head belonging to colour c and basis function b, and
//     rgb_c[i] = sigmoid(sum_b Y_b(dir[ray(i)]) lin[i][c B + b]),      lin[i] = h2[i] Wc^T + bc        (Wc [3 B, H2], bc [3 B])
// with Y_b the real spherical-harmonics polynomials of the ray direction, taken as given (the reference does not normalise it).
//
// The direction is constant along a ray and the contraction is linear, so it is folded into the WEIGHTS once per ray,
//     Weff[c] = sum_b Y_b Wc[c B + b]   (3 x H2),      beff[c] = sum_b Y_b bc[c B + b],      rgb_c[i] = sigmoid(h2[i] . Weff[c] + beff[c]),
// and every point of the ray runs the plain three-row head against Weff in LDS: 3 B H2 multiply-adds per RAY plus 3 H2 per point
// instead of 3 B H2 per point, whatever the degree - the kernels stay bound by reading y and h2.  The backward uses the same fold:
// d_lin[c B + b] = p_c Y_b with p_c = d_raw_c rgb_c (1 - rgb_c), so dh2 = sum_c p_c Weff[c], and the weight gradient factors per ray,
//     d_Wc[c B + b] = sum_rays Y_b(ray) A_c(ray),      A_c(ray) = sum_{i in ray} p_c[i] h2[i]      (3 x H2 per ray),
// formed in two steps: the heads' launch leaves A_c and sum_i p_c per ray, a second small launch expands them by the basis over
// blocks of rays, and the existing ordered reduce adds the blocks.  Arithmetic is fp32 (one exception: the terms of d_b_sigma, see
// heads_sh_bwd_kernel), no atomics, every cross-thread sum is added in a fixed order.  The optional `coef` output (the module's return value, octree sampling) is computed directly per point.
#include "common.hpp"
#include "row16.hpp"

namespace swn {

constexpr int SH_MAXB = 25;      // (4 + 1)^2

// Real spherical harmonics up to degree 4 as polynomials of an (unnormalised) direction, with the sign of each term folded into
// its value: Y[b] multiplies coefficient b.
__device__ __forceinline__ void sh_basis(int deg, float x, float y, float z, float* Y) {
#pragma unroll
  for (int b = 0; b < SH_MAXB; ++b) Y[b] = 0.f;
  Y[0] = 0.28209479177387814f;
  if (deg < 1) return;
  const float k1 = 0.4886025119029199f;
  Y[1] = -k1 * y;
  Y[2] = k1 * z;
  Y[3] = -k1 * x;
  if (deg < 2) return;
  const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
  const float k2 = 1.0925484305920792f;
  Y[4] = k2 * xy;
  Y[5] = -k2 * yz;
  Y[6] = 0.31539156525252005f * (2.f * zz - xx - yy);
  Y[7] = -k2 * xz;
  Y[8] = 0.5462742152960396f * (xx - yy);
  if (deg < 3) return;
  const float k3a = 0.5900435899266435f, k3b = 0.4570457994644658f;
  Y[9] = -k3a * y * (3.f * xx - yy);
  Y[10] = 2.890611442640554f * xy * z;
  Y[11] = -k3b * y * (4.f * zz - xx - yy);
  Y[12] = 0.3731763325901154f * z * (2.f * zz - 3.f * xx - 3.f * yy);
  Y[13] = -k3b * x * (4.f * zz - xx - yy);
  Y[14] = 1.445305721320277f * z * (xx - yy);
  Y[15] = -k3a * x * (xx - 3.f * yy);
  if (deg < 4) return;
  const float k4a = 1.7701307697799304f, k4b = 0.6690465435572892f;
  Y[16] = 2.5033429417967046f * xy * (xx - yy);
  Y[17] = -k4a * yz * (3.f * xx - yy);
  Y[18] = 0.9461746957575601f * xy * (7.f * zz - 1.f);
  Y[19] = -k4b * yz * (7.f * zz - 3.f);
  Y[20] = 0.10578554691520431f * (zz * (35.f * zz - 30.f) + 3.f);
  Y[21] = -k4b * xz * (7.f * zz - 3.f);
  Y[22] = 0.47308734787878004f * (xx - yy) * (7.f * zz - 1.f);
  Y[23] = -k4a * xz * (xx - 3.f * yy);
  Y[24] = 0.6258357354491761f * (xx * (xx - 3.f * yy) - yy * (3.f * xx - yy));
}

// a + b as an unevaluated pair: s = fl(a + b), e = the rounding error of that add, exactly (Knuth's TwoSum; plain fp32 adds, no
// reassociation: the library is not built with fast-math)
__device__ __forceinline__ void two_sum(float a, float b, float& s, float& e) {
  s = a + b;
  const float bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

// The fold of one ray, by the whole block: ys = the basis at dir, weff[c][lane][value] = Weff[c] in the 16-lane row layout (each lane's
// weights in its own value order, like wc_lds of swn_heads_bwd), beff[c].  Ends in a barrier; the caller puts one in front of the next fold.
template <typename RH, int H2>
__device__ __forceinline__ void sh_fold(const float* __restrict__ wc, const float* __restrict__ bc, const float* __restrict__ dir, int deg,
                                        float* ys, float (*weff)[16][RH::VPL], float* beff) {
  const int B = (deg + 1) * (deg + 1);
  if (threadIdx.x == 0) {
    float Y[SH_MAXB];
    sh_basis(deg, dir[0], dir[1], dir[2], Y);
#pragma unroll
    for (int b = 0; b < SH_MAXB; ++b) ys[b] = Y[b];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 3 * H2; e += 256) {
    const int c = e / H2, col = e - c * H2;
    const float* w = wc + (long)c * B * H2 + col;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc = fmaf(ys[b], w[(long)b * H2], acc);
    const int chunk = col / RH::EPC, within = col - chunk * RH::EPC;      // the inverse of Row16::col
    weff[c][chunk & 15][(chunk >> 4) * RH::EPC + within] = acc;
  }
  if (threadIdx.x < 3) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc = fmaf(ys[b], bc[threadIdx.x * B + b], acc);
    beff[threadIdx.x] = acc;
  }
  __syncthreads();
}

// raw[i] = (sigmoid(h2[i] . Weff[c] + beff[c]) c < 3, softplus(y . ws + bs + noise - 1)); coef[i] = h2[i] Wc^T + bc when asked for.
// A block walks whole rays (units of rows_per_group rows), its 16-lane groups the unit's rows q, q + 16, ...
template <typename T_, int M, int H2>
__global__ __launch_bounds__(256) void heads_sh_fwd_kernel(const T_* __restrict__ y, const T_* __restrict__ h2, const float* __restrict__ ws,
                                                           const float* __restrict__ bs, const float* __restrict__ wc,
                                                           const float* __restrict__ bc, const float* __restrict__ noise,
                                                           const float* __restrict__ dirs, int rows_per_group, int deg, long P,
                                                           float* __restrict__ raw, float* __restrict__ coef) {
  using RY = Row16<T_, M>;
  using RH = Row16<T_, H2>;
  __shared__ float ys[SH_MAXB];
  __shared__ float weff[3][16][RH::VPL];
  __shared__ float beff[3];
  const int j = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int B = (deg + 1) * (deg + 1);
  float wsv[RY::VPL];
  RY::loadf(ws, j, wsv);
  const float b_s = bs[0];
  const long rows = rows_per_group, n_units = P / rows_per_group;
  for (long u = blockIdx.x; u < n_units; u += gridDim.x) {
    sh_fold<RH, H2>(wc, bc, dirs + u * 3, deg, ys, weff, beff);
    const float b0 = beff[0], b1 = beff[1], b2 = beff[2];
    for (long r = grp; r < rows; r += 16) {
      const long i = u * rows + r;
      float yv[RY::VPL], hv[RH::VPL];
      RY::load(y + i * M, j, yv);
      RH::load(h2 + i * H2, j, hv);
      float s = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
#pragma unroll
      for (int v = 0; v < RY::VPL; ++v) s += yv[v] * wsv[v];
#pragma unroll
      for (int v = 0; v < RH::VPL; ++v) { c0 += hv[v] * weff[0][j][v]; c1 += hv[v] * weff[1][j][v]; c2 += hv[v] * weff[2][j][v]; }
      s = sum16(s); c0 = sum16(c0); c1 = sum16(c1); c2 = sum16(c2);
      if (j == 0) {
        const float uu = s + b_s + (noise ? noise[i] : 0.f) - 1.f;  // ShiftedSoftplus, models/nerf.py:68-69
        float4 o;
        o.x = 1.f / (1.f + expf(-(c0 + b0)));
        o.y = 1.f / (1.f + expf(-(c1 + b1)));
        o.z = 1.f / (1.f + expf(-(c2 + b2)));
        o.w = uu > 20.f ? uu : log1pf(expf(uu));
        *(float4*)(raw + i * 4) = o;
      }
      if (coef) {      // the linear outputs themselves (not on the training path): one row of Wc at a time, from global memory
        for (int k = 0; k < 3 * B; ++k) {
          float wv[RH::VPL];
          RH::loadf(wc + (long)k * H2, j, wv);
          float a = 0.f;
#pragma unroll
          for (int v = 0; v < RH::VPL; ++v) a += hv[v] * wv[v];
          a = sum16(a);
          if (j == 0) coef[i * (3 * B) + k] = a + bc[k];
        }
      }
    }
    __syncthreads();      // (the next unit's fold overwrites weff)
  }
}

// The backward of the heads with the fold.  Per unit (ray): dh2 rows (masked by h2 > 0), dsig, rowsum[u] = the column sums of the dh2 rows
// as stored, and ray_acc[u] = [A_0 | A_1 | A_2 | sum p_0, sum p_1, sum p_2, 0]  (3 H2 + 4 floats), the 16 row stripes added in a fixed
// order.  The block's sums for d_w_sigma and d_b_sigma -> partial[block] (M + 2 floats).  d_b_sigma is ONE scalar summed over every
// point, signed terms that cancel: it is carried as a compensated fp32 pair (sum, accumulated rounding errors) from the first add to
// the last (sh_bsig_reduce_kernel), so that its error is a rounding of the result and not a random walk over the partial sums.
template <typename T_, int M, int H2>
__global__ __launch_bounds__(256) void heads_sh_bwd_kernel(const T_* __restrict__ y, const T_* __restrict__ h2, const float* __restrict__ wc,
                                                           const float* __restrict__ bc, const float* __restrict__ dirs,
                                                           const float* __restrict__ raw, const float* __restrict__ d_raw, long P,
                                                           int rows_per_group, int deg, T_* __restrict__ dh2, float* __restrict__ dsig,
                                                           float* __restrict__ rowsum, float* __restrict__ ray_acc,
                                                           float* __restrict__ partial) {
  using RY = Row16<T_, M>;
  using RH = Row16<T_, H2>;
  constexpr int ACC = 3 * H2 + 4;
  __shared__ float ys[SH_MAXB];
  __shared__ float weff[3][16][RH::VPL];
  __shared__ float beff[3];
  __shared__ float st_lds[16][H2];      // the 16 row stripes of one quantity at a time
  __shared__ float p_lds[16][3];
  const int j = threadIdx.x & 15, grp = threadIdx.x >> 4;
  float aws[RY::VPL], abs_ = 0.f, abs_lo = 0.f;
#pragma unroll
  for (int v = 0; v < RY::VPL; ++v) aws[v] = 0.f;
  const long rows = rows_per_group, n_units = P / rows_per_group;
  for (long u = blockIdx.x; u < n_units; u += gridDim.x) {
    sh_fold<RH, H2>(wc, bc, dirs + u * 3, deg, ys, weff, beff);
    float cs[RH::VPL], awc[3][RH::VPL], ap0 = 0.f, ap1 = 0.f, ap2 = 0.f;
#pragma unroll
    for (int v = 0; v < RH::VPL; ++v) { cs[v] = 0.f; awc[0][v] = 0.f; awc[1][v] = 0.f; awc[2][v] = 0.f; }
    for (long r = grp; r < rows; r += 16) {
      const long i = u * rows + r;
      const float4 rr = *(const float4*)(raw + i * 4);
      const float4 d = *(const float4*)(d_raw + i * 4);
      uint4 yr[RY::NCH], hr[RH::NCH];
      RY::load_raw(y + i * M, j, yr);
      RH::load_raw(h2 + i * H2, j, hr);
      const float p0 = d.x * rr.x * (1.f - rr.x), p1 = d.y * rr.y * (1.f - rr.y), p2 = d.z * rr.z * (1.f - rr.z);
      const float dsp = d.w * -expm1f(-rr.w);      // softplus'(u) = 1 - exp(-softplus(u))
      if (j == 0) {
        dsig[i] = dsp;
        // the bias term once more in double (this lane only): over 10^4 .. 10^6 signed terms the fp32 roundings of expm1f and of the
        // product are a random walk larger than the sum's own rounding; dsig itself and every other sum stay fp32
        const double t_ = (double)d.w * (1.0 - exp(-(double)rr.w));
        const float th_ = (float)t_;
        float e_;
        two_sum(abs_, th_, abs_, e_);
        abs_lo += e_ + (float)(t_ - (double)th_);
      }
      ap0 += p0; ap1 += p1; ap2 += p2;
      float yv[RY::VPL];
      RY::unpack(yr, yv);
#pragma unroll
      for (int v = 0; v < RY::VPL; ++v) aws[v] += dsp * yv[v];
      float hv[RH::VPL], o[RH::VPL];
      RH::unpack(hr, hv);
#pragma unroll
      for (int v = 0; v < RH::VPL; ++v) {
        awc[0][v] += p0 * hv[v]; awc[1][v] += p1 * hv[v]; awc[2][v] += p2 * hv[v];
        const float gg = p0 * weff[0][j][v] + p1 * weff[1][j][v] + p2 * weff[2][j][v];
        o[v] = hv[v] > 0.f ? gg + 0.f : 0.f;      // (+ 0: a row whose d_raw is zero leaves +0 whatever the weights' signs)
      }
      RH::store(dh2 + i * H2, j, o);
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
    // the 16 row stripes meet in LDS, one quantity after the other, each added in a fixed order
    float* acc_out = ray_acc + u * ACC;
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int v = 0; v < RH::VPL; ++v) st_lds[grp][RH::col(j, v)] = q == 0 ? cs[v] : awc[q - 1][v];
      if (q == 0 && j == 0) { p_lds[grp][0] = ap0; p_lds[grp][1] = ap1; p_lds[grp][2] = ap2; }
      __syncthreads();
      float* dst = q == 0 ? (rowsum ? rowsum + u * H2 : nullptr) : acc_out + (q - 1) * H2;
      if (dst) {
        for (int c = threadIdx.x; c < H2; c += 256) {
          float s_ = 0.f;
#pragma unroll
          for (int g = 0; g < 16; ++g) s_ += st_lds[g][c];
          dst[c] = s_;
        }
      }
      if (q == 0 && threadIdx.x < 4) {
        float s_ = 0.f;
        if (threadIdx.x < 3) {
#pragma unroll
          for (int g = 0; g < 16; ++g) s_ += p_lds[g][threadIdx.x];
        }
        acc_out[3 * H2 + threadIdx.x] = s_;
      }
      __syncthreads();
    }
  }
  // block-level reduction of the sigma head's sums, the 16 row groups one after the other; ordered_reduce_kernel adds the blocks in order
  __shared__ float red[M + 2];
  for (int t = threadIdx.x; t < M + 2; t += 256) red[t] = 0.f;
  __syncthreads();
  for (int gq = 0; gq < 16; ++gq) {
    if (grp == gq) {
#pragma unroll
      for (int v = 0; v < RY::VPL; ++v) red[RY::col(j, v)] += aws[v];
      if (j == 0) {
        float s_, e_;
        two_sum(red[M], abs_, s_, e_);
        red[M] = s_;
        red[M + 1] += e_ + abs_lo;
      }
    }
    __syncthreads();
  }
  float* part = partial + (size_t)blockIdx.x * (M + 2);     // [M | b_sigma: sum, rounding errors]
  for (int t = threadIdx.x; t < M + 2; t += 256) part[t] = red[t];
}

// d_b_sigma += the blocks' pairs (columns M, M + 1 of partial, row stride M + 2), added in ascending order with two_sum: lane l takes
// the run of consecutive blocks l * per .. , lane 0 then adds the 64 run pairs in order.  One wave, fixed order: the same bits every run.
__global__ __launch_bounds__(64) void sh_bsig_reduce_kernel(const float* __restrict__ partial, int n_blocks, int M, float* __restrict__ d_bs) {
  __shared__ float hi[64], lo[64];
  const int per = (n_blocks + 63) / 64, b0 = threadIdx.x * per, b1 = n_blocks < b0 + per ? n_blocks : b0 + per;
  float s = 0.f, c = 0.f;
  for (int b = b0; b < b1; ++b) {
    const float* q = partial + (size_t)b * (M + 2) + M;
    float e_;
    two_sum(s, q[0], s, e_);
    c += e_ + q[1];
  }
  hi[threadIdx.x] = s;
  lo[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    float S = 0.f, C = 0.f;
    for (int l = 0; l < 64; ++l) {
      float e_;
      two_sum(S, hi[l], S, e_);
      C += e_ + lo[l];
    }
    d_bs[0] += S + C;
  }
}

// The per-ray sums expanded by the basis over SRB rays per block, rays in ascending order:
// partial[block] = [sum_n Y_b(n) A_c(n)  (3 B x H2, row c B + b) | sum_n Y_b(n) sum p_c(n)  (3 B)]; ordered_reduce_kernel adds the blocks.
constexpr int SRB = 64;
__global__ __launch_bounds__(256) void sh_wgrad_kernel(const float* __restrict__ ray_acc, const float* __restrict__ dirs, long n_units, int deg,
                                                       int H2, float* __restrict__ partial) {
  __shared__ float ysr[SRB][SH_MAXB];
  const int B = (deg + 1) * (deg + 1), ACC = 3 * H2 + 4;
  const long r0 = (long)blockIdx.x * SRB;
  const int nr = (int)(n_units - r0 < SRB ? n_units - r0 : SRB);
  if (threadIdx.x < SRB) {
    float Y[SH_MAXB];
    if ((int)threadIdx.x < nr) {
      const float* dir = dirs + (r0 + threadIdx.x) * 3;
      sh_basis(deg, dir[0], dir[1], dir[2], Y);
    } else {
#pragma unroll
      for (int b = 0; b < SH_MAXB; ++b) Y[b] = 0.f;
    }
#pragma unroll
    for (int b = 0; b < SH_MAXB; ++b) ysr[threadIdx.x][b] = Y[b];
  }
  __syncthreads();
  const int nw = 3 * B * H2, np = nw + 3 * B;
  float* part = partial + (size_t)blockIdx.x * np;
  for (int e = threadIdx.x; e < np; e += 256) {
    int b;
    const float* src;
    if (e < nw) {
      const int k = e / H2, col = e - k * H2, c = k / B;
      b = k - c * B;
      src = ray_acc + r0 * ACC + c * H2 + col;
    } else {
      const int k = e - nw, c = k / B;
      b = k - c * B;
      src = ray_acc + r0 * ACC + 3 * H2 + c;
    }
    float acc = 0.f;
    for (int n = 0; n < nr; ++n) acc = fmaf(ysr[n][b], src[(long)n * ACC], acc);
    part[e] = acc;
  }
}

// ---- swn_cells_blend_sh: the Mega-NeRF blend (mega_nerf.py:34-49) of rows of 3 B coefficients + sigma, then sigmoid(eval_sh) ----------
// A member row is up to 76 floats, so a point's channels lie over the 16 lanes of a group (channel j + 16 v in lane j): the group reads
// a member row as consecutive 64-byte runs, and the four groups of a wave take four consecutive points.  The slots and weights of 16
// cells are read once by the group (lane j: cell c0 + j); a ballot gives the members, walked in ascending order with the values handed
// round by shuffles.  A workgroup takes BSH_TILE consecutive points; the basis of every ray among them is computed once, by one thread
// each, into LDS.  The blended row goes through LDS to meet the basis: lane 4 c + q adds the terms b = q, q + 4, .. of colour c, the four
// partial sums are joined as (q0 + q1) + (q2 + q3).  Plain loads and stores, no atomics, every sum in a fixed order.
constexpr int BSH_MAX_CELLS = 64;
constexpr int BSH_TILE = 64;         // points per workgroup: 16 groups x 4 passes

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

template <int DEG>
__global__ __launch_bounds__(256) void cells_blend_sh_kernel(const float* __restrict__ weights, const int32_t* __restrict__ slot,
                                                            const int32_t* __restrict__ begin, const float* __restrict__ sub_out, long total,
                                                            const float* __restrict__ dirs, int rows_per_group, int K, int hard, long P,
                                                            float* __restrict__ raw, float* __restrict__ coef_out) {
#pragma clang fp contract(off)
  constexpr int B = (DEG + 1) * (DEG + 1), WD = 3 * B + 1, VPL = (WD + 15) / 16;
  __shared__ float ys[BSH_TILE][SH_MAXB];
  __shared__ float row[16][VPL * 16];
  const int j = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const long p0 = (long)blockIdx.x * BSH_TILE;
  const long p_end = p0 + BSH_TILE < P ? p0 + BSH_TILE : P;
  const long ray0 = p0 / rows_per_group;
  const int n_dirs = (int)((p_end - 1) / rows_per_group - ray0) + 1;      // <= BSH_TILE
  if ((int)threadIdx.x < n_dirs) {
    const float* d = dirs + (ray0 + threadIdx.x) * 3;
    float Y[SH_MAXB];
    sh_basis(DEG, d[0], d[1], d[2], Y);
#pragma unroll
    for (int b = 0; b < B; ++b) ys[threadIdx.x][b] = Y[b];
  }
  __syncthreads();
  for (int q = 0; q < BSH_TILE / 16; ++q) {      // (the same trip count for every thread: ballots, shuffles and barriers inside)
    const long p = p0 + q * 16 + grp;
    const bool valid = p < P;
    float acc[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v) acc[v] = 0.f;
    for (int c0 = 0; c0 < K; c0 += 16) {
      const int i = c0 + j;
      int s = -1;
      float wt = 0.f;
      if (valid && i < K) {
        s = slot[p * K + i];
        wt = weights[p * K + i];
      }
      unsigned bits = (unsigned)((__ballot(s >= 0) >> (threadIdx.x & 48)) & 0xFFFFull);      // this group's members among the 16 cells
      while (bits) {                              // ascending cell order (:34); the lanes of a group walk it together
        const int b = __ffs(bits) - 1;
        bits &= bits - 1;
        const int si = __shfl(s, b, 16);
        const float wi = __shfl(wt, b, 16);
        const long r = (long)begin[c0 + b] + si;
        if (r < 0 || r >= total) continue;        // (never for a slot list of swn_cells_pack)
        const float* src = sub_out + r * WD;
#pragma unroll
        for (int v = 0; v < VPL; ++v) {
          const int ch = j + 16 * v;
          if (ch < WD) {
            const float val = src[ch];
            if (hard) {                           // results[cluster_mask] = sub_result (:47)
              acc[v] = val;
            } else {                              // results[cluster_mask] += sub_result * weights[cluster_mask, i] (:49)
              const float prod = val * wi;
              acc[v] = acc[v] + prod;
            }
          }
        }
      }
    }
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      const int ch = j + 16 * v;
      row[grp][ch] = acc[v];
      if (valid && coef_out && ch < WD) coef_out[p * WD + ch] = acc[v];
    }
    __syncthreads();
    const int c = j >> 2, part = j & 3;
    float sres = 0.f;
    if (valid && c < 3) {
      const float* Y = ys[(int)(p / rows_per_group - ray0)];
      for (int b = part; b < B; b += 4) sres = fmaf(Y[b], row[grp][c * B + b], sres);
    }
    sres = sres + __shfl_xor(sres, 1, 16);
    sres = sres + __shfl_xor(sres, 2, 16);
    const float s1 = __shfl(sres, 4, 16), s2 = __shfl(sres, 8, 16);
    if (valid && j == 0) *(float4*)(raw + p * 4) = make_float4(sigmoidf_(sres), sigmoidf_(s1), sigmoidf_(s2), row[grp][3 * B]);
    __syncthreads();                              // (the next pass overwrites row)
  }
}

// Degree 0: a row is four floats, one thread per point like cells_blend_kernel<4>; the same blend, then the same evaluation with B = 1.
__global__ __launch_bounds__(256) void cells_blend_sh0_kernel(const float* __restrict__ weights, const int32_t* __restrict__ slot,
                                                             const int32_t* __restrict__ begin, const float* __restrict__ sub_out, long total,
                                                             const float* __restrict__ dirs, int rows_per_group, int K, int hard, long P,
                                                             float* __restrict__ raw, float* __restrict__ coef_out) {
#pragma clang fp contract(off)
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < K; ++i) {
    const int s = slot[p * K + i];
    if (s < 0) continue;
    const long r = (long)begin[i] + s;
    if (r < 0 || r >= total) continue;
    const float4 qv = *reinterpret_cast<const float4*>(sub_out + r * 4);
    const float v[4] = {qv.x, qv.y, qv.z, qv.w};
    if (hard) {
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = v[c];
    } else {
      const float wt = weights[p * K + i];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float prod = v[c] * wt;
        acc[c] = acc[c] + prod;
      }
    }
  }
  if (coef_out) *reinterpret_cast<float4*>(coef_out + p * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  const float* d = dirs + (p / rows_per_group) * 3;
  float Y[SH_MAXB];
  sh_basis(0, d[0], d[1], d[2], Y);
  // (the partial sums of the wide kernel that have no term are + 0: the same bits)
  *reinterpret_cast<float4*>(raw + p * 4) = make_float4(sigmoidf_(fmaf(Y[0], acc[0], 0.f)), sigmoidf_(fmaf(Y[0], acc[1], 0.f)),
                                                        sigmoidf_(fmaf(Y[0], acc[2], 0.f)), acc[3]);
}

static int sh_blocks(long n_units) { return n_units > 2048 ? 2048 : (n_units < 1 ? 1 : (int)n_units); }

// the three parts of the backward's workspace, each a multiple of 64 floats
struct ShWs { size_t sig, ray, wg; };
static ShWs sh_ws(int n_points, int model_dim, int h2_dim, int rows_per_group, int deg) {
  const long n_units = n_points / rows_per_group;
  const int B = (deg + 1) * (deg + 1);
  auto up = [](size_t n) { return (n + 63) / 64 * 64; };
  ShWs w;
  w.sig = up((size_t)sh_blocks(n_units) * (size_t)(model_dim + 2));
  w.ray = up((size_t)(n_units > 0 ? n_units : 1) * (size_t)(3 * h2_dim + 4));
  w.wg = up((size_t)cdiv(n_units > 0 ? n_units : 1, SRB) * (size_t)(3 * B * h2_dim + 3 * B));
  return w;
}


// ---- training Mega-NeRF cells with spherical-harmonics colour (mega.py, sh_training) --------------------------------------------------
// The reference blends the cells' raw [3 B + 1] rows and evaluates the basis on the BLEND (rendering.py:344-347), so a cell's head emits
// its coefficient row and the basis enters the backward only: with rgb = sigmoid(sum_b Y_b blended[c B + b]) the gradient of a cell's
// linear colour output is rank one in (c, b), d_lin[r][c B + b] = q_c[r] Y_b(r).  swn_cells_blend_sh_bwd leaves q [total, 4] and one
// direction per packed row; the wide gradient is never written.  A cell's packed rows are not whole rays, so nothing is folded per
// ray here: the heads below work per row against Wc staged in LDS.

// One thread per packed row (cells_blend_bwd_kernel's shape): the cell by bisection in the LDS copy of begin[] (soft margin only).
__global__ __launch_bounds__(256) void cells_blend_sh_bwd_kernel(const float* __restrict__ weights, const int32_t* __restrict__ rows,
                                                                const int32_t* __restrict__ begin, const float* __restrict__ raw,
                                                                const float* __restrict__ d_raw, const float* __restrict__ dirs,
                                                                const float* __restrict__ sub_out, long total, int rows_per_group, int K,
                                                                int hard, int deg, long P, float* __restrict__ q,
                                                                float* __restrict__ dirs_packed) {
#pragma clang fp contract(off)
  __shared__ int sb[BSH_MAX_CELLS + 1];
  if (!hard) {
    if ((int)threadIdx.x <= K) sb[threadIdx.x] = begin[threadIdx.x];
    __syncthreads();
  }
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total) return;
  const long p = rows[r];
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  float dx = 0.f, dy = 0.f, dz = 0.f;
  if (p >= 0 && p < P) {                      // (never false for a row list of swn_cells_pack)
    const float4 rr = *reinterpret_cast<const float4*>(raw + p * 4);
    const float4 d = *reinterpret_cast<const float4*>(d_raw + p * 4);
    o = d;
    if (!hard) {
      int lo = 0, hi = K - 1;                 // the first cell whose end lies past r
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long)sb[mid + 1] > r) hi = mid; else lo = mid + 1;
      }
      const float wt = weights[p * K + lo];
      o.x = wt * o.x, o.y = wt * o.y, o.z = wt * o.z, o.w = wt * o.w;
    }
    // (left to right, each product rounded once: w d_raw raw (1 - raw))
    o.x = o.x * rr.x * (1.f - rr.x);
    o.y = o.y * rr.y * (1.f - rr.y);
    o.z = o.z * rr.z * (1.f - rr.z);
    if (deg == 0) {                           // the cell's row holds s = sigmoid(lin) (models/nerf.py:140-141): its derivative here
      const float4 s = *reinterpret_cast<const float4*>(sub_out + r * 4);
      o.x = o.x * s.x * (1.f - s.x), o.y = o.y * s.y * (1.f - s.y), o.z = o.z * s.z * (1.f - s.z);
    }
    const float* dd = dirs + (p / rows_per_group) * 3;
    dx = dd[0], dy = dd[1], dz = dd[2];
  }
  *reinterpret_cast<float4*>(q + r * 4) = o;
  dirs_packed[r * 3 + 0] = dx;
  dirs_packed[r * 3 + 1] = dy;
  dirs_packed[r * 3 + 2] = dz;
}

constexpr int CF_KC = 25;                 // rows of Wc per LDS chunk (one colour at degree 4)
constexpr int CF_RPG = 4;                 // rows per 16-lane group and tile: a chunk in LDS serves 64 rows
constexpr int CF_TILE = 16 * CF_RPG;
constexpr int CF_MAXK = 3 * SH_MAXB;

// rows k0 .. k0 + nk of Wc [3 B, H2] into LDS in the 16-lane row layout (sh_fold's), by the whole block; the caller's barriers around it
template <typename RH, int H2>
__device__ __forceinline__ void coef_stage(const float* __restrict__ wc, int k0, int nk, float (*wl)[16][RH::VPL]) {
  for (int e = threadIdx.x; e < nk * H2; e += 256) {
    const int kk = e / H2, col = e - kk * H2;
    const int chunk = col / RH::EPC, within = col - chunk * RH::EPC;      // the inverse of Row16::col
    wl[kk][chunk & 15][(chunk >> 4) * RH::EPC + within] = wc[(long)(k0 + kk) * H2 + col];
  }
}

static int coef_blocks(long n) {
  const long t = (n + CF_TILE - 1) / CF_TILE;
  return t > 1024 ? 1024 : (t < 1 ? 1 : (int)t);
}

// out[r] = (h2[r] Wc^T + bc  [3 B], softplus(y[r] . ws + bs + noise[r] - 1)) with row stride `stride` floats: a cell's slice of the packed
// rows.  No basis, no fold.  A block walks tiles of 64 rows, a 16-lane group four of them; a linear output is the existing `coef`
// expression (per-lane products in value order, sum16, + bias).  Lane k & 15 keeps output k: a group stores 16 outputs as one run.
template <typename T_, int M, int H2>
__global__ __launch_bounds__(256) void heads_coef_fwd_kernel(const T_* __restrict__ y, const T_* __restrict__ h2, const float* __restrict__ ws,
                                                             const float* __restrict__ bs, const float* __restrict__ wc,
                                                             const float* __restrict__ bc, const float* __restrict__ noise, int deg,
                                                             int inner_sigmoid, long n, float* __restrict__ out, long stride) {
  using RY = Row16<T_, M>;
  using RH = Row16<T_, H2>;
  __shared__ float wl[CF_KC][16][RH::VPL];
  const int j = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int K3 = 3 * (deg + 1) * (deg + 1);
  float wsv[RY::VPL];
  RY::loadf(ws, j, wsv);
  const float b_s = bs[0];
  const long n_tiles = (n + CF_TILE - 1) / CF_TILE;
  for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    float hv[CF_RPG][RH::VPL];
    long ri[CF_RPG];
#pragma unroll
    for (int i = 0; i < CF_RPG; ++i) {
      const long r = t * CF_TILE + grp + 16 * i;
      ri[i] = r < n ? r : -1;
      const long rc = r < n ? r : n - 1;      // (rows past the end: a valid row is read, nothing is stored)
      float yv[RY::VPL];
      RY::load(y + rc * M, j, yv);
      RH::load(h2 + rc * H2, j, hv[i]);
      float s = 0.f;
#pragma unroll
      for (int v = 0; v < RY::VPL; ++v) s += yv[v] * wsv[v];
      s = sum16(s);
      if (j == 0 && r < n) {
        const float uu = s + b_s + (noise ? noise[r] : 0.f) - 1.f;      // ShiftedSoftplus, models/nerf.py:68-69
        out[r * stride + K3] = uu > 20.f ? uu : log1pf(expf(uu));
      }
    }
    for (int k0 = 0; k0 < K3; k0 += CF_KC) {
      const int nk = K3 - k0 < CF_KC ? K3 - k0 : CF_KC;
      __syncthreads();                        // (the previous chunk's readers are done)
      coef_stage<RH, H2>(wc, k0, nk, wl);
      __syncthreads();
      float keep[CF_RPG];
#pragma unroll
      for (int i = 0; i < CF_RPG; ++i) keep[i] = 0.f;
#pragma unroll 1
      for (int kk = 0; kk < nk; ++kk) {
        float wv[RH::VPL];
#pragma unroll
        for (int v = 0; v < RH::VPL; ++v) wv[v] = wl[kk][j][v];
        const float bk = bc[k0 + kk];
#pragma unroll
        for (int i = 0; i < CF_RPG; ++i) {
          float a = 0.f;
#pragma unroll
          for (int v = 0; v < RH::VPL; ++v) a += hv[i][v] * wv[v];
          a = sum16(a) + bk;
          if (inner_sigmoid) a = 1.f / (1.f + expf(-a));
          if ((kk & 15) == j) keep[i] = a;
        }
        if ((kk & 15) == 15 || kk == nk - 1) {
          const int kb = kk & ~15;
          if (kb + j <= kk) {
#pragma unroll
            for (int i = 0; i < CF_RPG; ++i)
              if (ri[i] >= 0) out[ri[i] * stride + k0 + kb + j] = keep[i];
          }
        }
      }
    }
  }
}

// The data half of the backward per row: g[k = c B + b] = q_c Y_b(dirs[r]) (one thread per row of the tile, into LDS), then
// dh2[r] = sum_k g[k] Wc[k] masked by h2 > 0 (the 16-lane layout, Wc in chunks like the forward), dsig = q_3 softplus'(u) from the
// cell's own sigma output, group_colsum[r] = the dh2 row as stored.  The block's sums for d_w_sigma and d_b_sigma -> partial[block]
// ([M | sum, rounding errors], heads_sh_bwd_kernel's format and its compensated pair: sh_bsig_reduce_kernel finishes it).
template <typename T_, int M, int H2>
__global__ __launch_bounds__(256) void heads_coef_bwd_kernel(const T_* __restrict__ y, const T_* __restrict__ h2, const float* __restrict__ wc,
                                                             const float* __restrict__ q, const float* __restrict__ dirs,
                                                             const float* __restrict__ sigma, long sigma_stride, long n, int deg,
                                                             T_* __restrict__ dh2, float* __restrict__ dsig, float* __restrict__ colsum,
                                                             float* __restrict__ partial) {
  using RY = Row16<T_, M>;
  using RH = Row16<T_, H2>;
  __shared__ float wl[CF_KC][16][RH::VPL];
  __shared__ float gl[CF_TILE][CF_MAXK + 1];
  __shared__ float dsl[CF_TILE];
  const int j = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int B = (deg + 1) * (deg + 1), K3 = 3 * B;
  float aws[RY::VPL], abs_ = 0.f, abs_lo = 0.f;      // (the pair: threads 0 .. 63, one tile row each)
#pragma unroll
  for (int v = 0; v < RY::VPL; ++v) aws[v] = 0.f;
  const long n_tiles = (n + CF_TILE - 1) / CF_TILE;
  for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    if (threadIdx.x < CF_TILE) {
      const long r = t * CF_TILE + threadIdx.x;
      float4 qq = make_float4(0.f, 0.f, 0.f, 0.f);
      float Y[SH_MAXB];
      float dsp = 0.f;
      if (r < n) {
        qq = *(const float4*)(q + r * 4);
        sh_basis(deg, dirs[r * 3], dirs[r * 3 + 1], dirs[r * 3 + 2], Y);
        const float sg = sigma[r * sigma_stride];
        dsp = qq.w * -expm1f(-sg);            // softplus'(u) = 1 - exp(-softplus(u))
        dsig[r] = dsp;
        // the bias term once more in double, carried as a compensated pair (heads_sh_bwd_kernel: signed terms that cancel)
        const double t_ = (double)qq.w * (1.0 - exp(-(double)sg));
        const float th_ = (float)t_;
        float e_;
        two_sum(abs_, th_, abs_, e_);
        abs_lo += e_ + (float)(t_ - (double)th_);
      } else {
#pragma unroll
        for (int b = 0; b < SH_MAXB; ++b) Y[b] = 0.f;
      }
#pragma unroll
      for (int b = 0; b < SH_MAXB; ++b) {
        if (b < B) {
          gl[threadIdx.x][b] = qq.x * Y[b];
          gl[threadIdx.x][B + b] = qq.y * Y[b];
          gl[threadIdx.x][2 * B + b] = qq.z * Y[b];
        }
      }
      dsl[threadIdx.x] = dsp;
    }
    __syncthreads();
    float o[CF_RPG][RH::VPL];
    unsigned pos[CF_RPG];
#pragma unroll
    for (int i = 0; i < CF_RPG; ++i) {
      const int rr = grp + 16 * i;
      const long r = t * CF_TILE + rr;
      const long rc = r < n ? r : n - 1;
      float yv[RY::VPL], hv[RH::VPL];
      RY::load(y + rc * M, j, yv);
      RH::load(h2 + rc * H2, j, hv);
      const float dsp = dsl[rr];              // (0 for a row past the end)
      pos[i] = 0u;
#pragma unroll
      for (int v = 0; v < RY::VPL; ++v) aws[v] += dsp * yv[v];
#pragma unroll
      for (int v = 0; v < RH::VPL; ++v) { o[i][v] = 0.f; pos[i] |= hv[v] > 0.f ? 1u << v : 0u; }
    }
    for (int k0 = 0; k0 < K3; k0 += CF_KC) {
      const int nk = K3 - k0 < CF_KC ? K3 - k0 : CF_KC;
      __syncthreads();                        // (the previous chunk's readers are done)
      coef_stage<RH, H2>(wc, k0, nk, wl);
      __syncthreads();
#pragma unroll 1
      for (int kk = 0; kk < nk; ++kk) {
        float wv[RH::VPL];
#pragma unroll
        for (int v = 0; v < RH::VPL; ++v) wv[v] = wl[kk][j][v];
#pragma unroll
        for (int i = 0; i < CF_RPG; ++i) {
          const float gk = gl[grp + 16 * i][k0 + kk];
#pragma unroll
          for (int v = 0; v < RH::VPL; ++v) o[i][v] = fmaf(gk, wv[v], o[i][v]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < CF_RPG; ++i) {
      const long r = t * CF_TILE + grp + 16 * i;
      if (r >= n) continue;
#pragma unroll
      for (int v = 0; v < RH::VPL; ++v) o[i][v] = (pos[i] >> v) & 1u ? o[i][v] + 0.f : 0.f;      // (+ 0: no -0 from a zero gradient)
      RH::store(dh2 + r * H2, j, o[i]);
      if (colsum) {
        float* cs = colsum + r * H2;
        if constexpr (sizeof(T_) == 2) {
#pragma unroll
          for (int v = 0; v < RH::VPL; v += 2) {          // what the store kept: the values rounded to T_
            const uint32_t pk = pack_bf16x2(o[i][v], o[i][v + 1]);
            cs[RH::col(j, v)] = bf16_to_f32((bf16_t)(pk & 0xFFFF));
            cs[RH::col(j, v + 1)] = bf16_to_f32((bf16_t)(pk >> 16));
          }
        } else {
#pragma unroll
          for (int v = 0; v < RH::VPL; ++v) cs[RH::col(j, v)] = o[i][v];
        }
      }
    }
    __syncthreads();                          // (the next tile overwrites gl and dsl)
  }
  // block-level reduction of the sigma head's sums, the 16 row groups one after the other, then the 64 pairs in thread order
  __shared__ float red[M + 2];
  __shared__ float ph[CF_TILE], pl[CF_TILE];
  for (int t = threadIdx.x; t < M + 2; t += 256) red[t] = 0.f;
  if (threadIdx.x < CF_TILE) { ph[threadIdx.x] = abs_; pl[threadIdx.x] = abs_lo; }
  __syncthreads();
  for (int gq = 0; gq < 16; ++gq) {
    if (grp == gq) {
#pragma unroll
      for (int v = 0; v < RY::VPL; ++v) red[RY::col(j, v)] += aws[v];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float S = 0.f, Cc = 0.f;
    for (int l = 0; l < CF_TILE; ++l) {
      float e_;
      two_sum(S, ph[l], S, e_);
      Cc += e_ + pl[l];
    }
    red[M] = S;
    red[M + 1] = Cc;
  }
  __syncthreads();
  float* part = partial + (size_t)blockIdx.x * (M + 2);
  for (int t = threadIdx.x; t < M + 2; t += 256) part[t] = red[t];
}

// The parameter half: d_Wc[k] = sum_r g[r][k] h2[r], d_bc[k] = sum_r g[r][k].  A thread owns one column of h2 and a run of the 3 B
// outputs k, its accumulators in registers over every tile the block walks (rows ascending); a tile's g rows and h2 rows meet in LDS.
// partial[block] = [3 B x H2 | 3 B sums | 3 B rounding errors]; ordered_reduce_kernel adds the blocks' weight parts.  The bias sums are
// few and each is one scalar over every row, signed terms that cancel: like d_b_sigma they are carried as compensated fp32 pairs from
// the first add to the last (coef_bc_reduce_kernel).  fp32 on the vector pipe.
constexpr int CW_TILE = 32;
static int coef_wgrad_blocks(long n) {
  const long t = (n + CW_TILE - 1) / CW_TILE;
  return t > 512 ? 512 : (t < 1 ? 1 : (int)t);
}

template <typename T_, int H2, int DEG>
__global__ __launch_bounds__(256) void heads_coef_wgrad_kernel(const T_* __restrict__ h2, const float* __restrict__ q,
                                                               const float* __restrict__ dirs, long n, float* __restrict__ partial) {
  constexpr int B = (DEG + 1) * (DEG + 1), K3 = 3 * B, KG = 256 / H2, NA = (K3 + KG - 1) / KG, GS = NA * KG;
  constexpr int EPC = 16 / (int)sizeof(T_), CPR = H2 / EPC;
  static_assert(KG >= 1 && KG * H2 == 256, "one column per thread");
  __shared__ float hl[CW_TILE][H2];
  __shared__ float gl[CW_TILE][GS];
  const int col = threadIdx.x % H2, kg = threadIdx.x / H2;
  float acc[NA], accb = 0.f, accb_lo = 0.f;
#pragma unroll
  for (int i = 0; i < NA; ++i) acc[i] = 0.f;
  const long n_tiles = (n + CW_TILE - 1) / CW_TILE;
  for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const long r0 = t * CW_TILE;
    if (threadIdx.x < CW_TILE) {
      const long r = r0 + threadIdx.x;
      float4 qq = make_float4(0.f, 0.f, 0.f, 0.f);
      float Y[SH_MAXB];
      if (r < n) {
        qq = *(const float4*)(q + r * 4);
        sh_basis(DEG, dirs[r * 3], dirs[r * 3 + 1], dirs[r * 3 + 2], Y);
      } else {
#pragma unroll
        for (int b = 0; b < SH_MAXB; ++b) Y[b] = 0.f;
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        gl[threadIdx.x][b] = qq.x * Y[b];
        gl[threadIdx.x][B + b] = qq.y * Y[b];
        gl[threadIdx.x][2 * B + b] = qq.z * Y[b];
      }
#pragma unroll
      for (int k = K3; k < GS; ++k) gl[threadIdx.x][k] = 0.f;
    }
    for (int ch = threadIdx.x; ch < CW_TILE * CPR; ch += 256) {
      const int row = ch / CPR, cc = ch - row * CPR;
      uint4 u = make_uint4(0u, 0u, 0u, 0u);                 // (rows past the end: zeros)
      if (r0 + row < n) u = *(const uint4*)(h2 + (r0 + row) * H2 + cc * EPC);
      float* dst = &hl[row][cc * EPC];
      if constexpr (sizeof(T_) == 2) {
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          dst[2 * i] = bf16_to_f32((bf16_t)(w[i] & 0xFFFF));
          dst[2 * i + 1] = bf16_to_f32((bf16_t)(w[i] >> 16));
        }
      } else {
        dst[0] = __uint_as_float(u.x); dst[1] = __uint_as_float(u.y); dst[2] = __uint_as_float(u.z); dst[3] = __uint_as_float(u.w);
      }
    }
    __syncthreads();
#pragma unroll 2
    for (int r = 0; r < CW_TILE; ++r) {
      const float h = hl[r][col];
      const float* g = &gl[r][kg * NA];
#pragma unroll
      for (int i = 0; i < NA; ++i) acc[i] = fmaf(g[i], h, acc[i]);
    }
    if ((int)threadIdx.x < K3) {
      for (int r = 0; r < CW_TILE; ++r) {
        float e_;
        two_sum(accb, gl[r][threadIdx.x], accb, e_);
        accb_lo += e_;
      }
    }
    __syncthreads();                          // (the next tile overwrites both)
  }
  float* part = partial + (size_t)blockIdx.x * (K3 * H2 + 2 * K3);
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int k = kg * NA + i;
    if (k < K3) part[k * H2 + col] = acc[i];
  }
  if ((int)threadIdx.x < K3) {
    part[K3 * H2 + threadIdx.x] = accb;
    part[K3 * H2 + K3 + threadIdx.x] = accb_lo;
  }
}

// d_b_color[k] += the blocks' pairs (columns off + k and off + K3 + k of partial, row stride np), added in ascending order with two_sum:
// sh_bsig_reduce_kernel's scheme, one workgroup of one wave per output.  Fixed order: the same bits every run.
__global__ __launch_bounds__(64) void coef_bc_reduce_kernel(const float* __restrict__ partial, int n_blocks, int np, int off, int K3,
                                                            float* __restrict__ d_bc) {
  __shared__ float hi[64], lo[64];
  const int k = blockIdx.x;
  const int per = (n_blocks + 63) / 64, b0 = threadIdx.x * per, b1 = n_blocks < b0 + per ? n_blocks : b0 + per;
  float s = 0.f, c = 0.f;
  for (int b = b0; b < b1; ++b) {
    const float* q = partial + (size_t)b * np + off + k;
    float e_;
    two_sum(s, q[0], s, e_);
    c += e_ + q[K3];
  }
  hi[threadIdx.x] = s;
  lo[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    float S = 0.f, Cc = 0.f;
    for (int l = 0; l < 64; ++l) {
      float e_;
      two_sum(S, hi[l], S, e_);
      Cc += e_ + lo[l];
    }
    float e_;
    two_sum(d_bc[k], S, S, e_);
    d_bc[k] = S + (Cc + e_);
  }
}

// the two parts of swn_heads_coef_bwd's workspace, each a multiple of 64 floats: sized by the block counts, which are capped
struct CoefWs { size_t sig, wg; };
static CoefWs coef_ws(long n, int model_dim, int h2_dim, int deg) {
  const int B = (deg + 1) * (deg + 1);
  auto up = [](size_t v) { return (v + 63) / 64 * 64; };
  CoefWs w;
  w.sig = up((size_t)coef_blocks(n) * (size_t)(model_dim + 2));
  w.wg = up((size_t)coef_wgrad_blocks(n) * (size_t)(3 * B * h2_dim + 6 * B));
  return w;
}

}  // namespace swn

using namespace swn;

#define SWN_SH_DISPATCH(MACRO)                                                                                                    \
  do {                                                                                                                            \
    if (dtype == SWN_HALF) {                                                                                                      \
      if (model_dim == 256 && h2_dim == 128) MACRO(bf16_t, 256, 128); else if (model_dim == 512 && h2_dim == 256) MACRO(bf16_t, 512, 256); \
      else if (model_dim == 256) MACRO(bf16_t, 256, 256); else MACRO(bf16_t, 512, 128);                                           \
    } else {                                                                                                                      \
      if (model_dim == 256 && h2_dim == 128) MACRO(float, 256, 128); else if (model_dim == 512 && h2_dim == 256) MACRO(float, 512, 256); \
      else if (model_dim == 256) MACRO(float, 256, 256); else MACRO(float, 512, 128);                                             \
    }                                                                                                                             \
  } while (0)

extern "C" int swn_heads_sh_fwd(const void* y, const void* h2, int dtype, const float* w_sigma, const float* b_sigma, const float* w_color,
                                const float* b_color, const float* sigma_noise, const float* dirs, int rows_per_group, int deg,
                                int n_points, int model_dim, int h2_dim, float* raw, float* coef, void* stream) {
  SWN_CHECK(dtype == SWN_F32 || dtype == SWN_HALF, "swn_heads_sh_fwd: bad dtype");
  SWN_CHECK(y && h2 && w_sigma && b_sigma && w_color && b_color && dirs && raw, "swn_heads_sh_fwd: null pointer");
  SWN_CHECK((model_dim == 256 || model_dim == 512) && (h2_dim == 128 || h2_dim == 256),
            "swn_heads_sh_fwd: model_dim in {256,512}, h2_dim in {128,256}");
  SWN_CHECK(deg >= 0 && deg <= 4, "swn_heads_sh_fwd: deg %d outside 0..4", deg);
  SWN_CHECK(n_points >= 0 && rows_per_group > 0 && n_points % rows_per_group == 0,
            "swn_heads_sh_fwd: rows_per_group %d must be positive and divide n_points %d", rows_per_group, n_points);
  if (n_points == 0) return 0;
  const int blocks = sh_blocks(n_points / rows_per_group);
#define SWN_SHF(T_, M_, H_) hipLaunchKernelGGL((heads_sh_fwd_kernel<T_, M_, H_>), dim3(blocks), dim3(256), 0, as_stream(stream), (const T_*)y, \
                                               (const T_*)h2, w_sigma, b_sigma, w_color, b_color, sigma_noise, dirs, rows_per_group, deg,      \
                                               (long)n_points, raw, coef)
  SWN_SH_DISPATCH(SWN_SHF);
#undef SWN_SHF
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_heads_sh_bwd_workspace_bytes(int n_points, int model_dim, int h2_dim, int rows_per_group, int deg, size_t* bytes) {
  SWN_CHECK(bytes && n_points >= 0 && rows_per_group > 0 && deg >= 0 && deg <= 4 && model_dim > 0 && h2_dim > 0,
            "swn_heads_sh_bwd_workspace_bytes: bad arguments");
  const ShWs w = sh_ws(n_points, model_dim, h2_dim, rows_per_group, deg);
  *bytes = (w.sig + w.ray + w.wg) * sizeof(float);
  return 0;
}

extern "C" int swn_heads_sh_bwd(const void* y, const void* h2, int dtype, const float* w_color, const float* b_color, const float* dirs,
                                const float* raw, const float* d_raw, int n_points, int model_dim, int h2_dim, int rows_per_group, int deg,
                                void* dh2, float* dsig, float* d_w_sigma, float* d_b_sigma, float* d_w_color, float* d_b_color,
                                float* group_colsum, void* workspace, size_t workspace_bytes, void* stream) {
  SWN_CHECK(dtype == SWN_F32 || dtype == SWN_HALF, "swn_heads_sh_bwd: bad dtype");
  SWN_CHECK(y && h2 && w_color && b_color && dirs && raw && d_raw && dh2 && dsig && d_w_sigma && d_b_sigma && d_w_color && d_b_color && workspace,
            "swn_heads_sh_bwd: null pointer");      // (group_colsum may be NULL)
  SWN_CHECK((model_dim == 256 || model_dim == 512) && (h2_dim == 128 || h2_dim == 256),
            "swn_heads_sh_bwd: model_dim in {256,512}, h2_dim in {128,256}");
  SWN_CHECK(deg >= 0 && deg <= 4, "swn_heads_sh_bwd: deg %d outside 0..4", deg);
  SWN_CHECK(n_points >= 0 && rows_per_group > 0 && n_points % rows_per_group == 0,
            "swn_heads_sh_bwd: rows_per_group %d must be positive and divide n_points %d", rows_per_group, n_points);
  size_t need = 0;
  swn_heads_sh_bwd_workspace_bytes(n_points, model_dim, h2_dim, rows_per_group, deg, &need);
  SWN_CHECK(workspace_bytes >= need, "swn_heads_sh_bwd: workspace of %zu bytes, need %zu", workspace_bytes, need);
  if (n_points == 0) return 0;
  const long n_units = n_points / rows_per_group;
  const int B = (deg + 1) * (deg + 1), blocks = sh_blocks(n_units), nb2 = cdiv(n_units, SRB);
  const ShWs w = sh_ws(n_points, model_dim, h2_dim, rows_per_group, deg);
  float* p_sig = (float*)workspace;
  float* ray_acc = p_sig + w.sig;
  float* p_wg = ray_acc + w.ray;
#define SWN_SHB(T_, M_, H_) hipLaunchKernelGGL((heads_sh_bwd_kernel<T_, M_, H_>), dim3(blocks), dim3(256), 0, as_stream(stream), (const T_*)y, \
                                               (const T_*)h2, w_color, b_color, dirs, raw, d_raw, (long)n_points, rows_per_group, deg,         \
                                               (T_*)dh2, dsig, group_colsum, ray_acc, p_sig)
  SWN_SH_DISPATCH(SWN_SHB);
#undef SWN_SHB
  OrdDst od{{d_w_sigma, nullptr, nullptr, nullptr}, {model_dim, 0, 0, 0}};      // (the two columns behind it go to no destination here)
  ordered_reduce_async(p_sig, blocks, model_dim + 2, od, true, as_stream(stream));
  hipLaunchKernelGGL(sh_bsig_reduce_kernel, dim3(1), dim3(64), 0, as_stream(stream), p_sig, blocks, model_dim, d_b_sigma);
  hipLaunchKernelGGL(sh_wgrad_kernel, dim3(nb2), dim3(256), 0, as_stream(stream), ray_acc, dirs, n_units, deg, h2_dim, p_wg);
  OrdDst oc{{d_w_color, d_b_color, nullptr, nullptr}, {3 * B * h2_dim, 3 * B, 0, 0}};
  ordered_reduce_async(p_wg, nb2, 3 * B * h2_dim + 3 * B, oc, true, as_stream(stream));
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_cells_blend_sh(const float* weights, const int32_t* slot, const int32_t* begin, const float* sub_out, long total,
                                  const float* dirs, int rows_per_group, int deg, int n_points, int n_cells, int hard, float* raw,
                                  float* coef_out, void* stream) {
  SWN_CHECK(n_cells >= 1 && n_cells <= BSH_MAX_CELLS, "swn_cells_blend_sh: n_cells %d outside [1, %d]", n_cells, BSH_MAX_CELLS);
  SWN_CHECK(deg >= 0 && deg <= 4, "swn_cells_blend_sh: deg %d outside 0..4", deg);
  SWN_CHECK(rows_per_group >= 1, "swn_cells_blend_sh: rows_per_group %d < 1", rows_per_group);
  SWN_CHECK(n_points >= 1 && total >= 1, "swn_cells_blend_sh: bad sizes (n_points %d, total %ld)", n_points, total);
  SWN_CHECK(n_points % rows_per_group == 0, "swn_cells_blend_sh: n_points %d is no multiple of rows_per_group %d", n_points, rows_per_group);
  SWN_CHECK(weights && slot && begin && sub_out && dirs && raw, "swn_cells_blend_sh: null pointer");      // (coef_out may be NULL)
  SWN_CHECK(((((uintptr_t)raw) | (deg == 0 ? ((uintptr_t)sub_out) | ((uintptr_t)coef_out) : 0)) & 15) == 0,
            "swn_cells_blend_sh: raw (deg 0: sub_out and coef_out too) must be 16-byte aligned");
#define SWN_BSH(D_) hipLaunchKernelGGL(cells_blend_sh_kernel<D_>, dim3(cdiv(n_points, BSH_TILE)), dim3(256), 0, as_stream(stream), weights, \
                                       slot, begin, sub_out, total, dirs, rows_per_group, n_cells, hard, (long)n_points, raw, coef_out)
  switch (deg) {
    case 0:
      hipLaunchKernelGGL(cells_blend_sh0_kernel, dim3(cdiv(n_points, 256)), dim3(256), 0, as_stream(stream), weights, slot, begin, sub_out,
                         total, dirs, rows_per_group, n_cells, hard, (long)n_points, raw, coef_out);
      break;
    case 1: SWN_BSH(1); break;
    case 2: SWN_BSH(2); break;
    case 3: SWN_BSH(3); break;
    default: SWN_BSH(4); break;
  }
#undef SWN_BSH
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_cells_blend_sh_bwd(const float* weights, const int32_t* rows, const int32_t* begin, const float* raw, const float* d_raw,
                                      const float* dirs, const float* sub_out, long total, int rows_per_group, int deg, int n_points,
                                      int n_cells, int hard, float* q, float* dirs_packed, void* stream) {
  SWN_CHECK(n_cells >= 1 && n_cells <= BSH_MAX_CELLS, "swn_cells_blend_sh_bwd: n_cells %d outside [1, %d]", n_cells, BSH_MAX_CELLS);
  SWN_CHECK(deg >= 0 && deg <= 4, "swn_cells_blend_sh_bwd: deg %d outside 0..4", deg);
  SWN_CHECK(rows_per_group >= 1, "swn_cells_blend_sh_bwd: rows_per_group %d < 1", rows_per_group);
  SWN_CHECK(n_points >= 1 && total >= 0, "swn_cells_blend_sh_bwd: bad sizes (n_points %d, total %ld)", n_points, total);
  SWN_CHECK(n_points % rows_per_group == 0, "swn_cells_blend_sh_bwd: n_points %d is no multiple of rows_per_group %d", n_points, rows_per_group);
  SWN_CHECK(rows && raw && d_raw && dirs && q && dirs_packed && (hard || (weights && begin)) && (deg != 0 || sub_out),
            "swn_cells_blend_sh_bwd: null pointer");      // (sub_out is read at degree 0 only)
  if (total == 0) return 0;
  SWN_CHECK(((((uintptr_t)raw) | ((uintptr_t)d_raw) | ((uintptr_t)q) | (deg == 0 ? (uintptr_t)sub_out : 0)) & 15) == 0,
            "swn_cells_blend_sh_bwd: raw, d_raw, q (deg 0: sub_out too) must be 16-byte aligned");
  SWN_CHECK(total <= 2147483647l * 256, "swn_cells_blend_sh_bwd: %ld rows exceed the grid", total);      // (cdiv returns an int)
  hipLaunchKernelGGL(cells_blend_sh_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), weights, rows, begin, raw, d_raw,
                     dirs, sub_out, total, rows_per_group, n_cells, hard, deg, (long)n_points, q, dirs_packed);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_heads_coef_fwd(const void* y, const void* h2, int dtype, const float* w_sigma, const float* b_sigma, const float* w_color,
                                  const float* b_color, const float* sigma_noise, int deg, int inner_sigmoid, int n_rows, int model_dim,
                                  int h2_dim, float* out, long out_stride, void* stream) {
  SWN_CHECK(dtype == SWN_F32 || dtype == SWN_HALF, "swn_heads_coef_fwd: bad dtype");
  SWN_CHECK((model_dim == 256 || model_dim == 512) && (h2_dim == 128 || h2_dim == 256),
            "swn_heads_coef_fwd: model_dim in {256,512}, h2_dim in {128,256}");
  SWN_CHECK(deg >= 0 && deg <= 4, "swn_heads_coef_fwd: deg %d outside 0..4", deg);
  SWN_CHECK(!inner_sigmoid || deg == 0, "swn_heads_coef_fwd: the inner sigmoid belongs to degree 0 (rgb_dim == 3), not to deg %d", deg);
  SWN_CHECK(n_rows >= 0 && out_stride >= 3 * (deg + 1) * (deg + 1) + 1, "swn_heads_coef_fwd: bad sizes (n_rows %d, out_stride %ld)", n_rows,
            out_stride);
  SWN_CHECK(y && h2 && w_sigma && b_sigma && w_color && b_color && out, "swn_heads_coef_fwd: null pointer");
  if (n_rows == 0) return 0;
  const int blocks = coef_blocks(n_rows);
#define SWN_CFF(T_, M_, H_) hipLaunchKernelGGL((heads_coef_fwd_kernel<T_, M_, H_>), dim3(blocks), dim3(256), 0, as_stream(stream), (const T_*)y, \
                                               (const T_*)h2, w_sigma, b_sigma, w_color, b_color, sigma_noise, deg, inner_sigmoid ? 1 : 0,       \
                                               (long)n_rows, out, out_stride)
  SWN_SH_DISPATCH(SWN_CFF);
#undef SWN_CFF
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_heads_coef_bwd_workspace_bytes(int n_rows, int model_dim, int h2_dim, int deg, size_t* bytes) {
  SWN_CHECK(bytes && n_rows >= 0 && deg >= 0 && deg <= 4 && model_dim > 0 && h2_dim > 0, "swn_heads_coef_bwd_workspace_bytes: bad arguments");
  const CoefWs w = coef_ws(n_rows, model_dim, h2_dim, deg);
  *bytes = (w.sig + w.wg) * sizeof(float);
  return 0;
}

template <typename T_, int H2>
static void coef_wgrad_launch(int deg, int blocks, hipStream_t s, const void* h2, const float* q, const float* dirs, long n, float* partial) {
  switch (deg) {
    case 0: hipLaunchKernelGGL((heads_coef_wgrad_kernel<T_, H2, 0>), dim3(blocks), dim3(256), 0, s, (const T_*)h2, q, dirs, n, partial); break;
    case 1: hipLaunchKernelGGL((heads_coef_wgrad_kernel<T_, H2, 1>), dim3(blocks), dim3(256), 0, s, (const T_*)h2, q, dirs, n, partial); break;
    case 2: hipLaunchKernelGGL((heads_coef_wgrad_kernel<T_, H2, 2>), dim3(blocks), dim3(256), 0, s, (const T_*)h2, q, dirs, n, partial); break;
    case 3: hipLaunchKernelGGL((heads_coef_wgrad_kernel<T_, H2, 3>), dim3(blocks), dim3(256), 0, s, (const T_*)h2, q, dirs, n, partial); break;
    default: hipLaunchKernelGGL((heads_coef_wgrad_kernel<T_, H2, 4>), dim3(blocks), dim3(256), 0, s, (const T_*)h2, q, dirs, n, partial); break;
  }
}

extern "C" int swn_heads_coef_bwd(const void* y, const void* h2, int dtype, const float* w_color, const float* q, const float* dirs,
                                  const float* sigma, long sigma_stride, int n_rows, int model_dim, int h2_dim, int deg, void* dh2,
                                  float* dsig, float* d_w_sigma, float* d_b_sigma, float* d_w_color, float* d_b_color, float* group_colsum,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  SWN_CHECK(dtype == SWN_F32 || dtype == SWN_HALF, "swn_heads_coef_bwd: bad dtype");
  SWN_CHECK((model_dim == 256 || model_dim == 512) && (h2_dim == 128 || h2_dim == 256),
            "swn_heads_coef_bwd: model_dim in {256,512}, h2_dim in {128,256}");
  SWN_CHECK(deg >= 0 && deg <= 4, "swn_heads_coef_bwd: deg %d outside 0..4", deg);
  SWN_CHECK(n_rows >= 0 && sigma_stride >= 1, "swn_heads_coef_bwd: bad sizes (n_rows %d, sigma_stride %ld)", n_rows, sigma_stride);
  SWN_CHECK(y && h2 && w_color && q && dirs && sigma && dh2 && dsig && d_w_sigma && d_b_sigma && d_w_color && d_b_color && workspace,
            "swn_heads_coef_bwd: null pointer");      // (group_colsum may be NULL)
  SWN_CHECK((((uintptr_t)q) & 15) == 0, "swn_heads_coef_bwd: q must be 16-byte aligned");
  const CoefWs w = coef_ws(n_rows, model_dim, h2_dim, deg);
  SWN_CHECK(workspace_bytes >= (w.sig + w.wg) * sizeof(float), "swn_heads_coef_bwd: workspace of %zu bytes, need %zu", workspace_bytes,
            (w.sig + w.wg) * sizeof(float));
  if (n_rows == 0) return 0;
  const int B = (deg + 1) * (deg + 1), blocks = coef_blocks(n_rows), nb2 = coef_wgrad_blocks(n_rows);
  float* p_sig = (float*)workspace;
  float* p_wg = p_sig + w.sig;
#define SWN_CFB(T_, M_, H_) hipLaunchKernelGGL((heads_coef_bwd_kernel<T_, M_, H_>), dim3(blocks), dim3(256), 0, as_stream(stream), (const T_*)y, \
                                               (const T_*)h2, w_color, q, dirs, sigma, sigma_stride, (long)n_rows, deg, (T_*)dh2, dsig,          \
                                               group_colsum, p_sig)
  SWN_SH_DISPATCH(SWN_CFB);
#undef SWN_CFB
  OrdDst od{{d_w_sigma, nullptr, nullptr, nullptr}, {model_dim, 0, 0, 0}};      // (the two columns behind it go to no destination here)
  ordered_reduce_async(p_sig, blocks, model_dim + 2, od, true, as_stream(stream));
  hipLaunchKernelGGL(sh_bsig_reduce_kernel, dim3(1), dim3(64), 0, as_stream(stream), p_sig, blocks, model_dim, d_b_sigma);
  if (dtype == SWN_HALF) {
    if (h2_dim == 128) coef_wgrad_launch<bf16_t, 128>(deg, nb2, as_stream(stream), h2, q, dirs, n_rows, p_wg);
    else coef_wgrad_launch<bf16_t, 256>(deg, nb2, as_stream(stream), h2, q, dirs, n_rows, p_wg);
  } else {
    if (h2_dim == 128) coef_wgrad_launch<float, 128>(deg, nb2, as_stream(stream), h2, q, dirs, n_rows, p_wg);
    else coef_wgrad_launch<float, 256>(deg, nb2, as_stream(stream), h2, q, dirs, n_rows, p_wg);
  }
  OrdDst oc{{d_w_color, nullptr, nullptr, nullptr}, {3 * B * h2_dim, 0, 0, 0}};      // (the bias columns behind it go to no destination here)
  ordered_reduce_async(p_wg, nb2, 3 * B * h2_dim + 6 * B, oc, true, as_stream(stream));
  hipLaunchKernelGGL(coef_bc_reduce_kernel, dim3(3 * B), dim3(64), 0, as_stream(stream), p_wg, nb2, 3 * B * h2_dim + 6 * B, 3 * B * h2_dim,
                     3 * B, d_b_color);
  SWN_LAUNCH_CHECK();
  return 0;
}
