// The residual-expert mix of the MoE layer (use_residual, tutel_moe_layer_nobatch.py:777-788, the DeepSpeed PR-MoE form):
//   c = softmax(x Wc^T + bc)   [P, 2] fp32,    y = y_moe * c[:, 0] + y_res * c[:, 1]
// and its backward.  Both passes stream whole rows: one group of lanes per token, 16-byte loads, the per-token dot products reduced
// across the group's lanes.  The coefficient gradients are per-block partial sums added in a fixed order (no float atomics).
#include "common.hpp"

namespace swn {
namespace {

constexpr int RM_THREADS = 256;
constexpr int RM_WAVES = RM_THREADS / 64;
constexpr int RM_FWD_MAX_BLOCKS = 4096;
constexpr int RM_BWD_MAX_BLOCKS = 1024;

// one 16-byte chunk of a row <-> N fp32 values
template <typename T> struct Chunk;
template <> struct Chunk<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void ld(const float* p, float* v) {
    const float4 q = *(const float4*)p;
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  }
  static __device__ __forceinline__ void st(float* p, const float* v) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct Chunk<bf16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void ld(const bf16_t* p, float* v) {
    const uint4 q = *(const uint4*)p;
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = bf16_to_f32((bf16_t)(w[i] & 0xFFFFu));
      v[2 * i + 1] = bf16_to_f32((bf16_t)(w[i] >> 16));
    }
  }
  static __device__ __forceinline__ void st(bf16_t* p, const float* v) {
    uint4 q;
    q.x = pack_bf16x2(v[0], v[1]); q.y = pack_bf16x2(v[2], v[3]); q.z = pack_bf16x2(v[4], v[5]); q.w = pack_bf16x2(v[6], v[7]);
    *(uint4*)p = q;
  }
};

// the lane layout of a row of M values of type T: LPT lanes per token, NC chunks of VEC values per lane, TPW tokens per wave
template <typename T, int M> struct RowLayout {
  static constexpr int VEC = Chunk<T>::N;
  static constexpr int CH = M / VEC;
  static constexpr int LPT = CH < 64 ? CH : 64;
  static constexpr int NC = CH / LPT;
  static constexpr int TPW = 64 / LPT;
  static_assert(M % VEC == 0 && CH % LPT == 0 && LPT >= 1, "row layout");
};

template <int LPT> __device__ __forceinline__ float group_sum(float v) {     // the LPT lanes of one token (aligned groups)
#pragma unroll
  for (int o = LPT / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T, int M>
__global__ __launch_bounds__(RM_THREADS) void residual_mix_fwd_kernel(const T* __restrict__ x, const T* __restrict__ ym,
                                                                      const T* __restrict__ yr, const float* __restrict__ wc,
                                                                      const float* __restrict__ bc, T* __restrict__ y,
                                                                      float* __restrict__ coef, int P) {
  using R = RowLayout<T, M>;
  constexpr int VEC = R::VEC, LPT = R::LPT, NC = R::NC, TPW = R::TPW;
  const int lane = threadIdx.x & 63, sub = lane % LPT, grp = lane / LPT;
  const long wave = ((long)blockIdx.x * RM_THREADS + threadIdx.x) >> 6;
  const long n_waves = (long)gridDim.x * RM_WAVES;
  float w0[NC][VEC], w1[NC][VEC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const int e = (c * LPT + sub) * VEC + i;
      w0[c][i] = wc[e];
      w1[c][i] = wc[M + e];
    }
  const float b0 = bc[0], b1 = bc[1];
  // the loop bound is uniform across the wave (ragged tails are masked, never skipped), so every group runs its shuffles
  for (long base = wave * TPW; base < P; base += n_waves * TPW) {
    const long t = base + grp;
    const bool ok = t < P;
    float xv[NC][VEC], mv[NC][VEC], rv[NC][VEC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const long off = t * M + (c * LPT + sub) * VEC;
      if (ok) {
        Chunk<T>::ld(x + off, xv[c]);
        Chunk<T>::ld(ym + off, mv[c]);
        Chunk<T>::ld(yr + off, rv[c]);
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) xv[c][i] = mv[c][i] = rv[c][i] = 0.f;
      }
    }
    float l0 = 0.f, l1 = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        l0 += xv[c][i] * w0[c][i];
        l1 += xv[c][i] * w1[c][i];
      }
    l0 = group_sum<LPT>(l0) + b0;
    l1 = group_sum<LPT>(l1) + b1;
    const float mx = fmaxf(l0, l1);
    const float e0 = expf(l0 - mx), e1 = expf(l1 - mx);
    const float s = e0 + e1;
    const float c0 = e0 / s, c1 = e1 / s;
    if (!ok) continue;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float o[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) o[i] = mv[c][i] * c0 + rv[c][i] * c1;
      Chunk<T>::st(y + t * M + (c * LPT + sub) * VEC, o);
    }
    if (sub == 0) *(float2*)(coef + 2 * t) = make_float2(c0, c1);
  }
}

// partial[block][0 : 2M] = sum over the block's tokens of dl[t] (x) x[t] (row 0, then row 1), partial[block][2M + j] = sum dl_j
template <typename T, int M>
__global__ __launch_bounds__(RM_THREADS) void residual_mix_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                      const T* __restrict__ ym, const T* __restrict__ yr,
                                                                      const float* __restrict__ coef, const float* __restrict__ wc,
                                                                      T* __restrict__ d_moe, T* __restrict__ d_res, T* __restrict__ dx,
                                                                      float* __restrict__ partial, int P) {
  using R = RowLayout<T, M>;
  constexpr int VEC = R::VEC, LPT = R::LPT, NC = R::NC, TPW = R::TPW;
  constexpr int NP = 2 * M + 2;
  __shared__ float red[RM_WAVES][NP];
  const int lane = threadIdx.x & 63, sub = lane % LPT, grp = lane / LPT, wid = threadIdx.x >> 6;
  float w0[NC][VEC], w1[NC][VEC], a0[NC][VEC], a1[NC][VEC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const int e = (c * LPT + sub) * VEC + i;
      w0[c][i] = wc[e];
      w1[c][i] = wc[M + e];
      a0[c][i] = a1[c][i] = 0.f;
    }
  float db0 = 0.f, db1 = 0.f;
  // block b takes the token groups b, b + gridDim.x, ... of RM_WAVES * TPW tokens (fixed for a given P: the same sums every launch)
  for (long base = ((long)blockIdx.x * RM_WAVES + wid) * TPW; base < P; base += (long)gridDim.x * RM_WAVES * TPW) {
    const long t = base + grp;
    const bool ok = t < P;
    float gv[NC][VEC], xv[NC][VEC], mv[NC][VEC], rv[NC][VEC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const long off = t * M + (c * LPT + sub) * VEC;
      if (ok) {
        Chunk<T>::ld(dy + off, gv[c]);
        Chunk<T>::ld(x + off, xv[c]);
        Chunk<T>::ld(ym + off, mv[c]);
        Chunk<T>::ld(yr + off, rv[c]);
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) gv[c][i] = xv[c][i] = mv[c][i] = rv[c][i] = 0.f;
      }
    }
    const float2 cc = ok ? *(const float2*)(coef + 2 * t) : make_float2(0.f, 0.f);
    float g0 = 0.f, g1 = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        g0 += gv[c][i] * mv[c][i];
        g1 += gv[c][i] * rv[c][i];
      }
    g0 = group_sum<LPT>(g0);
    g1 = group_sum<LPT>(g1);
    // softmax backward: dl_j = c_j (g_j - sum_k c_k g_k)
    const float sg = cc.x * g0 + cc.y * g1;
    const float dl0 = cc.x * (g0 - sg), dl1 = cc.y * (g1 - sg);      // (0 for a masked token: cc = 0)
    db0 += dl0;
    db1 += dl1;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        a0[c][i] += dl0 * xv[c][i];
        a1[c][i] += dl1 * xv[c][i];
      }
    if (!ok) continue;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const long off = t * M + (c * LPT + sub) * VEC;
      float om[VEC], orr[VEC], ox[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        om[i] = cc.x * gv[c][i];
        orr[i] = cc.y * gv[c][i];
        ox[i] = dl0 * w0[c][i] + dl1 * w1[c][i];
      }
      Chunk<T>::st(d_moe + off, om);
      Chunk<T>::st(d_res + off, orr);
      Chunk<T>::st(dx + off, ox);
    }
  }
  // the wave's token groups (lanes with the same sub), then the block's waves in order
#pragma unroll
  for (int o = LPT; o < 64; o <<= 1) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        a0[c][i] += __shfl_xor(a0[c][i], o, 64);
        a1[c][i] += __shfl_xor(a1[c][i], o, 64);
      }
    db0 += __shfl_xor(db0, o, 64);
    db1 += __shfl_xor(db1, o, 64);
  }
  if (grp == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const int e = (c * LPT + sub) * VEC + i;
        red[wid][e] = a0[c][i];
        red[wid][M + e] = a1[c][i];
      }
    if (sub == 0) {
      red[wid][2 * M] = db0;
      red[wid][2 * M + 1] = db1;
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < NP; j += RM_THREADS) {
    float s = red[0][j];
#pragma unroll
    for (int w = 1; w < RM_WAVES; ++w) s += red[w][j];
    partial[(size_t)blockIdx.x * NP + j] = s;
  }
}

template <typename T> constexpr int tokens_per_block(int M) { return RM_WAVES * (64 / ((M / Chunk<T>::N) < 64 ? (M / Chunk<T>::N) : 64)); }

int bwd_blocks(int dtype, int P, int M) {
  const int tpb = dtype == SWN_F32 ? tokens_per_block<float>(M) : tokens_per_block<bf16_t>(M);
  const int b = cdiv(P, tpb);
  return b < 1 ? 1 : (b > RM_BWD_MAX_BLOCKS ? RM_BWD_MAX_BLOCKS : b);
}

bool mix_dim_ok(int M) { return M == 64 || M == 128 || M == 256 || M == 512; }

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <typename T>
int fwd_launch(const void* x, const void* ym, const void* yr, const float* wc, const float* bc, int P, int M, void* y, float* coef,
               hipStream_t s) {
  int blocks = cdiv(P, tokens_per_block<T>(M));
  blocks = blocks > RM_FWD_MAX_BLOCKS ? RM_FWD_MAX_BLOCKS : blocks;
#define RM_FWD(MM)                                                                                                                  \
  hipLaunchKernelGGL((residual_mix_fwd_kernel<T, MM>), dim3(blocks), dim3(RM_THREADS), 0, s, (const T*)x, (const T*)ym, (const T*)yr, \
                     wc, bc, (T*)y, coef, P)
  switch (M) {
    case 64: RM_FWD(64); break;
    case 128: RM_FWD(128); break;
    case 256: RM_FWD(256); break;
    default: RM_FWD(512); break;
  }
#undef RM_FWD
  SWN_LAUNCH_CHECK();
  return 0;
}

template <typename T>
int bwd_launch(const void* dy, const void* x, const void* ym, const void* yr, const float* coef, const float* wc, int P, int M,
               void* d_moe, void* d_res, void* dx, float* partial, int blocks, hipStream_t s) {
#define RM_BWD(MM)                                                                                                                  \
  hipLaunchKernelGGL((residual_mix_bwd_kernel<T, MM>), dim3(blocks), dim3(RM_THREADS), 0, s, (const T*)dy, (const T*)x, (const T*)ym, \
                     (const T*)yr, coef, wc, (T*)d_moe, (T*)d_res, (T*)dx, partial, P)
  switch (M) {
    case 64: RM_BWD(64); break;
    case 128: RM_BWD(128); break;
    case 256: RM_BWD(256); break;
    default: RM_BWD(512); break;
  }
#undef RM_BWD
  SWN_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace swn

using namespace swn;

extern "C" int swn_residual_mix_fwd(const void* x, const void* y_moe, const void* y_res, const float* wc, const float* bc, int dtype,
                                    int n_tokens, int model_dim, void* y, float* coef, void* stream) {
  SWN_CHECK(dtype == SWN_F32 || dtype == SWN_HALF, "swn_residual_mix_fwd: bad dtype %d", dtype);
  SWN_CHECK(mix_dim_ok(model_dim), "swn_residual_mix_fwd: model_dim %d not in {64, 128, 256, 512}", model_dim);
  SWN_CHECK(n_tokens >= 0, "swn_residual_mix_fwd: bad token count %d", n_tokens);
  if (n_tokens == 0) return 0;
  SWN_CHECK(x && y_moe && y_res && wc && bc && y && coef, "swn_residual_mix_fwd: null pointer");
  SWN_CHECK(aligned16(x) && aligned16(y_moe) && aligned16(y_res) && aligned16(y) && aligned16(coef) && aligned16(wc),
            "swn_residual_mix_fwd: x, y_moe, y_res, y, coef and wc must be 16-byte aligned");
  const hipStream_t s = as_stream(stream);
  return dtype == SWN_F32 ? fwd_launch<float>(x, y_moe, y_res, wc, bc, n_tokens, model_dim, y, coef, s)
                          : fwd_launch<bf16_t>(x, y_moe, y_res, wc, bc, n_tokens, model_dim, y, coef, s);
}

extern "C" int swn_residual_mix_workspace_bytes(int dtype, int n_tokens, int model_dim, size_t* bytes) {
  SWN_CHECK(bytes, "swn_residual_mix_workspace_bytes: null pointer");
  SWN_CHECK(dtype == SWN_F32 || dtype == SWN_HALF, "swn_residual_mix_workspace_bytes: bad dtype %d", dtype);
  SWN_CHECK(mix_dim_ok(model_dim), "swn_residual_mix_workspace_bytes: model_dim %d not in {64, 128, 256, 512}", model_dim);
  SWN_CHECK(n_tokens >= 0, "swn_residual_mix_workspace_bytes: bad token count %d", n_tokens);
  *bytes = (size_t)bwd_blocks(dtype, n_tokens, model_dim) * (2 * model_dim + 2) * sizeof(float);
  return 0;
}

extern "C" int swn_residual_mix_bwd(const void* dy, const void* x, const void* y_moe, const void* y_res, const float* coef,
                                    const float* wc, int dtype, int n_tokens, int model_dim, void* d_moe, void* d_res, void* dx,
                                    float* d_wc, float* d_bc, void* workspace, size_t workspace_bytes, void* stream) {
  SWN_CHECK(dtype == SWN_F32 || dtype == SWN_HALF, "swn_residual_mix_bwd: bad dtype %d", dtype);
  SWN_CHECK(mix_dim_ok(model_dim), "swn_residual_mix_bwd: model_dim %d not in {64, 128, 256, 512}", model_dim);
  SWN_CHECK(n_tokens >= 0, "swn_residual_mix_bwd: bad token count %d", n_tokens);
  SWN_CHECK(d_wc && d_bc, "swn_residual_mix_bwd: null pointer");
  const hipStream_t s = as_stream(stream);
  if (n_tokens == 0) {      // no tokens: zero coefficient gradients, nothing else to write
    hipLaunchKernelGGL(fill_u32_kernel, dim3(1), dim3(256), 0, s, (uint32_t*)d_wc, 0u, (long)2 * model_dim);
    hipLaunchKernelGGL(fill_u32_kernel, dim3(1), dim3(256), 0, s, (uint32_t*)d_bc, 0u, 2L);
    SWN_LAUNCH_CHECK();
    return 0;
  }
  SWN_CHECK(dy && x && y_moe && y_res && coef && wc && d_moe && d_res && dx && workspace, "swn_residual_mix_bwd: null pointer");
  SWN_CHECK(aligned16(dy) && aligned16(x) && aligned16(y_moe) && aligned16(y_res) && aligned16(d_moe) && aligned16(d_res) &&
                aligned16(dx) && aligned16(coef) && aligned16(wc),
            "swn_residual_mix_bwd: row operands, coef and wc must be 16-byte aligned");
  const int blocks = bwd_blocks(dtype, n_tokens, model_dim);
  const int np = 2 * model_dim + 2;
  SWN_CHECK(workspace_bytes >= (size_t)blocks * np * sizeof(float), "swn_residual_mix_bwd: workspace too small (%zu < %zu bytes)",
            workspace_bytes, (size_t)blocks * np * sizeof(float));
  float* partial = (float*)workspace;
  const int rc = dtype == SWN_F32
                     ? bwd_launch<float>(dy, x, y_moe, y_res, coef, wc, n_tokens, model_dim, d_moe, d_res, dx, partial, blocks, s)
                     : bwd_launch<bf16_t>(dy, x, y_moe, y_res, coef, wc, n_tokens, model_dim, d_moe, d_res, dx, partial, blocks, s);
  if (rc) return rc;
  OrdDst d = {};
  d.p[0] = d_wc; d.n[0] = 2 * model_dim;
  d.p[1] = d_bc; d.n[1] = 2;
  ordered_reduce_async(partial, blocks, np, d, false, s);
  SWN_LAUNCH_CHECK();
  return 0;
}
