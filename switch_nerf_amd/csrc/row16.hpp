// The 16-lane row layout of the row-streaming kernels (elementwise.hip, affine.hip).
#pragma once
#include "common.hpp"

namespace swn {

// One token row per 16-lane group (4 rows per wave): a lane owns COLS/16 features in 16-byte chunks
// (chunk c = j + 16 q  ->  a 16-lane group reads 256 contiguous bytes per instruction), and row reductions are four
// DPP adds inside the 16-lane row (quad_perm, quad_perm, row_half_mirror, row_mirror) - no LDS traffic.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float sum16(float v) {
  v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);  // row_half_mirror
  v += dpp_mov<0x140>(v);  // row_mirror
  return v;
}

template <typename T, int COLS> struct Row16 {
  static constexpr int VPL = COLS / 16;                          // values per lane
  static constexpr int EPC = 16 / (int)sizeof(T);                // elements per 16-byte chunk
  static constexpr int NCH = VPL / EPC;                          // chunks per lane
  static_assert(NCH >= 1, "row too narrow for the 16-lane layout");
  static __device__ __forceinline__ int col(int j, int v) { return (j + 16 * (v / EPC)) * EPC + (v % EPC); }
  static __device__ __forceinline__ void load(const T* row, int j, float* x) {
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
      const uint4 u = *(const uint4*)(row + (j + 16 * q) * EPC);
      if constexpr (sizeof(T) == 2) {
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          x[q * 8 + 2 * i] = bf16_to_f32((bf16_t)(w[i] & 0xFFFF));
          x[q * 8 + 2 * i + 1] = bf16_to_f32((bf16_t)(w[i] >> 16));
        }
      } else {
        x[q * 4 + 0] = __uint_as_float(u.x); x[q * 4 + 1] = __uint_as_float(u.y);
        x[q * 4 + 2] = __uint_as_float(u.z); x[q * 4 + 3] = __uint_as_float(u.w);
      }
    }
  }
  // the same in two halves, so that the next row's 16-byte loads can be in flight while this row is processed
  static __device__ __forceinline__ void load_raw(const T* row, int j, uint4* raw) {
#pragma unroll
    for (int q = 0; q < NCH; ++q) raw[q] = *(const uint4*)(row + (j + 16 * q) * EPC);
  }
  static __device__ __forceinline__ void unpack(const uint4* raw, float* x) {
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
      const uint4 u = raw[q];
      if constexpr (sizeof(T) == 2) {
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          x[q * 8 + 2 * i] = bf16_to_f32((bf16_t)(w[i] & 0xFFFF));
          x[q * 8 + 2 * i + 1] = bf16_to_f32((bf16_t)(w[i] >> 16));
        }
      } else {
        x[q * 4 + 0] = __uint_as_float(u.x); x[q * 4 + 1] = __uint_as_float(u.y);
        x[q * 4 + 2] = __uint_as_float(u.z); x[q * 4 + 3] = __uint_as_float(u.w);
      }
    }
  }
  static __device__ __forceinline__ void store(T* row, int j, const float* x) {
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
      uint4 u;
      if constexpr (sizeof(T) == 2) {
        u.x = pack_bf16x2(x[q * 8 + 0], x[q * 8 + 1]); u.y = pack_bf16x2(x[q * 8 + 2], x[q * 8 + 3]);
        u.z = pack_bf16x2(x[q * 8 + 4], x[q * 8 + 5]); u.w = pack_bf16x2(x[q * 8 + 6], x[q * 8 + 7]);
      } else {
        u.x = __float_as_uint(x[q * 4 + 0]); u.y = __float_as_uint(x[q * 4 + 1]);
        u.z = __float_as_uint(x[q * 4 + 2]); u.w = __float_as_uint(x[q * 4 + 3]);
      }
      *(uint4*)(row + (j + 16 * q) * EPC) = u;
    }
  }
  // fp32 parameter vector laid out like the row
  static __device__ __forceinline__ void loadf(const float* vec, int j, float* x) {
#pragma unroll
    for (int v = 0; v < VPL; ++v) x[v] = vec[col(j, v)];
  }
};

}  // namespace swn
