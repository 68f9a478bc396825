// Seeded device-side noise (philox.hpp): the fill kernel behind every supplied-noise argument of the library, and the step counter's
// advance.  The step is READ FROM DEVICE MEMORY by the kernels, so a launch captured into a hipGraph follows it from replay to replay.
//   swn_rng_fill     out[i] = draw of element base + i of (seed, *step_dev, stream_id): uniform [0,1) or normal * scale
//   swn_rng_fill_rows  the same generator addressed through a row index: out[j * per_row + s] = draw of element
//                    (row_base + row_index[j]) * per_row + s of (seed, *step_dev, stream_id, domain) - the draws of a data-dependent
//                    subset of the rays (the background model's), keyed by each ray's GLOBAL index
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

// Output row j holds the elements E0 .. E0 + per_row - 1, E0 = (row_base + row_index[j]) * per_row, i.e. a run of at most `bpr` Philox
// blocks from block E0 >> 2 on.  Slot t = j * bpr + k: one thread, one block (E0 >> 2) + k, computed once per output row; it stores
// the words of that block which lie inside the row.  The Box-Muller pairs are the block's word pairs, i.e. they follow the GLOBAL
// element's parity: a row that starts (ends) on an odd element takes only the sin (cos) half of the pair it shares with its neighbour.
// VEC (host-decided): per_row % 4 == 0 and out 16-byte aligned - every row is whole blocks (bpr = per_row / 4), one 16-byte store each.
template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void rng_fill_rows_kernel(float* __restrict__ out, long n_rows, long per_row, long bpr, long row_base,
                                                            const int64_t* __restrict__ row_index, float scale, uint64_t seed,
                                                            const int64_t* __restrict__ step_dev, int stream_id, int domain) {
  const uint32_t step = (uint32_t)*step_dev;
  const long slots = n_rows * bpr;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < slots; t += stride) {
    const long j = t / bpr, k = t - j * bpr;
    const long e0 = (row_base + (row_index ? row_index[j] : j)) * per_row;
    const long b = (e0 >> 2) + k;
    if (4 * b >= e0 + per_row) continue;             // (the row ends before its last slot: fewer than bpr blocks at this offset)
    const PhiloxWords v = philox_block(seed, step, stream_id, b, domain);
    float r[4];
    if constexpr (KIND == 0) {
#pragma unroll
      for (int w = 0; w < 4; ++w) r[w] = philox_uniform(v.w[w]);
    } else {
      philox_normal_pair(v.w[0], v.w[1], scale, r[0], r[1]);
      philox_normal_pair(v.w[2], v.w[3], scale, r[2], r[3]);
    }
    const long s0 = 4 * b - e0;                      // position of the block's first word in the row: in [-3, per_row - 1]
    float* row = out + j * per_row;
    if constexpr (VEC) {
      *(float4*)(row + s0) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const long s = s0 + w;
        if (s >= 0 && s < per_row) row[s] = r[w];
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

extern "C" int swn_rng_fill_rows(float* out, int64_t n_rows, int64_t per_row, int64_t row_base, const int64_t* row_index,
                                 int64_t index_limit, int kind, float scale, uint64_t seed, const int64_t* step_dev, int stream_id,
                                 int domain, void* stream) {
  SWN_CHECK(kind == 0 || kind == 1, "swn_rng_fill_rows: kind must be 0 (uniform) or 1 (normal), got %d", kind);
  SWN_CHECK(stream_id >= 0 && stream_id < RNG_STREAMS, "swn_rng_fill_rows: stream id %d outside 0..%d", stream_id, RNG_STREAMS - 1);
  SWN_CHECK(domain >= 0 && domain < RNG_DOMAINS, "swn_rng_fill_rows: domain %d outside 0..%d", domain, RNG_DOMAINS - 1);
  SWN_CHECK(n_rows >= 0 && per_row >= 0, "swn_rng_fill_rows: n_rows and per_row must be >= 0");
  SWN_CHECK(row_base >= 0, "swn_rng_fill_rows: row_base must be >= 0");
  SWN_CHECK(index_limit >= 0, "swn_rng_fill_rows: index_limit must be >= 0");
  // every index is < limit, so the last element of the last addressable row is (row_base + limit) * per_row - 1
  const int64_t limit = row_index ? index_limit : (index_limit > n_rows ? index_limit : n_rows);
  SWN_CHECK(row_base <= INT64_MAX - limit, "swn_rng_fill_rows: row_base + index_limit overflows");
  SWN_CHECK(per_row == 0 || (row_base + limit <= INT64_MAX / per_row && n_rows <= INT64_MAX / (per_row + 1)),
            "swn_rng_fill_rows: per_row %lld overflows the element index ((row_base + index_limit) * per_row)", (long long)per_row);
  if (n_rows == 0 || per_row == 0) return 0;
  SWN_CHECK(out, "swn_rng_fill_rows: out is NULL");
  SWN_CHECK(step_dev, "swn_rng_fill_rows: step_dev is NULL");
  SWN_CHECK(((uintptr_t)out & 3) == 0, "swn_rng_fill_rows: out must be 4-byte aligned");
  const bool vec = (per_row & 3) == 0 && ((uintptr_t)out & 15) == 0;
  const long bpr = vec ? per_row >> 2 : ((per_row + 2) >> 2) + 1;      // the most blocks a row spans (at element offset 3)
  long blocks = (n_rows * bpr + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  const dim3 grid((unsigned)blocks), block(256);
  hipStream_t s = as_stream(stream);
#define SWN_ROWS_LAUNCH(KIND, VEC)                                                                                                  \
  hipLaunchKernelGGL((rng_fill_rows_kernel<KIND, VEC>), grid, block, 0, s, out, (long)n_rows, (long)per_row, bpr, (long)row_base, \
                     row_index, scale, seed, step_dev, stream_id, domain)
  if (kind == 0) {
    if (vec) SWN_ROWS_LAUNCH(0, true);
    else SWN_ROWS_LAUNCH(0, false);
  } else {
    if (vec) SWN_ROWS_LAUNCH(1, true);
    else SWN_ROWS_LAUNCH(1, false);
  }
#undef SWN_ROWS_LAUNCH
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_rng_advance(int64_t* step_dev, void* stream) {
  SWN_CHECK(step_dev, "swn_rng_advance: null pointer");
  hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(1), 0, as_stream(stream), step_dev);
  SWN_LAUNCH_CHECK();
  return 0;
}
