// The spatial-cell router of the Mega-NeRF model (mega.py; the reference's models/mega_nerf.py:19-61): a geometric, parameter-free,
// multi-membership gate around K dense NeRFs.
//   cells_assign_kernel    distances point -> centroid, membership and blend weights [P, K], members per cell
//   cells_count_kernel     members per (block of 256 points, cell)                            \
//   cells_scan_kernel      exclusive prefix of those over the blocks, begin[K + 1]             > swn_cells_pack
//   cells_place_kernel     slot[P, K] (row of a point inside a cell, or -1) and rows[total]   /
//   cells_gather_kernel    every cell's input rows (and sigma-noise rows) from rows[]
//   cells_pad_kernel, cells_gather_padded_kernel      the PADDED row space (swn_cells_pack_padded, swn_cells_gather_padded): every
//                          cell owns a fixed range of `capacity` rows, so nothing about a step's shapes depends on the batch
//   cells_gather_rng_kernel, cells_gather_padded_rng_kernel   the two gathers with the sigma noise DRAWN at the packed row (philox.hpp)
//                          instead of read from a [P] tensor: the seeded device noise of joint training (mega.py)
//   cells_blend_kernel     out[p] = sum over the member cells, ascending, of weights * sub-model output (a per-point gather: no atomics)
//   cells_blend_bwd_kernel d_sub[r] = weights * d_out[rows[r]]: the blend's adjoint, one packed row per thread (training, mega.py)
// Plain C++, fp32, fma contraction off: the distance is the direct sqrt(sum (x_j - c_j)^2) in the order j = dim_start .. 2 and the
// weights are mega_nerf.py:21-27 operation by operation, so a CPU restatement with the same operation order gives the same bits.
// Everything that decides an ORDER is an integer (counts, prefixes, ranks from wave ballots): the packing is a pure function of the
// input, rows ascend by point index inside a cell (the order x[cluster_mask] has in the reference).
#include "common.hpp"
#include "philox.hpp"

namespace swn {

constexpr int CELLS_MAX = 64;        // centroids in LDS; membership of a point as one 64-bit mask
constexpr int CELLS_BLOCK = 256;     // points per workgroup (4 waves)
constexpr int CELLS_WAVES = CELLS_BLOCK / 64;
constexpr int CELLS_SCAN_THREADS = 1024;

__device__ __forceinline__ float cell_dist(float x0, float x1, float x2, const float* __restrict__ c, int dim_start) {
#pragma clang fp contract(off)
  const float d1 = x1 - c[1], d2 = x2 - c[2];
  float s = d1 * d1 + d2 * d2;
  if (dim_start == 0) {
    const float d0 = x0 - c[0];
    s = (d0 * d0 + d1 * d1) + d2 * d2;
  }
  return sqrtf(s);
}

// Phase 1, one thread per point: the nearest distance (hard: its first index; soft: the threshold margin * d_min and the row sum of the
// kept inverse distances, summed in ascending cell order).  Phase 2, the block together: the [256, K] weight tile written in memory
// order (consecutive lanes, consecutive floats), each weight recomputed from the staged position - cheaper than a strided row store.
__global__ __launch_bounds__(CELLS_BLOCK) void cells_assign_kernel(const float* __restrict__ x, int stride, const float* __restrict__ centroids,
                                                                  int K, int dim_start, float margin, int hard, int P,
                                                                  float* __restrict__ weights, int32_t* __restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ float cen[CELLS_MAX * 3];
  __shared__ float xs[CELLS_BLOCK * 3];
  __shared__ float thr[CELLS_BLOCK];       // soft: margin * d_min
  __shared__ float rsum[CELLS_BLOCK];      // soft: row sum of the kept 1 / (d + 1e-8)
  __shared__ int amin[CELLS_BLOCK];        // hard: first index of the minimum
  __shared__ int cnt[CELLS_MAX];
  const int t = threadIdx.x;
  const long p0 = (long)blockIdx.x * CELLS_BLOCK;
  const long p = p0 + t;
  if (t < K * 3) cen[t] = centroids[t];
  if (t < CELLS_MAX) cnt[t] = 0;
  float x0 = 0.f, x1 = 0.f, x2 = 0.f;
  if (p < P) {
    const float* xp = x + p * stride;
    x0 = xp[0], x1 = xp[1], x2 = xp[2];
  }
  xs[t * 3 + 0] = x0, xs[t * 3 + 1] = x1, xs[t * 3 + 2] = x2;
  __syncthreads();
  float dmin = cell_dist(x0, x1, x2, cen, dim_start);
  int best = 0;
  for (int i = 1; i < K; ++i) {
    const float d = cell_dist(x0, x1, x2, cen + i * 3, dim_start);
    if (d < dmin) dmin = d, best = i;
  }
  const float th = margin * dmin;
  float sum = 0.f;
  if (!hard)
    for (int i = 0; i < K; ++i) {
      const float d = cell_dist(x0, x1, x2, cen + i * 3, dim_start);
      const float inv = d > th ? 0.f : 1.f / (d + 1e-8f);
      sum = sum + inv;
    }
  thr[t] = th, rsum[t] = sum, amin[t] = best;
  __syncthreads();
  const int n_here = (int)(P - p0 < CELLS_BLOCK ? P - p0 : CELLS_BLOCK);
  for (int e = t; e < n_here * K; e += CELLS_BLOCK) {
    const int pl = e / K, i = e - pl * K;
    float w;
    if (hard) {
      w = i == amin[pl] ? 1.f : 0.f;
    } else {
      const float d = cell_dist(xs[pl * 3], xs[pl * 3 + 1], xs[pl * 3 + 2], cen + i * 3, dim_start);
      const float inv = d > thr[pl] ? 0.f : 1.f / (d + 1e-8f);
      w = inv / rsum[pl];
    }
    weights[p0 * K + e] = w;
    if (w > 0.f) atomicAdd(&cnt[i], 1);      // (integer adds: the same counts in any order)
  }
  __syncthreads();
  if (t < K && cnt[t] != 0) atomicAdd(&counts[t], cnt[t]);
}

// The member mask of this thread's point (bit i = weights[p][i] > 0), and per cell the members of every wave of the block in
// wave_cnt[w][i]: one ballot per cell, uniform trip count (threads past P carry an empty mask).
__device__ __forceinline__ unsigned long long cells_wave_counts(const float* __restrict__ weights, int K, long p, int P,
                                                                int (*wave_cnt)[CELLS_MAX]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long mask = 0ull;
  if (p < P) {
    const float* wp = weights + p * K;
    for (int i = 0; i < K; ++i) mask |= wp[i] > 0.f ? 1ull << i : 0ull;
  }
  for (int i = 0; i < K; ++i) {
    const unsigned long long m = __ballot((mask >> i) & 1ull);
    if (lane == 0) wave_cnt[w][i] = __popcll(m);
  }
  __syncthreads();
  return mask;
}

__global__ __launch_bounds__(CELLS_BLOCK) void cells_count_kernel(const float* __restrict__ weights, int K, int P,
                                                                 int32_t* __restrict__ block_counts) {
  __shared__ int wave_cnt[CELLS_WAVES][CELLS_MAX];
  cells_wave_counts(weights, K, (long)blockIdx.x * CELLS_BLOCK + threadIdx.x, P, wave_cnt);
  const int t = threadIdx.x;
  if (t < K) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < CELLS_WAVES; ++w) s += wave_cnt[w][t];
    block_counts[(long)blockIdx.x * K + t] = s;
  }
}

// ONE workgroup: block_counts[n_blocks][K] -> in place, the members of the cell in the blocks before (exclusive prefix over the blocks).
// Thread = (run c of consecutive blocks, cell i): run sums, the runs before through LDS, then the running prefix inside the run.
// begin[0 .. K] = exclusive scan of counts; capacity > 0 (the padded row space): begin[k] = k * capacity whatever the counts.
__global__ __launch_bounds__(CELLS_SCAN_THREADS) void cells_scan_kernel(int32_t* __restrict__ block_counts, const int32_t* __restrict__ counts,
                                                                       int n_blocks, int K, int capacity, int32_t* __restrict__ begin) {
  __shared__ int part[CELLS_SCAN_THREADS];
  const int t = threadIdx.x;
  int n_runs = CELLS_SCAN_THREADS / K;
  n_runs = n_runs > 64 ? 64 : n_runs;
  const int c = t / K, i = t - c * K;
  const bool active = c < n_runs;
  const int per = (n_blocks + n_runs - 1) / n_runs;
  const int b0 = c * per, b1 = n_blocks < b0 + per ? n_blocks : b0 + per;
  int s = 0;
  if (active)
    for (int b = b0; b < b1; ++b) s += block_counts[(long)b * K + i];
  part[t] = s;
  __syncthreads();
  if (active) {
    int run = 0;
    for (int k = 0; k < c; ++k) run += part[k * K + i];
    for (int b = b0; b < b1; ++b) {
      const int v = block_counts[(long)b * K + i];
      block_counts[(long)b * K + i] = run;
      run += v;
    }
  }
  if (t == 0) {
    int run = 0;
    for (int k = 0; k < K; ++k) {
      begin[k] = run;
      run += capacity > 0 ? capacity : counts[k];
    }
    begin[K] = run;
  }
}

// capacity > 0 (the padded row space): a member whose rank inside its cell is capacity or more does not fit - no row, slot -1.
__global__ __launch_bounds__(CELLS_BLOCK) void cells_place_kernel(const float* __restrict__ weights, const int32_t* __restrict__ block_base,
                                                                 const int32_t* __restrict__ begin, int K, int P, long rows_capacity,
                                                                 int capacity, int32_t* __restrict__ rows, int32_t* __restrict__ slot) {
  __shared__ int wave_cnt[CELLS_WAVES][CELLS_MAX];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long p = (long)blockIdx.x * CELLS_BLOCK + threadIdx.x;
  const unsigned long long mask = cells_wave_counts(weights, K, p, P, wave_cnt);
  for (int i = 0; i < K; ++i) {
    const bool member = (mask >> i) & 1ull;
    const unsigned long long m = __ballot(member);
    if (p >= P) continue;
    int s = -1;
    if (member) {
      s = block_base[(long)blockIdx.x * K + i] + __popcll(m & ((1ull << lane) - 1ull));
      for (int k = 0; k < w; ++k) s += wave_cnt[k][i];
      if (capacity > 0 && s >= capacity) {
        s = -1;
      } else {
        const long r = (long)begin[i] + s;
        if (r >= 0 && r < rows_capacity) rows[r] = (int32_t)p;
      }
    }
    slot[p * K + i] = s;
  }
}

// one thread per element of the packed input [total, width]: consecutive lanes write consecutive floats
__global__ __launch_bounds__(256) void cells_gather_kernel(const float* __restrict__ x, int stride, int col0, const int32_t* __restrict__ rows,
                                                          long total, int P, const float* __restrict__ noise, float* __restrict__ x_out,
                                                          float* __restrict__ noise_out) {
  const int width = stride - col0;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total * width) return;
  const long r = e / width;
  const int c = (int)(e - r * width);
  const int p = rows[r];
  const bool ok = p >= 0 && p < P;            // (never false for a row list of swn_cells_pack)
  x_out[e] = ok ? x[(long)p * stride + col0 + c] : 0.f;
  if (c == 0 && noise) noise_out[r] = ok ? noise[p] : 0.f;
}

// The padded row space behind cells_place_kernel: row j of cell i's range is a padding row (-1) from j = counts[i] on - the place
// kernel wrote the min(counts[i], capacity) rows in front, so every one of the n_cells * capacity rows is written exactly once.
// overflow = the memberships that did not fit, summed over the cells in ascending order by one thread (no atomics).
__global__ __launch_bounds__(256) void cells_pad_kernel(const int32_t* __restrict__ counts, int K, int capacity, int32_t* __restrict__ rows,
                                                       int32_t* __restrict__ overflow) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0) {
    int over = 0;
    for (int i = 0; i < K; ++i) over += counts[i] > capacity ? counts[i] - capacity : 0;
    *overflow = over;
  }
  if (r >= (long)K * capacity) return;
  const int i = (int)(r / capacity);
  if (r - (long)i * capacity >= counts[i]) rows[r] = -1;
}

// cells_gather_kernel over the padded row space, rows of (position, direction, image index): a padding row (rows[r] < 0) reads
// nothing of x and becomes a point the cell's network can run on - its own centroid seen along (0, 0, 1) in image 0, sigma noise 0.
__global__ __launch_bounds__(256) void cells_gather_padded_kernel(const float* __restrict__ x, int stride, int col0,
                                                                 const int32_t* __restrict__ rows, const float* __restrict__ centroids,
                                                                 int K, int capacity, int P, const float* __restrict__ noise,
                                                                 float* __restrict__ x_out, float* __restrict__ noise_out) {
  constexpr int width = 7;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)K * capacity * width) return;
  const long r = e / width;
  const int c = (int)(e - r * width);
  const int p = rows[r];
  const bool real = p >= 0 && p < P;
  float v;
  if (real)
    v = x[(long)p * stride + col0 + c];
  else
    v = c < 3 ? centroids[(r / capacity) * 3 + c] : (c == 5 ? 1.f : 0.f);
  x_out[e] = v;
  if (c == 0 && noise) noise_out[r] = real ? noise[p] : 0.f;
}

// The sigma noise of a packed row, drawn where it is consumed: the row holds point p = rows[r], global element e = elem_base + p of
// (seed, step, stream_id), domain 0 - the bits swn_rng_fill (kind = normal) writes for element e.  The Box-Muller pair is the word
// pair (0,1) or (2,3) of block e >> 2 and the half follows the parity of the GLOBAL element e (as in rng_fill_rows_kernel), so an odd
// rows-per-ray or an odd ray base makes neighbouring points share a pair exactly as the fill does.  A point that sits in several cells
// (soft margin) draws the same element in each: the reference's sigma_noise[cluster_mask].
__device__ __forceinline__ float cells_row_normal(uint64_t seed, uint32_t step, int stream_id, long e, float scale) {
  const PhiloxWords v = philox_block(seed, step, stream_id, e >> 2);
  const bool hi = (e & 2) != 0;
  float n_even, n_odd;
  philox_normal_pair(hi ? v.w[2] : v.w[0], hi ? v.w[3] : v.w[1], scale, n_even, n_odd);
  return (e & 1) ? n_odd : n_even;
}

// cells_gather_kernel with the noise drawn.  The copy keeps its layout (one thread per element of x_out, the same bytes); the draw has
// its own: thread t < total draws row t, so the Philox rounds and the logf / sincosf run in full waves at the front of the grid and
// not in the one lane in `width` that holds a row's first column.  No [P] noise tensor exists; a row with rows[r] outside [0, P) gets +0.
__global__ __launch_bounds__(256) void cells_gather_rng_kernel(const float* __restrict__ x, int stride, int col0, const int32_t* __restrict__ rows,
                                                              long total, int P, uint64_t seed, const int64_t* __restrict__ step_dev,
                                                              int stream_id, long elem_base, float scale, float* __restrict__ x_out,
                                                              float* __restrict__ noise_out) {
  const int width = stride - col0;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total * width) return;
  const long r = e / width;
  const int c = (int)(e - r * width);
  const int p = rows[r];
  const bool ok = p >= 0 && p < P;
  x_out[e] = ok ? x[(long)p * stride + col0 + c] : 0.f;
  if (e < total) {
    const int q = rows[e];
    noise_out[e] = q >= 0 && q < P ? cells_row_normal(seed, (uint32_t)*step_dev, stream_id, elem_base + q, scale) : 0.f;
  }
}

// cells_gather_padded_kernel with the noise drawn (cells_gather_rng_kernel's layout): a padding row gets exactly +0.
__global__ __launch_bounds__(256) void cells_gather_padded_rng_kernel(const float* __restrict__ x, int stride, int col0,
                                                                     const int32_t* __restrict__ rows, const float* __restrict__ centroids,
                                                                     int K, int capacity, int P, uint64_t seed,
                                                                     const int64_t* __restrict__ step_dev, int stream_id, long elem_base,
                                                                     float scale, float* __restrict__ x_out, float* __restrict__ noise_out) {
  constexpr int width = 7;
  const long total = (long)K * capacity;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total * width) return;
  const long r = e / width;
  const int c = (int)(e - r * width);
  const int p = rows[r];
  const bool real = p >= 0 && p < P;
  float v;
  if (real)
    v = x[(long)p * stride + col0 + c];
  else
    v = c < 3 ? centroids[(r / capacity) * 3 + c] : (c == 5 ? 1.f : 0.f);
  x_out[e] = v;
  if (e < total) {
    const int q = rows[e];
    noise_out[e] = q >= 0 && q < P ? cells_row_normal(seed, (uint32_t)*step_dev, stream_id, elem_base + q, scale) : 0.f;
  }
}

template <int C>
__global__ __launch_bounds__(256) void cells_blend_kernel(const float* __restrict__ weights, const int32_t* __restrict__ slot,
                                                         const int32_t* __restrict__ begin, const float* __restrict__ sub_out, long total,
                                                         int K, int hard, int P, float* __restrict__ out) {
#pragma clang fp contract(off)
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  for (int i = 0; i < K; ++i) {
    const int s = slot[p * K + i];
    if (s < 0) continue;
    const long r = (long)begin[i] + s;
    if (r >= total) continue;                 // (never for a slot list of swn_cells_pack / _pack_padded)
    float v[C];
    if constexpr (C == 4) {
      const float4 q = *reinterpret_cast<const float4*>(sub_out + r * 4);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[C - 1] = q.w;
    } else {
      v[0] = sub_out[r];
    }
    if (hard) {                               // results[cluster_mask] = sub_result (mega_nerf.py:47)
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = v[c];
    } else {                                  // results[cluster_mask] += sub_result * weights[cluster_mask, i] (:49)
      const float wt = weights[p * K + i];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float prod = v[c] * wt;
        acc[c] = acc[c] + prod;
      }
    }
  }
  if constexpr (C == 4)
    *reinterpret_cast<float4*>(out + p * 4) = make_float4(acc[0], acc[1], acc[2], acc[C - 1]);
  else
    out[p] = acc[0];
}

// The adjoint of cells_blend_kernel with respect to sub_out: packed row r of cell i(r) belongs to point rows[r] and entered its output
// with the factor weights[rows[r]][i(r)] (hard: 1), so that is what its gradient is.  One thread per packed row, every row written
// once: no atomics, no zero fill.  i(r) is the cell with begin[i] <= r < begin[i + 1], found by bisection in the LDS copy of begin[]
// (empty cells have begin[i] == begin[i + 1] and are never the answer); the hard form needs no weight and skips both.
template <int C>
__global__ __launch_bounds__(256) void cells_blend_bwd_kernel(const float* __restrict__ weights, const int32_t* __restrict__ rows,
                                                             const int32_t* __restrict__ begin, const float* __restrict__ d_out, long total,
                                                             int K, int hard, int P, float* __restrict__ d_sub) {
#pragma clang fp contract(off)
  __shared__ int sb[CELLS_MAX + 1];
  if (!hard) {
    if (threadIdx.x <= K) sb[threadIdx.x] = begin[threadIdx.x];
    __syncthreads();
  }
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total) return;
  const int p = rows[r];
  const bool ok = p >= 0 && p < P;            // (false for the padding rows of swn_cells_pack_padded only: they get +0)
  float wt = 1.f;
  if (!hard && ok) {
    int lo = 0, hi = K - 1;                   // the first cell whose end lies past r
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((long)sb[mid + 1] > r) hi = mid; else lo = mid + 1;
    }
    wt = weights[(long)p * K + lo];
  }
  if constexpr (C == 4) {
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) q = *reinterpret_cast<const float4*>(d_out + (long)p * 4);
    if (!hard) q.x = q.x * wt, q.y = q.y * wt, q.z = q.z * wt, q.w = q.w * wt;
    *reinterpret_cast<float4*>(d_sub + r * 4) = q;
  } else {
    float v = ok ? d_out[p] : 0.f;
    if (!hard) v = v * wt;
    d_sub[r] = v;
  }
}

}  // namespace swn

using namespace swn;

extern "C" int swn_cells_assign(const float* x, int stride, const float* centroids, int n_cells, int dim_start, float margin,
                                int n_points, float* weights, int32_t* counts, void* stream) {
  SWN_CHECK(n_cells >= 1 && n_cells <= CELLS_MAX, "swn_cells_assign: n_cells %d outside [1, %d]", n_cells, CELLS_MAX);
  SWN_CHECK(x && centroids && weights && counts, "swn_cells_assign: null pointer");
  SWN_CHECK(n_points >= 1 && stride >= 3, "swn_cells_assign: bad sizes (n_points %d, stride %d)", n_points, stride);
  SWN_CHECK(dim_start == 0 || dim_start == 1, "swn_cells_assign: dim_start %d is neither 0 nor 1", dim_start);
  SWN_CHECK(margin >= 1.f, "swn_cells_assign: margin %g < 1", (double)margin);
  const hipError_t e = fill_u32_async(counts, 0u, (size_t)n_cells * 4, as_stream(stream));
  SWN_CHECK(e == hipSuccess, "swn_cells_assign: fill failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(cells_assign_kernel, dim3(cdiv(n_points, CELLS_BLOCK)), dim3(CELLS_BLOCK), 0, as_stream(stream), x, stride,
                     centroids, n_cells, dim_start, margin, margin == 1.f ? 1 : 0, n_points, weights, counts);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_cells_pack_workspace_bytes(int n_points, int n_cells, size_t* bytes) {
  SWN_CHECK(bytes, "swn_cells_pack_workspace_bytes: null pointer");
  SWN_CHECK(n_cells >= 1 && n_cells <= CELLS_MAX, "swn_cells_pack_workspace_bytes: n_cells %d outside [1, %d]", n_cells, CELLS_MAX);
  SWN_CHECK(n_points >= 1, "swn_cells_pack_workspace_bytes: n_points %d < 1", n_points);
  *bytes = (size_t)cdiv(n_points, CELLS_BLOCK) * n_cells * sizeof(int32_t);
  return 0;
}

extern "C" int swn_cells_pack(const float* weights, const int32_t* counts, int n_points, int n_cells, int32_t* begin, int32_t* rows,
                              long rows_capacity, int32_t* slot, void* workspace, size_t workspace_bytes, void* stream) {
  SWN_CHECK(n_cells >= 1 && n_cells <= CELLS_MAX, "swn_cells_pack: n_cells %d outside [1, %d]", n_cells, CELLS_MAX);
  SWN_CHECK(weights && counts && begin && rows && slot && workspace, "swn_cells_pack: null pointer");
  SWN_CHECK(n_points >= 1 && rows_capacity >= 1, "swn_cells_pack: bad sizes (n_points %d, rows_capacity %ld)", n_points, rows_capacity);
  const int n_blocks = cdiv(n_points, CELLS_BLOCK);
  SWN_CHECK(workspace_bytes >= (size_t)n_blocks * n_cells * sizeof(int32_t), "swn_cells_pack: workspace of %zu bytes, %zu needed",
            workspace_bytes, (size_t)n_blocks * n_cells * sizeof(int32_t));
  int32_t* block_counts = (int32_t*)workspace;
  hipLaunchKernelGGL(cells_count_kernel, dim3(n_blocks), dim3(CELLS_BLOCK), 0, as_stream(stream), weights, n_cells, n_points, block_counts);
  hipLaunchKernelGGL(cells_scan_kernel, dim3(1), dim3(CELLS_SCAN_THREADS), 0, as_stream(stream), block_counts, counts, n_blocks, n_cells,
                     0, begin);
  hipLaunchKernelGGL(cells_place_kernel, dim3(n_blocks), dim3(CELLS_BLOCK), 0, as_stream(stream), weights, block_counts, begin, n_cells,
                     n_points, rows_capacity, 0, rows, slot);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_cells_pack_padded(const float* weights, const int32_t* counts, int n_points, int n_cells, int capacity, int32_t* begin,
                                     int32_t* rows, int32_t* slot, int32_t* overflow, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  SWN_CHECK(n_cells >= 1 && n_cells <= CELLS_MAX, "swn_cells_pack_padded: n_cells %d outside [1, %d]", n_cells, CELLS_MAX);
  SWN_CHECK(weights && counts && begin && rows && slot && overflow && workspace, "swn_cells_pack_padded: null pointer");
  SWN_CHECK(n_points >= 1 && capacity >= 1, "swn_cells_pack_padded: bad sizes (n_points %d, capacity %d)", n_points, capacity);
  const long total = (long)n_cells * capacity;
  SWN_CHECK(total <= 2147483647l, "swn_cells_pack_padded: %d cells of %d rows exceed the 32-bit row space", n_cells, capacity);
  const int n_blocks = cdiv(n_points, CELLS_BLOCK);
  SWN_CHECK(workspace_bytes >= (size_t)n_blocks * n_cells * sizeof(int32_t), "swn_cells_pack_padded: workspace of %zu bytes, %zu needed",
            workspace_bytes, (size_t)n_blocks * n_cells * sizeof(int32_t));
  int32_t* block_counts = (int32_t*)workspace;
  hipLaunchKernelGGL(cells_count_kernel, dim3(n_blocks), dim3(CELLS_BLOCK), 0, as_stream(stream), weights, n_cells, n_points, block_counts);
  hipLaunchKernelGGL(cells_scan_kernel, dim3(1), dim3(CELLS_SCAN_THREADS), 0, as_stream(stream), block_counts, counts, n_blocks, n_cells,
                     capacity, begin);
  hipLaunchKernelGGL(cells_place_kernel, dim3(n_blocks), dim3(CELLS_BLOCK), 0, as_stream(stream), weights, block_counts, begin, n_cells,
                     n_points, total, capacity, rows, slot);
  hipLaunchKernelGGL(cells_pad_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), counts, n_cells, capacity, rows, overflow);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_cells_gather(const float* x, int stride, int col0, const int32_t* rows, long total, int n_points,
                                const float* sigma_noise, float* x_out, float* noise_out, void* stream) {
  SWN_CHECK(x && rows && x_out, "swn_cells_gather: null pointer");
  SWN_CHECK((sigma_noise == nullptr) == (noise_out == nullptr), "swn_cells_gather: sigma_noise and noise_out come together");
  SWN_CHECK(n_points >= 1 && total >= 0 && col0 >= 0 && col0 < stride, "swn_cells_gather: bad sizes (n_points %d, total %ld, columns [%d, %d))",
            n_points, total, col0, stride);
  if (total == 0) return 0;
  const long n = total * (stride - col0);
  SWN_CHECK(n <= 2147483647l * 256, "swn_cells_gather: %ld elements exceed the grid", n);      // (cdiv returns an int)
  hipLaunchKernelGGL(cells_gather_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), x, stride, col0, rows, total, n_points,
                     sigma_noise, x_out, noise_out);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_cells_gather_padded(const float* x, int stride, int col0, const int32_t* rows, const float* centroids, int n_cells,
                                       int capacity, int n_points, const float* sigma_noise, float* x_out, float* noise_out, void* stream) {
  SWN_CHECK(n_cells >= 1 && n_cells <= CELLS_MAX, "swn_cells_gather_padded: n_cells %d outside [1, %d]", n_cells, CELLS_MAX);
  SWN_CHECK(x && rows && centroids && x_out, "swn_cells_gather_padded: null pointer");
  SWN_CHECK((sigma_noise == nullptr) == (noise_out == nullptr), "swn_cells_gather_padded: sigma_noise and noise_out come together");
  SWN_CHECK(n_points >= 1 && capacity >= 1 && col0 >= 0, "swn_cells_gather_padded: bad sizes (n_points %d, capacity %d, col0 %d)", n_points,
            capacity, col0);
  SWN_CHECK(stride - col0 == 7, "swn_cells_gather_padded: columns [%d, %d) are not the 7 of (position, direction, image index)", col0, stride);
  const long n = (long)n_cells * capacity * 7;
  SWN_CHECK((long)n_cells * capacity <= 2147483647l, "swn_cells_gather_padded: %d cells of %d rows exceed the 32-bit row space", n_cells,
            capacity);
  hipLaunchKernelGGL(cells_gather_padded_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), x, stride, col0, rows, centroids,
                     n_cells, capacity, n_points, sigma_noise, x_out, noise_out);
  SWN_LAUNCH_CHECK();
  return 0;
}

// what both _rng gathers check of the draw before anything is launched; the element index ray_base * rows_per_ray + point must fit
static int cells_rng_check(const char* name, const int64_t* step_dev, const float* noise_out, int stream_id, int rows_per_ray,
                           int64_t ray_base, float scale, int n_points) {
  SWN_CHECK(step_dev && noise_out, "%s: null pointer", name);
  SWN_CHECK(scale > 0.f, "%s: scale %g is not > 0 (no sigma noise: that is the plain gather)", name, (double)scale);
  SWN_CHECK(stream_id == RNG_STREAM_SIGMA || stream_id == RNG_STREAM_SIGMA_FINE,
            "%s: stream id %d is neither %d (coarse sigma noise) nor %d (fine sigma noise)", name, stream_id, (int)RNG_STREAM_SIGMA,
            (int)RNG_STREAM_SIGMA_FINE);
  SWN_CHECK(rows_per_ray > 0, "%s: rows_per_ray %d is not > 0", name, rows_per_ray);
  SWN_CHECK(ray_base >= 0 && ray_base <= (INT64_MAX - (int64_t)n_points) / rows_per_ray,
            "%s: ray_base %lld is negative or overflows the element index (ray_base * rows_per_ray + point)", name, (long long)ray_base);
  return 0;
}

extern "C" int swn_cells_gather_rng(const float* x, int stride, int col0, const int32_t* rows, long total, int n_points, uint64_t seed,
                                    const int64_t* step_dev, int stream_id, int rows_per_ray, int64_t ray_base, float scale, float* x_out,
                                    float* noise_out, void* stream) {
  SWN_CHECK(x && rows && x_out, "swn_cells_gather_rng: null pointer");
  SWN_CHECK(n_points >= 1 && total >= 0 && col0 >= 0 && col0 < stride, "swn_cells_gather_rng: bad sizes (n_points %d, total %ld, columns [%d, %d))",
            n_points, total, col0, stride);
  if (cells_rng_check("swn_cells_gather_rng", step_dev, noise_out, stream_id, rows_per_ray, ray_base, scale, n_points)) return -1;
  if (total == 0) return 0;
  const long n = total * (stride - col0);
  SWN_CHECK(n <= 2147483647l * 256, "swn_cells_gather_rng: %ld elements exceed the grid", n);      // (cdiv returns an int)
  hipLaunchKernelGGL(cells_gather_rng_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), x, stride, col0, rows, total, n_points,
                     seed, step_dev, stream_id, (long)(ray_base * rows_per_ray), scale, x_out, noise_out);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_cells_gather_padded_rng(const float* x, int stride, int col0, const int32_t* rows, const float* centroids, int n_cells,
                                           int capacity, int n_points, uint64_t seed, const int64_t* step_dev, int stream_id,
                                           int rows_per_ray, int64_t ray_base, float scale, float* x_out, float* noise_out, void* stream) {
  SWN_CHECK(n_cells >= 1 && n_cells <= CELLS_MAX, "swn_cells_gather_padded_rng: n_cells %d outside [1, %d]", n_cells, CELLS_MAX);
  SWN_CHECK(x && rows && centroids && x_out, "swn_cells_gather_padded_rng: null pointer");
  SWN_CHECK(n_points >= 1 && capacity >= 1 && col0 >= 0, "swn_cells_gather_padded_rng: bad sizes (n_points %d, capacity %d, col0 %d)",
            n_points, capacity, col0);
  SWN_CHECK(stride - col0 == 7, "swn_cells_gather_padded_rng: columns [%d, %d) are not the 7 of (position, direction, image index)", col0,
            stride);
  if (cells_rng_check("swn_cells_gather_padded_rng", step_dev, noise_out, stream_id, rows_per_ray, ray_base, scale, n_points)) return -1;
  const long n = (long)n_cells * capacity * 7;
  SWN_CHECK((long)n_cells * capacity <= 2147483647l, "swn_cells_gather_padded_rng: %d cells of %d rows exceed the 32-bit row space", n_cells,
            capacity);
  hipLaunchKernelGGL(cells_gather_padded_rng_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), x, stride, col0, rows, centroids,
                     n_cells, capacity, n_points, seed, step_dev, stream_id, (long)(ray_base * rows_per_ray), scale, x_out, noise_out);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_cells_blend(const float* weights, const int32_t* slot, const int32_t* begin, const float* sub_out, long total,
                               int n_points, int n_cells, int channels, int hard, float* out, void* stream) {
  SWN_CHECK(n_cells >= 1 && n_cells <= CELLS_MAX, "swn_cells_blend: n_cells %d outside [1, %d]", n_cells, CELLS_MAX);
  SWN_CHECK(weights && slot && begin && sub_out && out, "swn_cells_blend: null pointer");
  SWN_CHECK(channels == 1 || channels == 4, "swn_cells_blend: channels %d is neither 1 nor 4", channels);
  SWN_CHECK(n_points >= 1 && total >= 1, "swn_cells_blend: bad sizes (n_points %d, total %ld)", n_points, total);
  SWN_CHECK(channels == 1 || ((((uintptr_t)sub_out) | ((uintptr_t)out)) & 15) == 0, "swn_cells_blend: sub_out / out must be 16-byte aligned");
  if (channels == 4)
    hipLaunchKernelGGL(cells_blend_kernel<4>, dim3(cdiv(n_points, 256)), dim3(256), 0, as_stream(stream), weights, slot, begin, sub_out,
                       total, n_cells, hard, n_points, out);
  else
    hipLaunchKernelGGL(cells_blend_kernel<1>, dim3(cdiv(n_points, 256)), dim3(256), 0, as_stream(stream), weights, slot, begin, sub_out,
                       total, n_cells, hard, n_points, out);
  SWN_LAUNCH_CHECK();
  return 0;
}

extern "C" int swn_cells_blend_bwd(const float* weights, const int32_t* rows, const int32_t* begin, const float* d_out, long total,
                                   int n_points, int n_cells, int channels, int hard, float* d_sub, void* stream) {
  SWN_CHECK(n_cells >= 1 && n_cells <= CELLS_MAX, "swn_cells_blend_bwd: n_cells %d outside [1, %d]", n_cells, CELLS_MAX);
  SWN_CHECK(channels == 1 || channels == 4, "swn_cells_blend_bwd: channels %d is neither 1 nor 4", channels);
  SWN_CHECK(n_points >= 1 && total >= 0, "swn_cells_blend_bwd: bad sizes (n_points %d, total %ld)", n_points, total);
  if (total == 0) return 0;
  SWN_CHECK(rows && d_out && d_sub && (hard || (weights && begin)), "swn_cells_blend_bwd: null pointer");
  SWN_CHECK(channels == 1 || ((((uintptr_t)d_out) | ((uintptr_t)d_sub)) & 15) == 0, "swn_cells_blend_bwd: d_out / d_sub must be 16-byte aligned");
  SWN_CHECK(total <= 2147483647l * 256, "swn_cells_blend_bwd: %ld rows exceed the grid", total);      // (cdiv returns an int)
  if (channels == 4)
    hipLaunchKernelGGL(cells_blend_bwd_kernel<4>, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), weights, rows, begin, d_out,
                       total, n_cells, hard, n_points, d_sub);
  else
    hipLaunchKernelGGL(cells_blend_bwd_kernel<1>, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), weights, rows, begin, d_out,
                       total, n_cells, hard, n_points, d_sub);
  SWN_LAUNCH_CHECK();
  return 0;
}
