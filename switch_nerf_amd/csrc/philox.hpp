// Counter-based noise generator of the library: Philox4x32-10 (Salmon et al., "Parallel Random Numbers: As Easy as 1, 2, 3", SC'11),
// keyed by (seed, step, stream, GLOBAL element index) - the noise of a training step is a pure function of the problem, not of a device
// generator's history.  Header only; the integer part compiles for the host too (known-answer checks).
//
// Addressing: element e (int64, global) is word (e & 3) of block b = e >> 2;
//   counter = {b_lo, b_hi, step (u32), stream id}, key = {seed_lo, seed_hi}.
// Uniform: u = (x >> 8) * 2^-24 in [0, 1) (torch.rand's range).
// Normal (Box-Muller over the word pairs (0,1) and (2,3)): u1 = ((x_a >> 8) + 1) * 2^-24 in (0, 1] (never inf),
//   r = sqrtf(-2 logf(u1)), theta = 2 pi (x_b >> 8) 2^-24; the even word gets r cos(theta), the odd word r sin(theta).
//   logf / sincosf are the accurate ones: tests/philox_restate.py restates this in float64 within a derived bound.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace swn {

// stream ids (fixed; ops.py carries the same table)
enum : int {
  RNG_STREAM_JITTER = 0,        // coarse stratified jitter          e = (ray_base + n) * S + s
  RNG_STREAM_SIGMA = 1,         // coarse sigma noise                e = (ray_base + n) * R + r   (R rows per ray)
  RNG_STREAM_FINE_U = 2,        // fine-pass u                       e = (ray_base + n) * F + f
  RNG_STREAM_SIGMA_FINE = 3,    // fine sigma noise                  as stream 1 with the fine row count
  RNG_STREAM_GATE = 4,          // gate noise                        e = (ray_base * R + p) * E + expert
  RNG_STREAM_ROUTER_NORMAL = 5, // moe.MoELayer's use_normal_noise draw, addressed like stream 4
  RNG_STREAMS = 6
};

struct PhiloxWords { uint32_t w[4]; };

__host__ __device__ __forceinline__ void philox_mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
  const uint64_t p = (uint64_t)a * (uint64_t)b;
  hi = (uint32_t)(p >> 32);
  lo = (uint32_t)p;
}

__host__ __device__ __forceinline__ PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                              uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0, lo0, hi1, lo1;
    philox_mulhilo(0xD2511F53u, c0, hi0, lo0);
    philox_mulhilo(0xCD9E8D57u, c2, hi1, lo1);
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return PhiloxWords{{c0, c1, c2, c3}};
}

// the four words of block `block` of (seed, step, stream)
__host__ __device__ __forceinline__ PhiloxWords philox_block(uint64_t seed, uint32_t step, int stream_id, int64_t block) {
  const uint64_t b = (uint64_t)block;
  return philox4x32_10((uint32_t)b, (uint32_t)(b >> 32), step, (uint32_t)stream_id, (uint32_t)seed, (uint32_t)(seed >> 32));
}

__host__ __device__ __forceinline__ float philox_uniform(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-8f; }   // 2^-24

// the uniform draw of ONE element (a consumer kernel drawing in place: sample_pe_kernel's jitter)
__device__ __forceinline__ float philox_uniform_at(uint64_t seed, uint32_t step, int stream_id, int64_t e) {
  const PhiloxWords v = philox_block(seed, step, stream_id, e >> 2);
  return philox_uniform(v.w[e & 3]);
}

// Box-Muller over one word pair: n_even = r cos(theta), n_odd = r sin(theta), both times `scale`
__device__ __forceinline__ void philox_normal_pair(uint32_t xa, uint32_t xb, float scale, float& n_even, float& n_odd) {
#pragma clang fp contract(off)
  const float u1 = (float)((xa >> 8) + 1u) * 5.9604644775390625e-8f;
  const float r = sqrtf(-2.f * logf(u1));
  const float theta = 6.283185307179586f * ((float)(xb >> 8) * 5.9604644775390625e-8f);
  float sn, cs;
  sincosf(theta, &sn, &cs);
  n_even = (r * cs) * scale;
  n_odd = (r * sn) * scale;
}

}  // namespace swn
