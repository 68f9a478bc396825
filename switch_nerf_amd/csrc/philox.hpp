// Counter-based noise generator of the library: Philox4x32-10 (Salmon et al., "Parallel Random Numbers: As Easy as 1, 2, 3", SC'11),
// keyed by (seed, step, stream, GLOBAL element index) - the noise of a training step is a pure function of the problem, not of a device
// generator's history.  Header only; the integer part compiles for the host too (known-answer checks).
//
// Addressing: element e (int64, global) is word (e & 3) of block b = e >> 2;
//   counter = {b_lo, b_hi, step (u32), stream id | (domain << 8)}, key = {seed_lo, seed_hi}.
// Domains: 0 = the foreground model (and every consumer without a background model: the counter word is the bare stream id);
//   1 = the background model of a scene (background.BackgroundScene).  Its draws reuse the stream ids 0-3, and its rays - a
//   data-dependent subset of the batch - are addressed through their position in the batch: background row j is global ray
//   g = ray_base + idx_bg[j], so a background ray's noise depends on (seed, step, global ray) only, not on which other rays leave
//   the bound.  With Sb / Fb the background's coarse / fine sample counts:
//     stream 0 jitter      e = g * Sb + a   (a: the ASCENDING sample index, the order of swn_bg_sample_pe's perturb_rand)
//     stream 1 sigma noise e = g * Sb + j   (j: the row order the network evaluates = descending depth)
//     stream 2 fine u      e = g * Fb + f        stream 3 fine sigma noise  e = g * Fb + f
//   swn_rng_fill_rows (rng.hip) is the generator addressed through such a row index.
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
enum : int { RNG_DOMAIN_FG = 0, RNG_DOMAIN_BG = 1, RNG_DOMAINS = 2 };

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

// the four words of block `block` of (seed, step, stream, domain); domain 0 leaves the counter word the bare stream id
__host__ __device__ __forceinline__ PhiloxWords philox_block(uint64_t seed, uint32_t step, int stream_id, int64_t block, int domain = 0) {
  const uint64_t b = (uint64_t)block;
  return philox4x32_10((uint32_t)b, (uint32_t)(b >> 32), step, (uint32_t)stream_id | ((uint32_t)domain << 8), (uint32_t)seed,
                       (uint32_t)(seed >> 32));
}

__host__ __device__ __forceinline__ float philox_uniform(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-8f; }   // 2^-24

// the uniform draw of ONE element (a consumer kernel drawing in place: the jitter of sample_pe_kernel / bg_sample_pe_kernel)
__device__ __forceinline__ float philox_uniform_at(uint64_t seed, uint32_t step, int stream_id, int64_t e, int domain = 0) {
  const PhiloxWords v = philox_block(seed, step, stream_id, e >> 2, domain);
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
