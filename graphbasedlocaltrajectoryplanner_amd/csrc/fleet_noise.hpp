// fleet_noise.hpp -- the random source of the fleet's closed-loop simulation (ltpl_fleet_sim_noise, include/ltpl_hip.h): a counter-based
// generator and one noise sample built from it. Plain functions, host- and device-compilable, no HIP types: tests/sim_noise_shim.cpp
// compiles this file alone with the host compiler; the host mirror is sim.philox4x32 / sim.noise_gauss.
//
//   philox4x32_10   Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers
//                   0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds
//   noise_gauss     g(seed, tick, obj, comp): key = (seed low word, seed high word); three blocks with the counters
//                   (tick, obj, 3 comp + b, 0), b = 0, 1, 2; K = the sum of their 12 output words as uint64 (< 2^36);
//                   g = ((double)K + 6.0) 2^-32 - 6.0 -- the sum of twelve uniforms ((w + 0.5) 2^-32) minus six: mean 0, variance
//                   1 - 2^-64, |g| < 6. The conversion, the sum (an integer < 2^37), the product with a power of two and the
//                   difference (a multiple of 2^-32 below 6) are all exact in fp64: no libm call, no fma, no tolerance
//   noise_add       v + sigma g (one multiply, one add; built with -ffp-contract=off on both sides); sigma == 0 draws nothing and
//                   hands v through untouched
//
// obj:  0xFFFFFFFF the ego estimate | k: entry k of the planner's own object list (opponents first, then statics; the index BEFORE the
//       on-track compaction) | 0x80000000 | (q - mate_lo): mate q of the planner's race
// comp: ego 0 x, 1 y, 2 v; object 0 x, 1 y, 2 theta, 3 v
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define FLEET_NOISE_FN __host__ __device__ inline
#else
#define FLEET_NOISE_FN inline
#endif

namespace fleet {

static constexpr uint32_t kNoiseEgo = 0xFFFFFFFFu;
static constexpr uint32_t kNoiseMate = 0x80000000u;

FLEET_NOISE_FN void philox4x32_10(const uint32_t ctr[4], uint32_t k0, uint32_t k1, uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;      // (high word: one v_mul_hi_u32 each)
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// `words` (may be null): the 12 output words, block by block
FLEET_NOISE_FN double noise_gauss(uint64_t seed, uint32_t tick, uint32_t obj, uint32_t comp, uint32_t* words = nullptr)
{
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint64_t K = 0;
    for (uint32_t b = 0; b < 3; ++b) {
        const uint32_t ctr[4] = {tick, obj, 3u * comp + b, 0u};
        uint32_t o[4];
        philox4x32_10(ctr, k0, k1, o);
        K += (uint64_t)o[0] + o[1] + o[2] + o[3];
        if (words) { words[4 * b] = o[0]; words[4 * b + 1] = o[1]; words[4 * b + 2] = o[2]; words[4 * b + 3] = o[3]; }
    }
    return ((double)K + 6.0) * (1.0 / 4294967296.0) - 6.0;
}

FLEET_NOISE_FN double noise_add(double v, double sigma, uint64_t seed, uint32_t tick, uint32_t obj, uint32_t comp)
{
    if (sigma == 0.0) return v;
    return v + sigma * noise_gauss(seed, tick, obj, comp);
}
// speeds: the perturbed value clamped at 0 (a NaN becomes 0 as well); sigma == 0 hands v through, clamp included
FLEET_NOISE_FN double noise_add_speed(double v, double sigma, uint64_t seed, uint32_t tick, uint32_t obj, uint32_t comp)
{
    if (sigma == 0.0) return v;
    const double w = v + sigma * noise_gauss(seed, tick, obj, comp);
    return w > 0.0 ? w : 0.0;
}

}  // namespace fleet
