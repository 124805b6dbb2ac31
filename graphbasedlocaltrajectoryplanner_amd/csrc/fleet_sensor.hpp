// fleet_sensor.hpp -- the sensor model of the fleet's closed-loop simulation (ltpl_fleet_sim_sensor, include/ltpl_hip.h): which of the tick's
// on-track objects a planner is shown. Plain functions, host- and device-compilable, no HIP types: tests/sim_sensor_shim.cpp compiles this
// file alone with the host compiler; the host mirror is sim.SensorModel / sim.sensor_uniform. A pure function of the tick's true state: no
// memory from tick to tick. fp64, + - * sqrt and comparisons only, in the order written here (built with -ffp-contract=off on both sides).
//
// Per planner: the true pose (px, py), the forward unit vector f = (fx, fy) and the tick's staged objects k = 0 .. n - 1 at their TRUE
// positions with their radii. Derived, in this order:  dx = x - px; dy = y - py; L2 = dx dx + dy dy.
// An object is tested in this order; the first test that fails is its cause of loss:
//   1 range      L2 > range range                                             (range = +inf: never)
//   2 near field L2 <= r_near r_near: tests 3 and 4 are skipped
//   3 fov        fov_cos > -1 and fx dx + fy dy < fov_cos sqrt(L2)            (fov_cos = -1: not evaluated)
//   4 occlusion  occl > 0 and some j != k of ALL n objects (lost ones included) with
//                L2_j < L2_k  and  dx_j dx_k + dy_j dy_k > 0  and  cross cross <= ((occl r_j) (occl r_j)) L2_k,  cross = dx_j dy_k - dy_j dx_k
//   5 dropout    p_drop > 0 and u < p_drop, u = ((double)w0 + 0.5) 2^-32 with w0 the first output word of ONE Philox4x32-10 block, key = the
//                sensor's seed, counter (tick, k, 0, 1). Every block of noise_gauss (fleet_noise.hpp) has 0 in counter word 3: the same
//                seed may serve both. p_drop == 0 draws nothing
// blind clearance of a lost object: sqrt(L2) - r (telemetry's clearance formula, on truth).
#pragma once

#include <cmath>
#include <cstdint>

#include "fleet_noise.hpp"

#define FLEET_SENSOR_FN FLEET_NOISE_FN

namespace fleet {

enum { kSenseSeen = 0, kSenseRange = 1, kSenseFov = 2, kSenseOccl = 3, kSenseDrop = 4 };

struct SensorParams { double range, r_near, fov_cos, occl, p_drop; };

// the object's own geometry, staged once per object
struct SensorObj { double dx, dy, L2; };
FLEET_SENSOR_FN SensorObj sensor_obj(double px, double py, double x, double y)
{
    const double dx = x - px, dy = y - py;
    return SensorObj{dx, dy, dx * dx + dy * dy};
}

FLEET_SENSOR_FN double sensor_uniform(uint64_t seed, uint32_t tick, uint32_t k, uint32_t* words = nullptr)
{
    const uint32_t ctr[4] = {tick, k, 0u, 1u};
    uint32_t o[4];
    philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32), o);
    if (words) { words[0] = o[0]; words[1] = o[1]; words[2] = o[2]; words[3] = o[3]; }
    return ((double)o[0] + 0.5) * (1.0 / 4294967296.0);
}

// object j hides object k (test 4 without the `occl > 0` guard)
FLEET_SENSOR_FN bool sensor_hides(double occl, double dxj, double dyj, double L2j, double rj, double dxk, double dyk, double L2k)
{
    if (!(L2j < L2k)) return false;
    if (!(dxj * dxk + dyj * dyk > 0.0)) return false;
    const double cross = dxj * dyk - dyj * dxk, s = occl * rj;
    return cross * cross <= (s * s) * L2k;
}

// cause of loss of object k among the n objects (dx, dy, L2, r: arrays of n; on the device: LDS, every lane walks j in step, a broadcast).
// `u`: the dropout draw where one was made (untouched otherwise)
FLEET_SENSOR_FN int sensor_cause(const SensorParams& P, uint64_t seed, uint32_t tick, double fx, double fy, const double* dx, const double* dy,
                                 const double* L2, const double* r, int n, int k, double* u)
{
    const double dxk = dx[k], dyk = dy[k], L2k = L2[k];
    if (L2k > P.range * P.range) return kSenseRange;
    if (!(L2k <= P.r_near * P.r_near)) {
        if (P.fov_cos > -1.0 && fx * dxk + fy * dyk < P.fov_cos * sqrt(L2k)) return kSenseFov;
        if (P.occl > 0.0) {
            bool hidden = false;
            for (int j = 0; j < n; ++j)
                if (j != k && sensor_hides(P.occl, dx[j], dy[j], L2[j], r[j], dxk, dyk, L2k)) hidden = true;
            if (hidden) return kSenseOccl;
        }
    }
    if (P.p_drop > 0.0) {
        const double v = sensor_uniform(seed, tick, (uint32_t)k);
        *u = v;
        if (v < P.p_drop) return kSenseDrop;
    }
    return kSenseSeen;
}

FLEET_SENSOR_FN double sensor_clearance(double L2, double r) { return sqrt(L2) - r; }

}  // namespace fleet
