// fleet_safety.hpp -- the safety monitor of the fleet's closed-loop simulation (ltpl_fleet_sim_safety, include/ltpl_hip.h): surrogate safety
// measures of every tick (time to collision, required deceleration, time headway, gap, impact speed), a per-planner record and an incident
// log. Plain functions, host- and device-compilable, no HIP types: tests/sim_safety_shim.cpp compiles this file alone with the host
// compiler; the host mirror is sim.SafetyModel. Measurement only: nothing here is read by the planner. fp64, + - * / sqrt and comparisons
// only, in the order written here (built with -ffp-contract=off on both sides); no sin / cos / atan2.
//
// Per planner and live tick: the TRUE pose P = (px, py), dt, the monitor's tick index, the pose of the previous live tick (kept in the
// record) and the tick's staged on-track objects k = 0 .. n - 1: position X = (ox, oy), the ingestion's 0.2 s point Q = (qx, qy), radius r_o.
// Ego velocity W = ((px - prev_x) / dt, (py - prev_y) / dt): the displacement the car really made. A tick with a valid previous pose is
// EVALUATED; one without (the first after the call, the first after a branch from a source without a record) counts in `ticks`, moves the
// gap fields and overlap_ticks with W = (0, 0) and stores the pose -- nothing else.
// Per object (safety_obj), in this order:
//   1  ux = (qx - ox) / 0.2, uy = (qy - oy) / 0.2
//   2  rx = ox - px, ry = oy - py; vx = ux - wx, vy = uy - wy
//   3  rr = rx rx + ry ry; dist = sqrt(rr)
//   4  gap = (dist - r_o) - r_ego
//   5  rho = r_o + r_ego; c = rr - rho rho; b = rx vx + ry vy; a = vx vx + vy vy
//   6  rr, a, b or r_o not finite: SKIPPED -- counted, takes part in nothing
//   7  overlap = !(gap > 0)
//   8  closing = b < 0 ? (-b) / dist : 0; with dist == 0: sqrt(a)
//   9  ttc = 0 when overlap or !(c > 0); else with b < 0 and disc = b b - a c >= 0 (a COLLISION COURSE): c / (sqrt(disc) - b); else +inf
//   10 drac = (closing closing) / (2 gap) when not overlapping and on a collision course, else 0
//   11 w2 = wx wx + wy wy, wn = sqrt(w2); with wn > 0: lon = (rx wx + ry wy) / wn, lat = (rx wy - ry wx) / wn; IN THE CORRIDOR when
//      lon > 0 and |lat| <= rho + margin: thw = (lon - rho) / wn, 0 when !(lon - rho > 0); otherwise, and with wn == 0, +inf
// Per tick (SafetyTick): gap_t and ttc_t minima on the key (value, slot), ties to the lower slot, a NaN never wins, slot -1 without an
// object; drac_t, impact_t (closing over the overlapping objects) and closing_t maxima from 0; thw_t a minimum from +inf; overlap and
// skipped counts. The record and the incident ring: safety_apply.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FLEET_SAFETY_FN __host__ __device__ inline
#else
#define FLEET_SAFETY_FN inline
#endif

namespace fleet {

enum { SAF_TICKS = 0, SAF_TICKS_EVAL, SAF_PREV_X, SAF_PREV_Y, SAF_PREV_VALID, SAF_GAP_MIN, SAF_GAP_TICK, SAF_GAP_SLOT, SAF_TTC_MIN, SAF_TTC_TICK,
       SAF_TTC_SLOT, SAF_TET, SAF_TIT, SAF_DRAC_MAX, SAF_DRAC_TICK, SAF_DRAC_TICKS, SAF_THW_MIN, SAF_THW_TICKS, SAF_OVERLAP_TICKS, SAF_IMPACT_MAX,
       SAF_N_SKIPPED, SAF_N_INCIDENTS, SAF_INC_OPEN, SAF_HIST, SAF_DOUBLES = SAF_HIST + 8 };
enum { SAF_INC_FIRST = 0, SAF_INC_LAST, SAF_INC_TTC, SAF_INC_SLOT, SAF_INC_GAP, SAF_INC_CLOSING, SAF_INC_DOUBLES };
enum { kSafIncidents = 8, kSafNoSlot = 0x7fffffff };
enum { kSafSkipped = 1, kSafOverlap = 2, kSafCourse = 4, kSafCorridor = 8 };

struct SafetyParams { double r_ego, ttc_thr, drac_thr, thw_thr, margin; };
struct SafetyObj { double ttc, drac, thw, gap, closing; int flags; };

FLEET_SAFETY_FN bool safety_finite(double v) { return v - v == 0.0; }

FLEET_SAFETY_FN SafetyObj safety_obj(const SafetyParams& P, double px, double py, double wx, double wy, double ox, double oy, double qx, double qy,
                                     double r_o)
{
    const double ux = (qx - ox) / 0.2, uy = (qy - oy) / 0.2;
    const double rx = ox - px, ry = oy - py, vx = ux - wx, vy = uy - wy;
    const double rr = rx * rx + ry * ry, dist = sqrt(rr);
    const double gap = (dist - r_o) - P.r_ego;
    const double rho = r_o + P.r_ego, c = rr - rho * rho, b = rx * vx + ry * vy, a = vx * vx + vy * vy;
    SafetyObj o{INFINITY, 0.0, INFINITY, gap, 0.0, 0};
    if (!safety_finite(rr) || !safety_finite(a) || !safety_finite(b) || !safety_finite(r_o)) { o.flags = kSafSkipped; return o; }
    const bool overlap = !(gap > 0.0);
    double closing = 0.0;
    if (dist == 0.0) closing = sqrt(a);
    else if (b < 0.0) closing = (-b) / dist;
    o.closing = closing;
    const double disc = b * b - a * c;
    const bool course = b < 0.0 && disc >= 0.0;
    if (overlap || !(c > 0.0)) o.ttc = 0.0;
    else if (course) o.ttc = c / (sqrt(disc) - b);
    if (!overlap && course) o.drac = (closing * closing) / (2.0 * gap);
    const double w2 = wx * wx + wy * wy, wn = sqrt(w2);
    bool corridor = false;
    if (wn > 0.0) {
        const double lon = (rx * wx + ry * wy) / wn, lat = (rx * wy - ry * wx) / wn;
        const double al = lat < 0.0 ? -lat : lat;
        if (lon > 0.0 && al <= rho + P.margin) {
            corridor = true;
            const double d = lon - rho;
            o.thw = d > 0.0 ? d / wn : 0.0;
        }
    }
    o.flags = (overlap ? (int)kSafOverlap : 0) | (course ? (int)kSafCourse : 0) | (corridor ? (int)kSafCorridor : 0);
    return o;
}

// the tick's values: one fold per lane on the device (safety_fold over its objects, then the wave's reductions), one over all objects on
// the host. The fold leaves the two counts alone: the caller counts (the host in its loop, the device by ballot / popcount)
struct SafetyTick {
    double gap, ttc, drac, thw, impact, closing;
    int gap_slot, ttc_slot, overlaps, skipped;
};
FLEET_SAFETY_FN SafetyTick safety_tick_start() { return SafetyTick{INFINITY, INFINITY, 0.0, INFINITY, 0.0, 0.0, kSafNoSlot, kSafNoSlot, 0, 0}; }
FLEET_SAFETY_FN void safety_fold(SafetyTick& T, const SafetyObj& o, int slot)
{
    if (o.flags & kSafSkipped) return;
    if (o.gap < T.gap || (o.gap == T.gap && slot < T.gap_slot)) { T.gap = o.gap; T.gap_slot = slot; }
    if (o.ttc < T.ttc || (o.ttc == T.ttc && slot < T.ttc_slot)) { T.ttc = o.ttc; T.ttc_slot = slot; }
    if (o.drac > T.drac) T.drac = o.drac;
    if (o.thw < T.thw) T.thw = o.thw;
    if (o.closing > T.closing) T.closing = o.closing;
    if ((o.flags & kSafOverlap) && o.closing > T.impact) T.impact = o.closing;
}

// the start state of a record and of a planner's ring
FLEET_SAFETY_FN void safety_start(double* rec, double* inc)
{
    for (int i = 0; i < SAF_DOUBLES; ++i) rec[i] = 0.0;
    rec[SAF_GAP_MIN] = INFINITY; rec[SAF_TTC_MIN] = INFINITY; rec[SAF_THW_MIN] = INFINITY;
    if (inc) for (int i = 0; i < kSafIncidents * SAF_INC_DOUBLES; ++i) inc[i] = NAN;
}

// the record and incident rules of one live tick (lane 0 on the device). `evaluated`: the record held a valid previous pose when the tick
// began (T then computed with its W). Slots arrive as kSafNoSlot where there was no object and are stored as -1
FLEET_SAFETY_FN void safety_apply(double* rec, double* inc, const SafetyParams& P, double px, double py, double dt, double tick, bool evaluated,
                                  const SafetyTick& T)
{
    const double gap_slot = T.gap_slot == kSafNoSlot ? -1.0 : (double)T.gap_slot, ttc_slot = T.ttc_slot == kSafNoSlot ? -1.0 : (double)T.ttc_slot;
    rec[SAF_TICKS] += 1.0;
    if (T.gap < rec[SAF_GAP_MIN]) { rec[SAF_GAP_MIN] = T.gap; rec[SAF_GAP_TICK] = tick; rec[SAF_GAP_SLOT] = gap_slot; }
    if (T.overlaps > 0) rec[SAF_OVERLAP_TICKS] += 1.0;
    rec[SAF_PREV_X] = px; rec[SAF_PREV_Y] = py; rec[SAF_PREV_VALID] = 1.0;
    if (!evaluated) return;
    rec[SAF_TICKS_EVAL] += 1.0;
    if (T.ttc < rec[SAF_TTC_MIN]) { rec[SAF_TTC_MIN] = T.ttc; rec[SAF_TTC_TICK] = tick; rec[SAF_TTC_SLOT] = ttc_slot; }
    const bool below = T.ttc < P.ttc_thr;
    if (below) { rec[SAF_TET] += dt; rec[SAF_TIT] += (P.ttc_thr - T.ttc) * dt; }
    if (T.drac > rec[SAF_DRAC_MAX]) { rec[SAF_DRAC_MAX] = T.drac; rec[SAF_DRAC_TICK] = tick; }
    if (T.drac > P.drac_thr) rec[SAF_DRAC_TICKS] += 1.0;
    if (T.thw < rec[SAF_THW_MIN]) rec[SAF_THW_MIN] = T.thw;
    if (T.thw < P.thw_thr) rec[SAF_THW_TICKS] += 1.0;
    if (T.impact > rec[SAF_IMPACT_MAX]) rec[SAF_IMPACT_MAX] = T.impact;
    rec[SAF_N_SKIPPED] += (double)T.skipped;
    int bin = 7;
    for (int j = 6; j >= 0; --j) if (T.ttc < (P.ttc_thr * (double)(j + 1)) / 7.0) bin = j;
    rec[SAF_HIST + bin] += 1.0;
    if (!below) { rec[SAF_INC_OPEN] = 0.0; return; }
    if (rec[SAF_INC_OPEN] == 0.0) {
        rec[SAF_N_INCIDENTS] += 1.0; rec[SAF_INC_OPEN] = 1.0;
        double* e = inc + (size_t)((long long)(rec[SAF_N_INCIDENTS] - 1.0) % kSafIncidents) * SAF_INC_DOUBLES;
        e[SAF_INC_FIRST] = tick; e[SAF_INC_LAST] = tick; e[SAF_INC_TTC] = T.ttc; e[SAF_INC_SLOT] = ttc_slot; e[SAF_INC_GAP] = T.gap;
        e[SAF_INC_CLOSING] = T.closing;
    } else {
        double* e = inc + (size_t)((long long)(rec[SAF_N_INCIDENTS] - 1.0) % kSafIncidents) * SAF_INC_DOUBLES;
        e[SAF_INC_LAST] = tick;
        if (T.ttc < e[SAF_INC_TTC]) { e[SAF_INC_TTC] = T.ttc; e[SAF_INC_SLOT] = ttc_slot; }
        if (T.gap < e[SAF_INC_GAP]) e[SAF_INC_GAP] = T.gap;
        if (T.closing > e[SAF_INC_CLOSING]) e[SAF_INC_CLOSING] = T.closing;
    }
}

// the ego velocity of the tick: (0, 0) without a valid previous pose
FLEET_SAFETY_FN bool safety_velocity(const double* rec, double px, double py, double dt, double* wx, double* wy)
{
    if (rec[SAF_PREV_VALID] == 0.0) { *wx = 0.0; *wy = 0.0; return false; }
    *wx = (px - rec[SAF_PREV_X]) / dt; *wy = (py - rec[SAF_PREV_Y]) / dt;
    return true;
}

// one tick on the host, all objects in turn: objs[n][5] = x, y, px, py, r. per_obj (or null) [n][6] = ttc, drac, thw, gap, closing, flags;
// per_tick (or null) [8] = gap_t, gap_slot, ttc_t, ttc_slot, drac_t, thw_t, impact_t, closing_t
FLEET_SAFETY_FN void safety_tick_out(const SafetyTick& T, double* per_tick)
{
    per_tick[0] = T.gap; per_tick[1] = T.gap_slot == kSafNoSlot ? -1.0 : (double)T.gap_slot;
    per_tick[2] = T.ttc; per_tick[3] = T.ttc_slot == kSafNoSlot ? -1.0 : (double)T.ttc_slot;
    per_tick[4] = T.drac; per_tick[5] = T.thw; per_tick[6] = T.impact; per_tick[7] = T.closing;
}
inline void safety_tick_host(const SafetyParams& P, double px, double py, double dt, double tick, const double* objs, int n, double* rec, double* inc,
                             double* per_obj, double* per_tick)
{
    double wx, wy;
    const bool evaluated = safety_velocity(rec, px, py, dt, &wx, &wy);
    SafetyTick T = safety_tick_start();
    for (int k = 0; k < n; ++k) {
        const double* o = objs + (size_t)5 * k;
        const SafetyObj s = safety_obj(P, px, py, wx, wy, o[0], o[1], o[2], o[3], o[4]);
        safety_fold(T, s, k);
        if (s.flags & kSafSkipped) ++T.skipped;
        if (s.flags & kSafOverlap) ++T.overlaps;
        if (per_obj) {
            double* q = per_obj + (size_t)6 * k;
            q[0] = s.ttc; q[1] = s.drac; q[2] = s.thw; q[3] = s.gap; q[4] = s.closing; q[5] = (double)s.flags;
        }
    }
    if (per_tick) safety_tick_out(T, per_tick);
    safety_apply(rec, inc, P, px, py, dt, tick, evaluated, T);
}

}  // namespace fleet
