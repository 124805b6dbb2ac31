// fleet_react.hpp -- the reactive opponents of the fleet's closed-loop simulation (ltpl_fleet_sim_react, include/ltpl_hip.h): a
// car-following rule that sets every race-line opponent's EFFECTIVE vel_scale at the head of a tick from the car ahead of it on the race
// line -- another opponent or the ego. Plain functions, host- and device-compilable, no HIP types: tests/sim_react_shim.cpp compiles this
// file alone with the host compiler; the host mirror is sim.ReactModel / sim.react_tick. fp64, + - * / sqrt and comparisons only, in the
// order written here (built with -ffp-contract=off on both sides); no pow, no trigonometry.
//
// Per planner and tick: the TRUE pose (x, y) and speed v of the previous tick, dt, the model's tick index, the race table S, X, Y, V of n
// rows (lap length L = S[n - 1]) and per opponent q: s_q, the configured scale c_q, the effective scale e_q (the state), the length l_q.
//   0  the ego on the race line: steps 1 and 2 of fleet_predict.hpp (pred_nearest, pred_candidate) give (s_e, d_e) or nothing; the ego is a
//      possible leader iff a projection exists and |d_e| <= lat_gate (equality inside, a NaN outside)
//   1  Vq = veh_interp(V) at s_q; v_q = e_q Vq. Decided first: !(c_q > 0) or !(Vq > 0): PASSIVE, e' = c_q, counted; as a leader of others
//      its speed is c_q Vq
//   2  leader: candidates in the order ego, opponents r = 0 .. no - 1 (r != q). D = s_j - s_q; D < 0: D = D + L. Against an opponent with
//      D == 0: r < q is ahead at 0, r > q a lap ahead (D = L). Only a strictly smaller D replaces (the ego wins ties, then the lower index;
//      a NaN never wins). No leader unless D <= look. Leader's speed u and length l_j: the ego's (v, ego_len), opponent r's (e_r V(s_r), l_r)
//      with e_r of the START of the tick
//   3  gap = (D - 0.5 l_j) - 0.5 l_q
//   4  r = e_q / c_q; free = 1 - (r r)(r r). No leader: acc = a_max free. Leader and !(gap > 0): acc = -b_max (an OVERLAP). Otherwise
//      dv = v_q - u; z = v_q headway + (v_q dv) / (2 sqrt(a_max b_comf)), !(z > 0): 0; k = (gap0 + z) / gap; acc = a_max (free - k k).
//      Then acc < -b_max: -b_max (CLAMPED, counted); acc > a_max: a_max
//   5  e' = e_q + (acc dt) / Vq; !(e' > 0): 0; e' > c_q: c_q
// With no leader and e == c: r = 1, free = 0, acc = 0, e' = e + 0 / Vq = e -- a field that never finds a leader drives the blind run bit
// for bit. Every opponent reads the values of the start of the tick: the result does not depend on the order of evaluation.
#pragma once

#include <cmath>

#include "fleet_predict.hpp"

#define FLEET_REACT_FN FLEET_VEH_FN

namespace fleet {

// the planner's record (LTPL_FLEET_SIM_REACT_DOUBLES)
enum { RCT_TICKS = 0, RCT_OPP_TICKS, RCT_FOLLOW_TICKS, RCT_EGO_LEAD_TICKS, RCT_CLAMPED, RCT_OVERLAPS, RCT_PASSIVE, RCT_GAP_MIN, RCT_GAP_TICK,
       RCT_GAP_SLOT, RCT_ACC_MIN, RCT_ACC_TICK, RCT_ACC_SLOT, RCT_EGO_GAP_MIN, RCT_EGO_GAP_TICK, RCT_EGO_OUTSIDE, RCT_DOUBLES };
enum { kReactNone = -2, kReactEgo = -1, kReactNoSlot = 0x7fffffff, kReactMaxOpp = 96 };
enum { kReactPassive = 1, kReactFollow = 2, kReactEgoLead = 4, kReactOverlap = 8, kReactClamped = 16 };

struct ReactParams { double on, a_max, b_comf, b_max, headway, gap0, look, lat_gate, ego_len; };
struct ReactTable { const double* s; const double* x; const double* y; const double* v; int n; };
// the ego of the tick: has (a candidate segment exists), lead (has and inside the gate), s / d of the projection, its speed
struct ReactEgo { bool has, lead; double s, d, v; };
struct ReactOpp { double e, delta, gap, acc; int leader, flags; };

// step 0 on the nearest row `istar` (pred_nearest on the host; the wave's minimum over (d2, i) on the device)
FLEET_REACT_FN ReactEgo react_ego(const ReactParams& P, const ReactTable& R, int istar, double x, double y, double v)
{
    const PredTable T{R.s, R.x, R.y, R.n};
    PredCand c{}, hi{};
    int a = -1;
    if (istar >= 1 && pred_candidate(T, istar - 1, x, y, &c)) a = istar - 1;
    if (istar + 1 < R.n && pred_candidate(T, istar, x, y, &hi) && (a < 0 || hi.q2 < c.q2)) { c = hi; a = istar; }
    ReactEgo E{false, false, 0.0, 0.0, v};
    if (a < 0) return E;
    E.has = true;
    E.s = R.s[a] + c.t * (R.s[a + 1] - R.s[a]);
    E.d = (c.ex * (y - R.y[a]) - c.ey * (x - R.x[a])) / sqrt(c.l2);
    E.lead = pred_abs(E.d) <= P.lat_gate;
    return E;
}

// the race line's speed at s (step 1)
FLEET_REACT_FN double react_vrl(const ReactTable& R, double s) { return veh_interp(s, R.s, R.v, R.n, veh_segment(s, R.s, R.n)); }
FLEET_REACT_FN bool react_passive(double c, double Vq) { return !(c > 0.0) || !(Vq > 0.0); }
// an opponent's speed as a leader of others, from the values of the start of the tick
FLEET_REACT_FN double react_speed(double c, double e, double Vq) { return react_passive(c, Vq) ? c * Vq : e * Vq; }

// steps 1 .. 5 of opponent q among `no` opponents: s / u / len the staged s, leader speed (react_speed) and length of every opponent
FLEET_REACT_FN ReactOpp react_opp(const ReactParams& P, const ReactTable& R, const ReactEgo& E, double dt, int q, int no, const double* s,
                                  const double* u, const double* len, double c_q, double e_q, double Vq)
{
    ReactOpp o{c_q, INFINITY, INFINITY, 0.0, kReactNone, 0};
    if (react_passive(c_q, Vq)) { o.flags = kReactPassive; return o; }
    const double L = R.s[R.n - 1], s_q = s[q], l_q = len[q];
    const double v_q = e_q * Vq;
    double best = INFINITY, ul = 0.0, ll = 0.0;
    int leader = kReactNone;
    if (E.lead) {
        double D = E.s - s_q;
        if (D < 0.0) D = D + L;
        if (D < best) { best = D; leader = kReactEgo; ul = E.v; ll = P.ego_len; }
    }
    for (int r = 0; r < no; ++r) {
        if (r == q) continue;
        double D = s[r] - s_q;
        if (D < 0.0) D = D + L;
        if (D == 0.0 && r > q) D = L;
        if (D < best) { best = D; leader = r; ul = u[r]; ll = len[r]; }
    }
    if (leader != kReactNone && !(best <= P.look)) leader = kReactNone;
    const double r = e_q / c_q;
    const double free = 1.0 - (r * r) * (r * r);
    double acc;
    if (leader == kReactNone) {
        acc = P.a_max * free;
    } else {
        o.delta = best;
        o.gap = (best - 0.5 * ll) - 0.5 * l_q;
        o.flags |= kReactFollow | (leader == kReactEgo ? (int)kReactEgoLead : 0);
        if (!(o.gap > 0.0)) {
            acc = -P.b_max;
            o.flags |= kReactOverlap;
        } else {
            const double dv = v_q - ul;
            double z = v_q * P.headway + (v_q * dv) / (2.0 * sqrt(P.a_max * P.b_comf));
            if (!(z > 0.0)) z = 0.0;
            const double k = (P.gap0 + z) / o.gap;
            acc = P.a_max * (free - k * k);
        }
    }
    if (acc < -P.b_max) { acc = -P.b_max; o.flags |= kReactClamped; }
    if (acc > P.a_max) acc = P.a_max;
    double e = e_q + (acc * dt) / Vq;
    if (!(e > 0.0)) e = 0.0;
    if (e > c_q) e = c_q;
    o.e = e; o.acc = acc; o.leader = leader;
    return o;
}

// the tick's values: one fold per lane on the device (react_fold over its opponents, then the wave's reductions), one over all opponents
// on the host. The fold leaves the counts alone: the caller counts (the host in its loop, the device by ballot / popcount)
struct ReactTick {
    double gap, acc, ego_gap;
    int gap_slot, acc_slot, follow, ego_lead, clamped, overlaps, passive;
};
FLEET_REACT_FN ReactTick react_tick_start() { return ReactTick{INFINITY, INFINITY, INFINITY, kReactNoSlot, kReactNoSlot, 0, 0, 0, 0, 0}; }
FLEET_REACT_FN void react_fold(ReactTick& T, const ReactOpp& o, int slot)
{
    if (o.flags & kReactPassive) return;
    if (o.acc < T.acc || (o.acc == T.acc && slot < T.acc_slot)) { T.acc = o.acc; T.acc_slot = slot; }
    if (!(o.flags & kReactFollow)) return;
    if (o.gap < T.gap || (o.gap == T.gap && slot < T.gap_slot)) { T.gap = o.gap; T.gap_slot = slot; }
    if ((o.flags & kReactEgoLead) && o.gap < T.ego_gap) T.ego_gap = o.gap;
}

// the start state of a record
FLEET_REACT_FN void react_start(double* rec)
{
    for (int i = 0; i < RCT_DOUBLES; ++i) rec[i] = 0.0;
    rec[RCT_GAP_MIN] = INFINITY; rec[RCT_ACC_MIN] = INFINITY; rec[RCT_EGO_GAP_MIN] = INFINITY;
    rec[RCT_GAP_TICK] = -1.0; rec[RCT_GAP_SLOT] = -1.0; rec[RCT_ACC_TICK] = -1.0; rec[RCT_ACC_SLOT] = -1.0; rec[RCT_EGO_GAP_TICK] = -1.0;
}

// the record rules of one tick (lane 0 on the device)
FLEET_REACT_FN void react_apply(double* rec, const ReactEgo& E, int no, double tick, const ReactTick& T)
{
    rec[RCT_TICKS] += 1.0;
    rec[RCT_OPP_TICKS] += (double)no;
    rec[RCT_FOLLOW_TICKS] += (double)T.follow;
    rec[RCT_EGO_LEAD_TICKS] += (double)T.ego_lead;
    rec[RCT_CLAMPED] += (double)T.clamped;
    rec[RCT_OVERLAPS] += (double)T.overlaps;
    rec[RCT_PASSIVE] += (double)T.passive;
    if (T.gap < rec[RCT_GAP_MIN]) { rec[RCT_GAP_MIN] = T.gap; rec[RCT_GAP_TICK] = tick; rec[RCT_GAP_SLOT] = (double)T.gap_slot; }
    if (T.acc < rec[RCT_ACC_MIN]) { rec[RCT_ACC_MIN] = T.acc; rec[RCT_ACC_TICK] = tick; rec[RCT_ACC_SLOT] = (double)T.acc_slot; }
    if (T.ego_gap < rec[RCT_EGO_GAP_MIN]) { rec[RCT_EGO_GAP_MIN] = T.ego_gap; rec[RCT_EGO_GAP_TICK] = tick; }
    if (E.has && !E.lead) rec[RCT_EGO_OUTSIDE] += 1.0;
}

// one tick on the host, all opponents in turn: opp[n][4] = s, c, e, length (n <= kReactMaxOpp). e_out[n]; per_opp (or null) [n][4] =
// leader (-2 none, -1 ego, else index), delta, gap, acc; ego_out (or null) [3] = s_e, d_e, has
inline void react_tick_host(const ReactParams& P, const ReactTable& R, double x, double y, double v, double dt, double tick, const double* opp,
                            int n, double* rec, double* e_out, double* per_opp, double* ego_out)
{
    const ReactEgo E = react_ego(P, R, pred_nearest(PredTable{R.s, R.x, R.y, R.n}, x, y), x, y, v);
    if (ego_out) { ego_out[0] = E.s; ego_out[1] = E.d; ego_out[2] = E.has ? 1.0 : 0.0; }
    double s[kReactMaxOpp], u[kReactMaxOpp], len[kReactMaxOpp], V[kReactMaxOpp];
    for (int q = 0; q < n; ++q) {
        const double* o = opp + (size_t)4 * q;
        s[q] = o[0]; len[q] = o[3]; V[q] = react_vrl(R, o[0]); u[q] = react_speed(o[1], o[2], V[q]);
    }
    ReactTick T = react_tick_start();
    for (int q = 0; q < n; ++q) {
        const double* o = opp + (size_t)4 * q;
        const ReactOpp r = react_opp(P, R, E, dt, q, n, s, u, len, o[1], o[2], V[q]);
        react_fold(T, r, q);
        T.follow += (r.flags & kReactFollow) != 0; T.ego_lead += (r.flags & kReactEgoLead) != 0; T.clamped += (r.flags & kReactClamped) != 0;
        T.overlaps += (r.flags & kReactOverlap) != 0; T.passive += (r.flags & kReactPassive) != 0;
        e_out[q] = r.e;
        if (per_opp) { double* w = per_opp + (size_t)4 * q; w[0] = (double)r.leader; w[1] = r.delta; w[2] = r.gap; w[3] = r.acc; }
    }
    react_apply(rec, E, n, tick, T);
}

}  // namespace fleet
