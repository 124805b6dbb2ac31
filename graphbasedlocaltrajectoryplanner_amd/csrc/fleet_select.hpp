// fleet_select.hpp -- the behaviour selector of the fleet's closed-loop simulation (ltpl_fleet_sim_selector, include/ltpl_hip.h): which of
// the previous tick's exported trajectories a planner should drive, as an ORDERED preference list that k_fleet_sim_step walks exactly as
// it walks the user's list. Plain functions, host- and device-compilable, no HIP types: tests/sim_selector_shim.cpp compiles this file
// alone with the host compiler; the host mirror is sim.SelectorModel. A pure function of its inputs: no memory from tick to tick. fp64,
// + - * / sqrt and comparisons only, in the order written here (built with -ffp-contract=off on both sides).
//
// Inputs: the user's list (1 .. 5 entries of LTPL_ACT_*: the allowed set plus the tie order; the rule never adds an action), sel_prev (the
// action of the previous tick), the exported set (per action: exported or not, and rows 0 .. n - 1, n = min(rows, n_export), columns s, x,
// y, vx), the staged objects of the previous tick (x, y, the ingestion's 0.2 s point px, py, radius r) and the parameters horizon T > 0,
// r_ego >= 0, c_hard, c_soft, w_clear >= 0, w_switch >= 0.
// An action a is SCORED when it is straight, follow, left or right, stands in the user's list, is exported and has n >= 2:
//   1 times      t_0 = 0; row i >= 1: m = v_i + v_{i-1}; the first row with !(m > 0) (a NaN included) is n_r: the car stands from there on,
//                rows >= n_r are unreachable; n_r = n without one. Otherwise t_i = t_{i-1} + (2 (s_i - s_{i-1})) / m. The WINDOW is the set of
//                reachable rows with t_i <= T (a NaN time is in no window; row 0 always is), `last` its highest row.
//   2 pace       row last + 1 reachable: f = (T - t_last) / (t_{last+1} - t_last), s_T = s_last + f (s_{last+1} - s_last),
//                vbar = (s_T - s_0) / T; else the car stands (n_r < n): vbar = (s_last - s_0) / T; else the trajectory ends inside the
//                horizon: vbar = (s_last - s_0) / t_last, and vbar = v_0 when t_last == 0
//   3 clearance  every window row i against every object o: c = t_i / 0.2, X = x_o + (px_o - x_o) c, Y = y_o + (py_o - y_o) c,
//                d = (sqrt((x_i - X)(x_i - X) + (y_i - Y)(y_i - Y)) - r_o) - r_ego; clear = the smallest d, +inf without objects; the
//                minimum is taken on the key (d, 256 o + i) by sel_better: a NaN d never wins, ties go to the lower (object, row);
//                clear_obj = o of the minimum, -1 where no pair won
//   4 score      pen = c_soft - clear, 0 unless pen > 0; J = (vbar - w_clear pen) - (a != sel_prev ? w_switch : 0). J != J (a NaN):
//                the action is UNSAFE and ranks with clearance -inf (its reported clear stays). Otherwise unsafe when !(clear >= c_hard):
//                equality is safe, c_hard = -inf makes every action with a number for a score safe
//   5 order      every ENTRY e of the user's list gets a group and a key: 0 safe scored, key J; 1 emergency, key 0; 2 unsafe scored, key
//                clear (-inf with a NaN score); 3 every other entry (not exported, n < 2, not one of the four), key 0. Entry f stands before
//                entry e when group_f < group_e, or the groups are equal and (key_f > key_e, or !(key_e > key_f) and f < e): within a group
//                larger keys first, ties in the user's order. The keys of one group hold no NaN, so this is a strict total order and the
//                output is a permutation of the user's list; a duplicated entry keeps its copies side by side.
// Not evaluated (the list is copied unchanged, the record untouched): a planner switched off in the mask, a planner that has not started
// or has its error word set, and a one-entry list.
// THE ACTION TAKEN is the first entry of a list that is in the exported set (emergency included), -1 without one; the record compares
// the one of the ordered list with the one of the user's list.
#pragma once

#include <cmath>

#include "fleet_vehicle.hpp"

#define FLEET_SEL_FN FLEET_VEH_FN

namespace fleet {

static constexpr int kSelActions = 4;                // straight, follow, left, right: LTPL_ACT_* 0 .. 3
static constexpr int kSelEmergency = 4;              // LTPL_ACT_EMERGENCY
static constexpr int kSelMaxPref = 5;                // LTPL_FLEET_SIM_MAX_PREF
static constexpr int kSelMaxRows = 256;              // LTPL_FLEET_SIM_MAX_EXPORT
static constexpr int kSelMaxObj = 96;
static constexpr int kSelNone = 0x7fffffff;
static constexpr double kSelIngestT = 0.2;           // s: the horizon of the ingestion's point (ObjectListInterface.py:121)

// flags of an action
enum { kSelScored = 1, kSelUnsafe = 2, kSelNan = 4, kSelExported = 8 };
// the planner's record (LTPL_FLEET_SIM_SELECTOR_DOUBLES)
enum { SLS_TICKS = 0, SLS_N_SCORED, SLS_N_SWITCH, SLS_N_OVERRIDE, SLS_N_UNSAFE, SLS_N_EMERGENCY, SLS_CHOSEN0, SLS_CLEAR_MIN = SLS_CHOSEN0 + kSelActions,
       SLS_J_LAST, SLS_DOUBLES };

struct SelParams { double horizon, r_ego, c_hard, c_soft, w_clear, w_switch; };
struct SelAct { int flags; int clear_obj; double vbar, clear, J; };
struct SelBest { double d; int i; };

FLEET_SEL_FN SelBest sel_better(SelBest a, SelBest b) { return (b.d < a.d || (b.d == a.d && b.i < a.i)) ? b : a; }

// step 1, row i >= 1: its time step; *stand: the car stands from this row on
FLEET_SEL_FN double sel_dt(double s0, double s1, double v0, double v1, bool* stand)
{
    const double m = v1 + v0;
    *stand = !(m > 0.0);
    return (2.0 * (s1 - s0)) / m;
}
// step 1, the serial part: t[1 .. n_r - 1] hold the time steps and become the times; returns `last`
FLEET_SEL_FN int sel_prefix(double* t, int n_r, double T)
{
    double a = 0.0;
    int last = 0;
    t[0] = 0.0;
    for (int i = 1; i < n_r; ++i) {
        a = a + t[i];
        t[i] = a;
        if (a <= T) last = i;
    }
    return last;
}
// step 2
FLEET_SEL_FN double sel_vbar(const double* s, double v0, const double* t, int n, int n_r, int last, double T)
{
    if (last + 1 < n_r) {
        const double f = (T - t[last]) / (t[last + 1] - t[last]);
        const double sT = s[last] + f * (s[last + 1] - s[last]);
        return (sT - s[0]) / T;
    }
    if (n_r < n) return (s[last] - s[0]) / T;
    if (t[last] == 0.0) return v0;
    return (s[last] - s[0]) / t[last];
}
// step 3, one (row, object) pair
FLEET_SEL_FN double sel_gap(double x, double y, double t, double ox, double oy, double opx, double opy, double orad, double r_ego)
{
    const double c = t / kSelIngestT;
    const double X = ox + (opx - ox) * c, Y = oy + (opy - oy) * c;
    const double dx = x - X, dy = y - Y;
    return (sqrt(dx * dx + dy * dy) - orad) - r_ego;
}
// step 4 on a scored action whose vbar and clear are set
FLEET_SEL_FN void sel_score(const SelParams& P, int a, int sel_prev, SelAct* A)
{
    double pen = P.c_soft - A->clear;
    if (!(pen > 0.0)) pen = 0.0;
    const double sw = a != sel_prev ? P.w_switch : 0.0;
    A->J = (A->vbar - P.w_clear * pen) - sw;
    if (A->J != A->J) A->flags |= kSelNan | kSelUnsafe;
    else if (!(A->clear >= P.c_hard)) A->flags |= kSelUnsafe;
}
// step 5: group and key of the entry `a`
FLEET_SEL_FN int sel_group(int a, const SelAct* A, double* key)
{
    *key = 0.0;
    if (a == kSelEmergency) return 1;
    if (a < 0 || a >= kSelActions || !(A[a].flags & kSelScored)) return 3;
    if (A[a].flags & kSelUnsafe) { *key = (A[a].flags & kSelNan) ? -INFINITY : A[a].clear; return 2; }
    *key = A[a].J;
    return 0;
}
// step 5: the place of entry e in the ordered list
FLEET_SEL_FN int sel_rank(int e, const int* user, int L, const SelAct* A)
{
    double ke, kf;
    const int ge = sel_group(user[e], A, &ke);
    int r = 0;
    for (int f = 0; f < L; ++f) {
        if (f == e) continue;
        const int gf = sel_group(user[f], A, &kf);
        if (gf < ge || (gf == ge && (kf > ke || (!(ke > kf) && f < e)))) ++r;
    }
    return r;
}
// the action taken from a list: its first entry in the exported set (bit a of `exported`), -1 without one
FLEET_SEL_FN int sel_first(const int* list, int L, unsigned exported)
{
    for (int i = 0; i < L; ++i) if (list[i] >= 0 && list[i] <= kSelEmergency && ((exported >> list[i]) & 1u)) return list[i];
    return -1;
}
// the record of one evaluation
FLEET_SEL_FN void sel_record(double* rec, const int* user, const int* ord, int L, const SelAct* A, unsigned exported, int sel_prev)
{
    const int taken = sel_first(ord, L, exported), alone = sel_first(user, L, exported);
    int n_scored = 0, n_safe = 0;
    for (int a = 0; a < kSelActions; ++a) {
        if (A[a].flags & kSelScored) { ++n_scored; if (!(A[a].flags & kSelUnsafe)) ++n_safe; }
    }
    rec[SLS_TICKS] += 1.0;
    rec[SLS_N_SCORED] += (double)n_scored;
    if (taken >= 0 && taken != sel_prev) rec[SLS_N_SWITCH] += 1.0;
    if (taken != alone) rec[SLS_N_OVERRIDE] += 1.0;
    if (n_safe == 0) rec[SLS_N_UNSAFE] += 1.0;
    if (taken == kSelEmergency) rec[SLS_N_EMERGENCY] += 1.0;
    else if (taken >= 0) rec[SLS_CHOSEN0 + taken] += 1.0;
    if (taken >= 0 && taken < kSelActions && (A[taken].flags & kSelScored)) {
        if (A[taken].clear < rec[SLS_CLEAR_MIN]) rec[SLS_CLEAR_MIN] = A[taken].clear;
        rec[SLS_J_LAST] = A[taken].J;
    }
}

// One whole evaluation in plain serial code (the host side of the rule; the device spreads steps 1 and 3 over a wave).
// n_rows[a] for a = 0 .. 4: -1 not exported, else n (entry 4: emergency, only the sign is read); rows: [4][4][256] = per action the
// columns s, x, y, vx; objs: [cnt][5] = x, y, px, py, r; out: order[L], act[4]; rec (or null): the planner's record, updated
inline void sel_case(const SelParams& P, const int* user, int L, int sel_prev, const int* n_rows, const double* rows, const double* objs, int cnt,
                     int* order, SelAct* act, double* rec)
{
    unsigned exported = 0;
    for (int a = 0; a <= kSelEmergency; ++a) if (n_rows[a] >= 0) exported |= 1u << a;
    double t[kSelMaxRows];
    for (int a = 0; a < kSelActions; ++a) {
        SelAct& A = act[a];
        A = SelAct{n_rows[a] >= 0 ? (int)kSelExported : 0, -1, 0.0, INFINITY, 0.0};
        bool listed = false;
        for (int e = 0; e < L; ++e) listed = listed || user[e] == a;
        const int n = n_rows[a];
        if (!listed || n < 2) continue;
        A.flags |= kSelScored;
        const double* s = rows + (size_t)a * 4 * kSelMaxRows; const double* x = s + kSelMaxRows; const double* y = x + kSelMaxRows; const double* v = y + kSelMaxRows;
        int n_r = n;
        for (int i = 1; i < n; ++i) {
            bool stand;
            t[i] = sel_dt(s[i - 1], s[i], v[i - 1], v[i], &stand);
            if (stand) { n_r = i; break; }
        }
        const int last = sel_prefix(t, n_r, P.horizon);
        A.vbar = sel_vbar(s, v[0], t, n, n_r, last, P.horizon);
        SelBest b{INFINITY, kSelNone};
        for (int o = 0; o < cnt; ++o) {
            const double* q = objs + (size_t)5 * o;
            for (int i = 0; i <= last; ++i)
                if (t[i] <= P.horizon) b = sel_better(b, SelBest{sel_gap(x[i], y[i], t[i], q[0], q[1], q[2], q[3], q[4], P.r_ego), o * kSelMaxRows + i});
        }
        A.clear = b.d; A.clear_obj = b.i == kSelNone ? -1 : b.i / kSelMaxRows;
        sel_score(P, a, sel_prev, &A);
    }
    for (int e = 0; e < L; ++e) order[sel_rank(e, user, L, act)] = user[e];
    if (rec) sel_record(rec, user, order, L, act, exported, sel_prev);
}

}  // namespace fleet
