// fleet_predict.hpp -- the prediction model of the fleet's closed-loop simulation (ltpl_fleet_sim_predictor, include/ltpl_hip.h): where the
// objects a planner is handed will be over the next `horizon` seconds, as 1 + K positions per object in place of the ingestion's two.
// Plain functions, host- and device-compilable, no HIP types: tests/sim_predictor_shim.cpp compiles this file alone with the host
// compiler; the host mirror is sim.PredictorModel. A pure function of the tick's staged list: no memory from tick to tick. fp64,
// + - * / sqrt and comparisons only, in the order written here (built with -ffp-contract=off on both sides).
//
// Per object: x, y (the position), px, py (the ingestion's 0.2 s point), v (the speed), as staged for the planner this tick. Per planner:
// mode, horizon T > 0, relax in [0, 1], d_max >= 0 (+inf allowed). Fleet-wide: K = n_points in 1 .. 8 and the race-line table S, X, Y of n
// rows (SimDev::race, columns s_rl, x, y). Output: K points for the times t_j = (T j) / K, j = 1 .. K.
//   mode 0  as ingested: every point is (px, py)
//   mode 1  straight line: c_j = t_j / 0.2; (x + (px - x) c_j, y + (py - y) c_j)
//   mode 2  along the track:
//     1 nearest row   i* = the first row with the smallest d2_i = dx dx + dy dy, dx = X_i - x, dy = Y_i - y (np.argmin; a d2 that is NaN
//                     or +inf is never smaller: if every one is, i* = 0)
//     2 segment       candidates (i* - 1, i*) and (i*, i* + 1), no wrap at the table's ends. Segment (a, a + 1): ex = X_b - X_a,
//                     ey = Y_b - Y_a, l2 = ex ex + ey ey, skipped when l2 == 0; t = ((x - X_a) ex + (y - Y_a) ey) / l2 clamped to [0, 1];
//                     foot fx = X_a + t ex, fy = Y_a + t ey; q2 = (x - fx)(x - fx) + (y - fy)(y - fy). The upper candidate wins only with
//                     a smaller q2. s0 = S_a + t (S_b - S_a); d = (ex (y - Y_a) - ey (x - X_a)) / sqrt(l2)
//     3 points        s_j = s0 + v t_j; s_j >= S[n - 1]: s_j -= S[n - 1], once (a wrap). Segment g = the largest row with S_g <= s_j
//                     (bisection; -1 below S[0]); X(s_j), Y(s_j) = np.interp on it, clamped at both ends (veh_segment / veh_interp of
//                     fleet_vehicle.hpp: the arithmetic of fleet::sim_segment / fleet::sim_interp). Direction: the segment
//                     (g', g' + 1), g' = g clamped to 0 .. n - 2: ux = ex / sqrt(l2), uy = ey / sqrt(l2); d_j = d (1 - relax (j / K));
//                     the point is (X(s_j) - d_j uy, Y(s_j) + d_j ux), or (X(s_j), Y(s_j)) where l2 == 0
//     4 fallbacks     to the straight line of mode 1, tested in this order: no candidate segment; |d| > d_max (equality stays);
//                     (px - x) ex + (py - y) ey < 0 on the chosen segment (the object moves against the track)
// Decided first, in this order: mode 0 is "as ingested" whatever v is; in modes 1 and 2 an object with !(v > 0) is "still": K copies
// of (px, py).
#pragma once

#include <cmath>

#include "fleet_vehicle.hpp"

#define FLEET_PRED_FN FLEET_VEH_FN

namespace fleet {

static constexpr int kPredMaxPoints = 8;
static constexpr double kPredIngestT = 0.2;          // s: the horizon of the ingestion's point (ObjectListInterface.py:121)

// outcome of an object; in this order the counters [2] .. [8] of the planner's record
enum { kPredIngested = 0, kPredStill, kPredStraightMode, kPredStraightDmax, kPredStraightDir, kPredStraightNoSeg, kPredTrack, kPredOutcomes };
// the planner's record (LTPL_FLEET_SIM_PREDICTOR_DOUBLES)
enum { PRS_TICKS = 0, PRS_N_OBJ, PRS_OUTCOME0, PRS_D_MAX = PRS_OUTCOME0 + kPredOutcomes, PRS_N_WRAP, PRS_DOUBLES };

struct PredParams { double mode, horizon, relax, d_max; };
struct PredTable { const double* s; const double* x; const double* y; int n; };
struct PredProj { int outcome; double s0, d; };
struct PredPoint { double x, y; bool wrapped; };

FLEET_PRED_FN double pred_d2(double x, double y, double X, double Y)
{
    const double dx = X - x, dy = Y - y;
    return dx * dx + dy * dy;
}

// step 1 on the host (the device strides the rows with the wave and takes the minimum over (d2, i))
FLEET_PRED_FN int pred_nearest(const PredTable& R, double x, double y)
{
    double bd = INFINITY; int bi = 0;
    for (int i = 0; i < R.n; ++i) {
        const double d2 = pred_d2(x, y, R.x[i], R.y[i]);
        if (d2 < bd) { bd = d2; bi = i; }
    }
    return bi;
}

// candidate segment (a, a + 1) of step 2: false where l2 == 0
struct PredCand { double t, q2, ex, ey, l2; };
FLEET_PRED_FN bool pred_candidate(const PredTable& R, int a, double x, double y, PredCand* c)
{
    const double ex = R.x[a + 1] - R.x[a], ey = R.y[a + 1] - R.y[a];
    const double l2 = ex * ex + ey * ey;
    if (l2 == 0.0) return false;
    double t = ((x - R.x[a]) * ex + (y - R.y[a]) * ey) / l2;
    if (t < 0.0) t = 0.0;
    if (t > 1.0) t = 1.0;
    const double fx = R.x[a] + t * ex, fy = R.y[a] + t * ey;
    const double gx = x - fx, gy = y - fy;
    *c = PredCand{t, gx * gx + gy * gy, ex, ey, l2};
    return true;
}

// the decisions of an object, steps 2 and 4 on the nearest row `istar` (mode 2 only reads it)
FLEET_PRED_FN PredProj pred_project(const PredParams& P, const PredTable& R, int istar, double x, double y, double px, double py, double v)
{
    PredProj o{kPredIngested, 0.0, 0.0};
    if (P.mode == 0.0) return o;
    if (!(v > 0.0)) { o.outcome = kPredStill; return o; }
    if (P.mode == 1.0) { o.outcome = kPredStraightMode; return o; }
    PredCand c{}, hi{};
    int a = -1;
    if (istar >= 1 && pred_candidate(R, istar - 1, x, y, &c)) a = istar - 1;
    if (istar + 1 < R.n && pred_candidate(R, istar, x, y, &hi) && (a < 0 || hi.q2 < c.q2)) { c = hi; a = istar; }
    if (a < 0) { o.outcome = kPredStraightNoSeg; return o; }
    o.s0 = R.s[a] + c.t * (R.s[a + 1] - R.s[a]);
    o.d = (c.ex * (y - R.y[a]) - c.ey * (x - R.x[a])) / sqrt(c.l2);
    if (o.d > P.d_max || -o.d > P.d_max) { o.outcome = kPredStraightDmax; return o; }
    if ((px - x) * c.ex + (py - y) * c.ey < 0.0) { o.outcome = kPredStraightDir; return o; }
    o.outcome = kPredTrack;
    return o;
}

FLEET_PRED_FN double pred_abs(double d) { return d < 0.0 ? -d : d; }

// point j = 1 .. K of an object
FLEET_PRED_FN PredPoint pred_point(const PredParams& P, const PredTable& R, int K, int j, const PredProj& o, double x, double y, double px, double py,
                                   double v)
{
    if (o.outcome == kPredIngested || o.outcome == kPredStill) return PredPoint{px, py, false};
    const double tj = (P.horizon * (double)j) / (double)K;
    if (o.outcome != kPredTrack) {
        const double cj = tj / kPredIngestT;
        return PredPoint{x + (px - x) * cj, y + (py - y) * cj, false};
    }
    double sj = o.s0 + v * tj;
    bool wrapped = false;
    if (sj >= R.s[R.n - 1]) { sj = sj - R.s[R.n - 1]; wrapped = true; }
    const int g = veh_segment(sj, R.s, R.n);
    const double X = veh_interp(sj, R.s, R.x, R.n, g), Y = veh_interp(sj, R.s, R.y, R.n, g);
    const int q = g < 0 ? 0 : (g > R.n - 2 ? R.n - 2 : g);
    const double ex = R.x[q + 1] - R.x[q], ey = R.y[q + 1] - R.y[q];
    const double l2 = ex * ex + ey * ey;
    if (l2 == 0.0) return PredPoint{X, Y, wrapped};
    const double l = sqrt(l2), ux = ex / l, uy = ey / l;
    const double dj = o.d * (1.0 - P.relax * ((double)j / (double)K));
    return PredPoint{X - dj * uy, Y + dj * ux, wrapped};
}

}  // namespace fleet
