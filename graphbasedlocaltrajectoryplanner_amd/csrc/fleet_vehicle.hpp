// fleet_vehicle.hpp -- the vehicle model of the fleet's closed-loop simulation (ltpl_fleet_sim_vehicle, include/ltpl_hip.h): a kinematic
// single-track car with actuator lags, a friction circle of its TRUE grip and a pure-pursuit / speed controller, between the planned
// trajectory and the pose the next tick starts from. Plain functions, host- and device-compilable, no HIP types: tests/sim_vehicle_shim.cpp
// compiles this file alone with the host compiler; the host mirror is sim.VehicleModel. fp64, + - * / sqrt only (fabs / copysign / compares
// are exact), one fixed operation order, built with -ffp-contract=off on both sides: host and device agree to the last bit. The heading is
// carried as a unit vector (c, s), never as an angle: the direction of travel. (The library's heading theta is measured from the y axis:
// c = -sin theta, s = cos theta at the call that sets the state, theta = atan2(-c, s) where the tick hands the heading on.)
//
// A tick of dt on the trajectory rows s, x, y, vx, ax (n rows):
//   t = 0; k = 0; while (t < dt) { if (k % ctl_steps == 0) control; plant; t += 0.001; ++k; }    then (c, s) /= sqrt(c c + s s)
// CONTROL (veh_control) at the pose p = (x, y):
//   projection  every segment i = 0 .. n - 2 with l2 = dx dx + dy dy > 0 (veh_seg): u = ((px - x_i) dx + (py - y_i) dy) / l2 clamped to
//               [0, 1], foot f = (x_i + u dx, y_i + u dy), d2 = |p - f|^2; the smallest d2 wins, ties to the lower i (veh_better; the
//               device searches with one lane per segment and a wave-wide minimum, the host serially: veh_search). On the winner
//               e = (dx (py - y_i) - dy (px - x_i)) / sqrt(l2) (left of the trajectory: positive), sf = s_i + u (s_{i+1} - s_i)
//   references  vref, aff = np.interp of vx, ax at sf (veh_interp on veh_segment: the arithmetic of fleet::sim_interp / sim_segment)
//   look-ahead  Ld = max(ld_min, t_look v), st = sf + Ld; target = np.interp of x, y at st (clamped at the last row); where st > s_{n-1}
//               the target is extended by (st - s_{n-1}) (dx / sqrt(l2), dy / sqrt(l2)) of the LAST segment with l2 > 0
//   curvature   r = target - p, yl = -s r_x + c r_y, L2 = r_x r_x + r_y r_y, kappa_cmd = L2 > 0 ? (2 yl) / L2 : 0, clamped to +-kappa_max
//   friction    ay_lim = ay_max grip, ax_lim = ax_max grip, v2 = v v; |kappa_cmd| v2 > ay_lim: kappa_cmd = copysign(ay_lim / v2, kappa_cmd),
//               sat_lat counts; q = (kappa_cmd v2) / ay_lim, rem = ax_lim sqrt(max(0, 1 - q q)); a_cmd = aff + k_v (vref - v) clamped to
//               +-rem, sat_lon counts where it was clamped
//   statistics  e, e_max = max |e|, e2_sum += e e, dv_max = max |vref - v|, ctl += 1
//   no usable trajectory (n <= 2, or no segment with l2 > 0): the steering is held (kappa_cmd = kappa), a_cmd = -ax_lim, and NO
//               statistic changes (ctl counts the control steps that had a trajectory: e2_sum / ctl is the mean square error)
// PLANT (veh_plant), h = 0.001:
//   a += (a_cmd - a) (h / tau_a); kappa += (kappa_cmd - kappa) (h / tau_kappa); v += a h, a negative v becomes 0; ds = v h;
//   t = 0.5 kappa ds; c' = ((1 - t t) c - (2 t) s) / (1 + t t), s' = ((1 - t t) s + (2 t) c) / (1 + t t)  (the rotation by 2 atan t);
//   x += ds (0.5 (c + c')), y += ds (0.5 (s + s'))  (the chord of that rotation);  (c, s) = (c', s')
// With kappa and v constant the car stays on the circle of radius 1 / kappa up to rounding: the chord of a rotation by phi with
// tan(phi / 2) = t and length ds cos(phi / 2) belongs to the radius ds / (2 t).
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define FLEET_VEH_FN __host__ __device__ inline
#else
#define FLEET_VEH_FN inline
#endif

namespace fleet {

static constexpr double kVehStep = 0.001;           // the plant's step (SIM_DT_STEP of the other two simulators)

struct VehState { double x, y, c, s, v, a, kappa; };
struct VehParams { double ax_max, ay_max, grip, kappa_max, tau_a, tau_kappa, k_v, t_look, ld_min; };
struct VehStats { double e, e_max, e2_sum, dv_max, ctl, sat_lat, sat_lon; };
struct VehRows { const double* s; const double* x; const double* y; const double* vx; const double* ax; int n; };
struct VehCmd { double kappa, a; };
struct VehBest { double d; int i; };
static constexpr int kVehNone = 0x7fffffff;         // VehBest::i of a search that met no segment with l2 > 0

// the arithmetic of fleet::sim_segment / fleet::sim_interp (fleet_sim.hpp: numpy's arr_interp for a scalar) on plain columns
FLEET_VEH_FN int veh_segment(double x, const double* xp, int n)
{
    if (!(x >= xp[0])) return -1;
    int lo = 0, hi = n;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (xp[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}
FLEET_VEH_FN double veh_interp(double x, const double* xp, const double* fp, int n, int j)
{
    if (x != x) return x;
    if (j < 0) return fp[0];
    if (j >= n - 1) return fp[n - 1];
    const double xj = xp[j], f0 = fp[j];
    if (xj == x) return f0;
    const double f1 = fp[j + 1];
    const double slope = (f1 - f0) / (xp[j + 1] - xj);
    double r = slope * (x - xj) + f0;
    if (r != r) {
        r = slope * (x - xp[j + 1]) + f1;
        if (r != r && f0 == f1) r = f0;
    }
    return r;
}

FLEET_VEH_FN VehBest veh_better(VehBest a, VehBest b) { return (b.d < a.d || (b.d == a.d && b.i < a.i)) ? b : a; }

// segment i as a candidate of the projection: false where its length is zero (such a segment is never offered)
FLEET_VEH_FN bool veh_seg(const VehRows& R, int i, double px, double py, double* d2, double* u_out = nullptr)
{
    const double dx = R.x[i + 1] - R.x[i], dy = R.y[i + 1] - R.y[i];
    const double l2 = dx * dx + dy * dy;
    if (!(l2 > 0.0)) return false;
    double u = ((px - R.x[i]) * dx + (py - R.y[i]) * dy) / l2;
    if (u < 0.0) u = 0.0;
    if (u > 1.0) u = 1.0;
    const double fx = R.x[i] + u * dx, fy = R.y[i] + u * dy;
    const double ex = px - fx, ey = py - fy;
    *d2 = ex * ex + ey * ey;
    if (u_out) *u_out = u;
    return true;
}
// the serial search (host; the device walks the segments with one lane each and reduces with the same veh_better)
FLEET_VEH_FN VehBest veh_search(const VehRows& R, double px, double py)
{
    VehBest b{INFINITY, kVehNone};
    for (int i = 0; i + 1 < R.n; ++i) {
        double d2;
        if (veh_seg(R, i, px, py, &d2)) b = veh_better(b, VehBest{d2, i});
    }
    return b;
}

FLEET_VEH_FN VehCmd veh_control(const VehState& S, const VehParams& P, const VehRows& R, VehBest best, VehStats& st)
{
    const double ax_lim = P.ax_max * P.grip, ay_lim = P.ay_max * P.grip;
    const int n = R.n, i = best.i;
    if (n <= 2 || i < 0 || i >= n - 1) return VehCmd{S.kappa, -ax_lim};
    const double px = S.x, py = S.y;
    double d2, u;
    veh_seg(R, i, px, py, &d2, &u);
    const double dx = R.x[i + 1] - R.x[i], dy = R.y[i + 1] - R.y[i];
    const double l2 = dx * dx + dy * dy;
    const double e = (dx * (py - R.y[i]) - dy * (px - R.x[i])) / sqrt(l2);
    const double sf = R.s[i] + u * (R.s[i + 1] - R.s[i]);
    const int j = veh_segment(sf, R.s, n);
    const double vref = veh_interp(sf, R.s, R.vx, n, j), aff = veh_interp(sf, R.s, R.ax, n, j);
    const double tl = P.t_look * S.v;
    const double Ld = tl > P.ld_min ? tl : P.ld_min;
    const double sl = sf + Ld;
    const int jt = veh_segment(sl, R.s, n);
    double gx = veh_interp(sl, R.s, R.x, n, jt), gy = veh_interp(sl, R.s, R.y, n, jt);
    if (sl > R.s[n - 1]) {
        for (int k = n - 2; k >= 0; --k) {                  // (segment `i` has a length: the walk ends there at the latest)
            const double ex = R.x[k + 1] - R.x[k], ey = R.y[k + 1] - R.y[k];
            const double m2 = ex * ex + ey * ey;
            if (m2 > 0.0) {
                const double m = sqrt(m2), over = sl - R.s[n - 1];
                gx += over * (ex / m); gy += over * (ey / m);
                break;
            }
        }
    }
    const double rx = gx - px, ry = gy - py;
    const double yl = -S.s * rx + S.c * ry;
    const double L2 = rx * rx + ry * ry;
    double kc = L2 > 0.0 ? (2.0 * yl) / L2 : 0.0;
    if (kc > P.kappa_max) kc = P.kappa_max;
    if (kc < -P.kappa_max) kc = -P.kappa_max;
    const double v2 = S.v * S.v;
    if (fabs(kc) * v2 > ay_lim) { kc = copysign(ay_lim / v2, kc); st.sat_lat += 1.0; }
    const double q = (kc * v2) / ay_lim;
    const double w = 1.0 - q * q;
    const double rem = ax_lim * sqrt(w > 0.0 ? w : 0.0);
    const double dv = vref - S.v;
    double ac = aff + P.k_v * dv;
    if (ac > rem) { ac = rem; st.sat_lon += 1.0; }
    else if (ac < -rem) { ac = -rem; st.sat_lon += 1.0; }
    st.e = e;
    if (fabs(e) > st.e_max) st.e_max = fabs(e);
    st.e2_sum += e * e;
    if (fabs(dv) > st.dv_max) st.dv_max = fabs(dv);
    st.ctl += 1.0;
    return VehCmd{kc, ac};
}

FLEET_VEH_FN void veh_plant(VehState& S, const VehParams& P, VehCmd cmd)
{
    const double h = kVehStep;
    S.a += (cmd.a - S.a) * (h / P.tau_a);
    S.kappa += (cmd.kappa - S.kappa) * (h / P.tau_kappa);
    S.v += S.a * h;
    if (S.v < 0.0) S.v = 0.0;
    const double ds = S.v * h;
    const double t = 0.5 * S.kappa * ds;
    const double tt = t * t, t2 = 2.0 * t;
    const double cn = ((1.0 - tt) * S.c - t2 * S.s) / (1.0 + tt), sn = ((1.0 - tt) * S.s + t2 * S.c) / (1.0 + tt);
    S.x += ds * (0.5 * (S.c + cn));
    S.y += ds * (0.5 * (S.s + sn));
    S.c = cn; S.s = sn;
}

// one tick; `search(px, py)` -> VehBest: veh_search, or the wave-wide form of the kernels (every lane then runs this loop on the same values)
template <class SEARCH>
FLEET_VEH_FN void veh_tick(VehState& S, const VehParams& P, const VehRows& R, double dt, int ctl_steps, VehStats& st, SEARCH search)
{
    double t = 0.0;
    int k = 0;
    VehCmd cmd{S.kappa, 0.0};
    while (t < dt) {
        if (k % ctl_steps == 0) cmd = veh_control(S, P, R, R.n > 2 ? search(S.x, S.y) : VehBest{INFINITY, kVehNone}, st);
        veh_plant(S, P, cmd);
        t += kVehStep;
        ++k;
    }
    const double r = sqrt(S.c * S.c + S.s * S.s);
    S.c = S.c / r; S.s = S.s / r;
}

}  // namespace fleet
