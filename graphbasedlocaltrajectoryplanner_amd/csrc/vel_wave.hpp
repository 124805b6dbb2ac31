// vel_wave.hpp -- the velocity stage (seam 2), ONE WAVE PER PROFILE: the recurrences of tph.calc_vel_profile / _brake / _follow over
// LDS-resident arrays (DevVelParams ... follow_profile), the job kernel of the seam and of the fleet (k_vel_profile) and the per-primitive
// velocity stage of the fused tick (tick_vel_stage). Included by ltpl_hip.hip behind the path kernel (needs DevLat, DevPathsIn / Out,
// WavePath, wave_ops.hpp).
#pragma once
// Standstill in the w = v^2 state. The reference compares v > 0.1; the kernels compare w > fl(0.1 * 0.1) = 0.010000000000000002, NOT the
// literal 0.01: for v = 0.1 exactly (a v_start or v_obj of 0.1 m/s) fl(v * v) exceeds 0.01 and the car would count as moving where the
// reference has it stopped (ego stop distance one element longer, another branch, vel_bound flipped: tests/vel_cases.py "v_start == 0.1").
// With this constant the two agree for every double: squaring separates neighbouring doubles around 0.1, and sqrt(w) > 0.1 <=> w > fl(0.1^2).
constexpr double W_STANDSTILL = 0.1 * 0.1;
// ---------------------------------------------------------------------------------------------------------------------
// velocity stage (seam 2): tph.calc_vel_profile / calc_vel_profile_brake / calc_vel_profile_follow on the device
// ---------------------------------------------------------------------------------------------------------------------
// One wave64 owns one profile. Vectorisable parts (curvature -> lateral-limit speed, run-start detection, final
// sqrt, acceleration) are spread over the lanes; the forward / backward recurrences are inherently sequential scans
// and run on lane 0 over LDS-resident arrays. The recurrence state is w = v^2, which removes the sqrt and the
// divisions from the dependent chain (v_{i+1}^2 = v_i^2 + 2 a_x(v_i) ds_i); comparisons happen in w as well (sqrt is
// monotone). Differences to the reference's v-state arithmetic are rounding-level (~1e-16 relative).
struct DevVelParams {
    double e, inv_e, drag_m, len_veh, v_max;
    int n_axm, ctrl;
    const double* axm;          // [n_axm * 2] in device memory
    double c_p, k_p, k_d, tan_w;
};

// np.interp(v, axm[:, 0], axm[:, 1]) on the LDS copy of the table
__device__ __forceinline__ double interp_axm(double v, const double* t, int n)
{
    if (n == 1 || v <= t[0]) return t[1];
    if (v >= t[2 * (n - 1)]) return t[2 * (n - 1) + 1];
    int j = 0;
    while (j + 1 < n && t[2 * (j + 1)] <= v) ++j;
    const double x0 = t[2 * j], x1 = t[2 * (j + 1)], f0 = t[2 * j + 1], f1 = t[2 * (j + 1) + 1];
    return (f1 - f0) / (x1 - x0) * (v - x0) + f0;
}

// tire share of tph calc_ax_poss: ax_max * (1 - (ay_used / ay_max)^e)^(1/e), 0 when the radicand is not positive.
// EM selects the exponent at compile time (1: e == 1, 2: e == 2, 0: general pow) so that the recurrences below are
// straight-line code: with one wave per profile every taken branch is a pipeline refill nobody hides.
template <int EM>
__device__ __forceinline__ double tire_avail(double q, double ax_max, const DevVelParams& p)
{
    if constexpr (EM == 1) {
        const double rad = 1.0 - q;
        return rad > 0.0 ? ax_max * rad : 0.0;
    } else if constexpr (EM == 2) {
        const double rad = 1.0 - q * q;
        return rad > 0.0 ? ax_max * sqrt(rad) : 0.0;
    } else {
        const double rad = 1.0 - pow(q, p.e);
        return rad > 0.0 ? ax_max * pow(rad, p.inv_e) : 0.0;
    }
}

#define VMODE_ACCEL_FORW 0
#define VMODE_DECEL_FORW 1
#define VMODE_DECEL_BACKW 2

// tph calc_ax_poss in w = v^2; kq = |kappa| / ay_max (so that ay_used / ay_max = w * kq); axm1 = machine limit when the
// table has a single row (AXM1), otherwise the LDS copy of the table is interpolated at v = sqrt(w)
template <int EM, bool AXM1, int MODE>
__device__ __forceinline__ double ax_poss_w(double w, double kq, double ax_max, const DevVelParams& p,
                                            const double* axm_tab, double axm1)
{
    const double q = w * kq;
    double ax = tire_avail<EM>(q, fabs(ax_max), p);
    if constexpr (MODE == VMODE_ACCEL_FORW) {
        const double axm = AXM1 ? axm1 : interp_axm(sqrt(w), axm_tab, p.n_axm);
        ax = ax < axm ? ax : axm;
        return ax - w * p.drag_m;
    } else if constexpr (MODE == VMODE_DECEL_FORW) {
        return -ax - w * p.drag_m;
    } else {
        return ax + w * p.drag_m;
    }
}

// lane l <- lane l - 1 across the whole wave64 (DPP wave_shr:1); lane 0 receives `first`
__device__ __forceinline__ double wave_shr1_f64(double v, double first)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(first), __double2loint(v), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(first), __double2hiint(v), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int wave_shr1_i32(int v, int first)
{
    return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false);
}

// one sweep of tph __solver_fb_acc_profile on w[0..n). Backward sweeps address the profile, curvature and element
// lengths mirrored but -- restated quirk of the reference solver -- the gg limits unmirrored.
// The recurrence is sequential, but everything except the state is known up front. SYSTOLIC form: the wave handles 64
// steps at a time, lane l holds the operands of step base + l (for exponent 1 and a constant machine limit: the affine
// coefficients); in every iteration ALL lanes evaluate their step on the state handed over by the lane below (DPP
// wave_shr:1, no LDS, no broadcast), so after iteration l lane l holds the final value of its step. One iteration is the
// bare dependent chain: ~a dozen VALU instructions.
template <int EM, bool AXM1, bool GGARR, bool BACK>
__device__ __forceinline__ void fb_sweep(int n, const VelScratch& vs, double cax, double cay, const DevVelParams& p, double vmax2, int lane)
{
    if (n < 2) return;
    // run starts: first index of every run of positive differences of the (mirrored) profile BEFORE the sweep
    for (int i = lane; i < n - 1; i += 64) {
        const int a = BACK ? n - 1 - i : i, b = BACK ? n - 2 - i : i + 1;
        const bool acc = vs.w[b] - vs.w[a] > 0.0;
        bool prev = false;
        if (i > 0) { const int a0 = BACK ? n - i : i - 1, b0 = BACK ? n - 1 - i : i; prev = vs.w[b0] - vs.w[a0] > 0.0; }
        vs.start[i] = (acc && !prev) ? 1 : 0;
    }
    wave_sync_lds();
    constexpr int MODE = BACK ? VMODE_DECEL_BACKW : VMODE_ACCEL_FORW;
    constexpr bool AFFINE = EM == 1 && AXM1;
    const double icay = 1.0 / cay, axm1 = vs.axm[1], dm = p.drag_m;
    double wi = vs.w[BACK ? n - 1 : 0];                   // state entering the chunk (uniform)
    int active = 0;
    for (int base = 0; base < n - 1; base += 64) {
        const int cnt = (n - 1 - base) < 64 ? (n - 1 - base) : 64;
        const int ic = (lane < cnt) ? base + lane : base + cnt - 1;
        const int Pa = BACK ? n - 1 - ic : ic, Pb = BACK ? n - 2 - ic : ic + 1, Ei = BACK ? n - 2 - ic : ic;
        // operands of step ic (the gg limits are indexed by the step, the rest by the mirrored point)
        const double kq_i = vs.kabs[Pa] * (GGARR ? vs.igay[ic] : icay), kq_n = vs.kabs[Pb] * (GGARR ? vs.igay[ic + 1] : icay);
        const double ax_i = GGARR ? fabs(vs.gax[ic]) : fabs(cax), ax_n = GGARR ? fabs(vs.gax[ic + 1]) : fabs(cax);
        const double e_i = vs.el[Ei], wold = vs.w[Pb];
        const int st = vs.start[ic];
        // affine coefficients (state independent):
        //   forward : w' = min(max(T, Z), M),  T = w A1 + B1, Z = w A0, M = w A0 + B2
        //   backward: w' = max(T, Z), then the look-ahead with the limits of the next point (t0 = wn C0 + w, t1 = wn C1 + w + D1)
        const double te = 2.0 * e_i;
        const double A0 = BACK ? 1.0 + te * dm : 1.0 - te * dm, A1 = A0 - te * (ax_i * kq_i), B1 = te * ax_i, B2 = te * axm1;
        const double C0 = te * dm, C1 = C0 - te * (ax_n * kq_n), D1 = te * ax_n;
        double w_in = wi, wnext = wold;
        int act_in = active, act_out = 0;
        // four steps per loop iteration: steps beyond cnt recompute final values from final inputs (idempotent), nothing is stored for them
        auto sys_step = [&]() {
            const bool act = (act_in | st) != 0;
            double wn;
            if constexpr (AFFINE) {
                if constexpr (!BACK) {
                    const double Z = A0 * w_in, T = fma(A1, w_in, B1), M = fma(A0, w_in, B2);
                    wn = fmax(fmin(fmax(T, Z), M), 0.0);
                } else {
                    const double Z = A0 * w_in, T = fma(A1, w_in, B1);
                    wn = fmax(fmax(T, Z), 0.0);
                    const double t0 = fma(C0, wn, w_in), t1 = fma(C1, wn, w_in + D1);
                    wn = fmin(fmax(fmax(t1, t0), 0.0), wn);
                }
            } else {
                const double acur = ax_poss_w<EM, AXM1, MODE>(w_in, kq_i, ax_i, p, vs.axm, axm1);
                wn = w_in + 2.0 * acur * e_i;
                wn = wn < 0.0 ? 0.0 : wn;
                if constexpr (BACK) {
                    const double anext = ax_poss_w<EM, AXM1, MODE>(wn, kq_n, ax_n, p, vs.axm, axm1);
                    double wt = w_in + 2.0 * anext * e_i;
                    wt = wt < 0.0 ? 0.0 : wt;
                    wn = wt < wn ? wt : wn;
                }
            }
            wnext = (act && (wn < wold)) ? wn : wold;
            act_out = (act && !(wn > vmax2)) ? 1 : 0;
            // hand the state to the next lane; lane 0 keeps the state entering the chunk
            w_in = wave_shr1_f64(wnext, wi);
            act_in = wave_shr1_i32(act_out, active);
                };
        for (int it = 0; it < cnt; it += 4) { sys_step(); sys_step(); sys_step(); sys_step(); }
        if (lane < cnt) vs.w[Pb] = wnext;
        wi = readlane_f64(wnext, cnt - 1);
        active = __builtin_amdgcn_readlane(act_out, cnt - 1);
        wave_sync_lds();
    }
}

// tph.calc_vel_profile(closed=False): vs.kabs / el / (gax, gay) hold the inputs, result in vs.w (as v^2)
template <int EM, bool AXM1, bool GGARR>
__device__ __forceinline__ void fb_profile(int n, const VelScratch& vs, double cax, double cay, const DevVelParams& p, double v_max,
                           double v_start, bool has_v_end, double v_end, int lane)
{
    if (v_start < 0.0) v_start = 0.0;
    if (has_v_end && v_end < 0.0) v_end = 0.0;
    const double vmax2 = v_max * v_max;
    for (int i = lane; i < n; i += 64) {
        const double ay = GGARR ? vs.gay[i] : cay;
        double w = ay / vs.kabs[i];                 // ay * radius; kappa == 0 -> inf
        if (!(w < vmax2)) w = vmax2;
        if (i == 0 && w > v_start * v_start) w = v_start * v_start;
        vs.w[i] = w;
    }
    wave_sync_lds();
    dbg_stamp(vs.dbg, 8);
    fb_sweep<EM, AXM1, GGARR, false>(n, vs, cax, cay, p, vmax2, lane);
    dbg_stamp(vs.dbg, 9);
    if (lane == 0 && has_v_end && vs.w[n - 1] > v_end * v_end) vs.w[n - 1] = v_end * v_end;
    wave_sync_lds();
    fb_sweep<EM, AXM1, GGARR, true>(n, vs, cax, cay, p, vmax2, lane);
    dbg_stamp(vs.dbg, 10);
}

// tph.calc_vel_profile_brake on LDS arrays: out[0..n) as v^2, zeros after standstill. Same systolic scheme as fb_sweep.
template <int EM, bool GGARR>
__device__ __forceinline__ void brake_profile(int n, double* out, const VelScratch& vs, double cax, double cay, double v_start,
                              const DevVelParams& p, int lane)
{
    const double icay = 1.0 / cay;
    double w = v_start * v_start;                          // state entering the chunk (uniform)
    int stopped = 0;
    if (lane == 0) out[0] = w;
    for (int base = 0; base < n - 1; base += 64) {
        const int cnt = (n - 1 - base) < 64 ? (n - 1 - base) : 64;
        const int ic = (lane < cnt) ? base + lane : base + cnt - 1;
        const double kq_i = vs.kabs[ic] * (GGARR ? vs.igay[ic] : icay), e_i = vs.el[ic], ax_i = GGARR ? vs.gax[ic] : cax;
        const double te = 2.0 * e_i, axa = fabs(ax_i);
        const double A0 = 1.0 - te * p.drag_m, A1 = A0 + te * (axa * kq_i), B1 = te * axa;
        double w_in = w, w_out = w; int st_in = stopped, st_out = 0;
        double r = 0.0;
        auto sys_step = [&]() {
            if constexpr (EM == 1) r = fmin(fma(A1, w_in, -B1), A0 * w_in);
            else r = w_in + 2.0 * ax_poss_w<EM, true, VMODE_DECEL_FORW>(w_in, kq_i, ax_i, p, vs.axm, 0.0) * e_i;
            st_out = (st_in || (r < 0.0)) ? 1 : 0;
            w_out = st_out ? w_in : r;
            w_in = wave_shr1_f64(w_out, w);
            st_in = wave_shr1_i32(st_out, stopped);
                };
        for (int it = 0; it < cnt; it += 4) { sys_step(); sys_step(); sys_step(); sys_step(); }      // (idempotent beyond cnt)
        if (lane < cnt) out[base + lane + 1] = st_out ? 0.0 : r;
        w = readlane_f64(w_out, cnt - 1);
        stopped = __builtin_amdgcn_readlane(st_out, cnt - 1);
    }
    wave_sync_lds();
}

// out[0] = 0, out[i] = out[i - 1] + src[i - 1] for i < m, in the SEQUENTIAL summation order of np.cumsum (bit-identical),
// executed systolically: lane l adds its element to the partial sum handed over by lane l - 1 (DPP wave_shr:1)
__device__ __forceinline__ void wave_cumsum_seq(const double* src, double* out, int m, int lane)
{
    double carry = 0.0;
    if (lane == 0 && m > 0) out[0] = 0.0;
    for (int base = 0; base < m - 1; base += 64) {
        const int cnt = (m - 1 - base) < 64 ? (m - 1 - base) : 64;
        const double e = src[(lane < cnt) ? base + lane : base + cnt - 1];
        double s_in = carry, s_out = 0.0;
        for (int it = 0; it < cnt; it += 4) {                        // (idempotent beyond cnt)
#pragma unroll
            for (int u = 0; u < 4; ++u) { s_out = s_in + e; s_in = wave_shr1_f64(s_out, carry); }
        }
        if (lane < cnt) out[base + lane + 1] = s_out;
        carry = readlane_f64(s_out, cnt - 1);
    }
    wave_sync_lds();
}

// out[0] = 0, out[i] = sum of src[0 .. i-1] for i < m as a wave-parallel prefix sum (log-step shuffles, 64 elements per round).
// NOT the summation order of np.cumsum: used where the arc length only enters results with a 1e-5 tolerance (distance to the
// object in the batch follow preparation), never where indices are derived from it.
__device__ __forceinline__ void wave_cumsum_par(const double* src, double* out, int m, int lane)
{
    double carry = 0.0;
    if (lane == 0 && m > 0) out[0] = 0.0;
    for (int base = 0; base < m - 1; base += 64) {
        const int i = base + lane;
        const double e = i < m - 1 ? src[i] : 0.0;
        double x = e;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const double y = __shfl_up(x, d); if (lane >= d) x += y; }
        if (i < m - 1) out[i + 1] = carry + x;
        carry += __shfl(x, 63);
    }
    wave_sync_lds();
}

// first index i in [0, m) with pred(i), or m (wave-parallel search; pred is evaluated per lane)
template <typename Pred>
__device__ __forceinline__ int wave_find_first(int m, int lane, Pred pred)
{
    for (int base = 0; base < m; base += 64) {
        const int i = base + lane;
        const unsigned long long b = __ballot(i < m && pred(i));
        if (b) return base + __ffsll((long long)b) - 1;
    }
    return m;
}

__device__ __forceinline__ double angle3pt_dev(double ax, double ay, double bx, double by, double cx, double cy)
{
    double ang = atan2(cy - by, cx - bx) - atan2(ay - by, ax - bx);
    if (ang > D_PI) ang -= 2.0 * D_PI;
    else if (ang <= -D_PI) ang += 2.0 * D_PI;
    return ang;
}

// get_s_coord.py:34-47 picks the neighbour of the closest point by comparing |angle3pt(nb, pos, neighbour)|. The wrapped
// difference of two atan2 values is the angle between u = nb - pos and v = neighbour - pos in [0, pi], and the cosine is
// monotone there: |ang1| > |ang2|  <=>  u.v1 / |v1| < u.v2 / |v2|  (|u| cancels). Two dot products and two square roots instead
// of four atan2 (~600 instructions per projection). Degenerate vectors (pos on a polyline point) take the atan2 form.
// Returns -1 / 0 / +1 for |ang1| < / == / > |ang2|.
// `clamp1` / `clamp2`: the open polyline's index clamp put neighbour 1 / 2 onto the closest point itself (nb = 0 / nb = n - 1). The reference
// then has ang1 (ang2) == 0 EXACTLY -- both atan2 calls see the same vectors -- and never takes the degenerate segment a == b, while the
// cosines compare |u|^2 |v| with itself up to rounding (Cauchy-Schwarz equality) and did, for queries collinear with the end segment:
// t = 0 / 0, s = NaN. Neighbour 1 clamped: -1 (the reference's 0 for ang2 == 0 selects the same segment and the same first index);
// neighbour 2 clamped: +1 (the reference's 0 for ang1 == 0 is its own 0 / 0).
__device__ __forceinline__ int angle_order_dev(double nx, double ny, double px, double py, double x1, double y1, double x2, double y2,
                                               bool clamp1 = false, bool clamp2 = false)
{
    if (clamp2) return 1;
    if (clamp1) return -1;
    const double ux = nx - px, uy = ny - py, v1x = x1 - px, v1y = y1 - py, v2x = x2 - px, v2y = y2 - py;
    const double n1 = v1x * v1x + v1y * v1y, n2 = v2x * v2x + v2y * v2y, nu = ux * ux + uy * uy;
    if (!(n1 > 0.0) || !(n2 > 0.0) || !(nu > 0.0)) {
        const double a1 = fabs(angle3pt_dev(nx, ny, px, py, x1, y1)), a2 = fabs(angle3pt_dev(nx, ny, px, py, x2, y2));
        return a1 > a2 ? 1 : (a1 < a2 ? -1 : 0);
    }
    const double c1 = (ux * v1x + uy * v1y) * sqrt(n2), c2 = (ux * v2x + uy * v2y) * sqrt(n1);
    return c1 < c2 ? 1 : (c1 > c2 ? -1 : 0);
}

// get_s_coord.py:8-99 on a strided polyline in global / LDS memory, all lanes take part; every lane returns s and idx0
__device__ __forceinline__ double get_s_coord_dev(int n, const double* x, const double* y, int stride, const double* s_arr, int s_stride,
                                  double px, double py, bool closed, int lane, int* idx0)
{
    double bd = INFINITY; int nb = 0x7fffffff;
    for (int i = lane; i < n; i += 64) {
        const double dx = x[(size_t)i * stride] - px, dy = y[(size_t)i * stride] - py;
        const double d2 = dx * dx + dy * dy;
        if (d2 < bd) { bd = d2; nb = i; }
    }
    wave_min2(bd, nb);
    int i1, i2;
    if (closed) { i1 = nb - 1; if (i1 < 0) i1 += n; i2 = nb + 1; if (i2 > n - 1) i2 = 0; }
    else { i1 = nb - 1 > 0 ? nb - 1 : 0; i2 = nb + 1 < n - 1 ? nb + 1 : n - 1; }
    const double nx = x[(size_t)nb * stride], ny = y[(size_t)nb * stride];
    const double x1 = x[(size_t)i1 * stride], y1 = y[(size_t)i1 * stride];
    const double x2 = x[(size_t)i2 * stride], y2 = y[(size_t)i2 * stride];
    const int ord = angle_order_dev(nx, ny, px, py, x1, y1, x2, y2, i1 == nb, i2 == nb);
    double ax, ay, bx, by;
    if (ord > 0) { ax = x1; ay = y1; bx = nx; by = ny; } else { ax = nx; ay = ny; bx = x2; by = y2; }
    const double t = ((px - ax) * (bx - ax) + (py - ay) * (by - ay)) / ((bx - ax) * (bx - ax) + (by - ay) * (by - ay));
    const double fx = ax + t * (bx - ax), fy = ay + t * (by - ay);
    const double ds = sqrt((ax - fx) * (ax - fx) + (ay - fy) * (ay - fy));
    const double s = (ord > 0 ? s_arr[(size_t)i1 * s_stride] : s_arr[(size_t)nb * s_stride]) + ds;
    if (idx0) *idx0 = (ord >= 0) ? i1 : nb;
    return s;
}

// Index pair start of the global race line segment an object is projected on (calc_vel_profile_follow.py:172-176:
// get_s_coord(closed=True, only the first index is used). All 2 x ceil(G / 64) loads of a lane are independent: four points per
// round trip from the contiguous x / y copies instead of one strided load per iteration.
__device__ __forceinline__ int globrl_index_dev(const DevLat& lat, double px, double py, int lane)
{
    const int G = lat.G - 1;
    double bd = INFINITY; int nb = 0x7fffffff;
    for (int i0 = 0; i0 < G; i0 += 256) {
        double xs[4], ys[4]; int id[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = i0 + u * 64 + lane; id[u] = i < G ? i : G - 1; xs[u] = at(lat.grx, id[u]); ys[u] = at(lat.gry, id[u]); }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double dx = xs[u] - px, dy = ys[u] - py, d2 = dx * dx + dy * dy;
            if (d2 < bd) { bd = d2; nb = id[u]; }
        }
    }
    wave_min2(bd, nb);
    int i1 = nb - 1; if (i1 < 0) i1 += G;
    int i2 = nb + 1; if (i2 > G - 1) i2 = 0;
    const int ord = angle_order_dev(at(lat.grx, nb), at(lat.gry, nb), px, py, at(lat.grx, i1), at(lat.gry, i1), at(lat.grx, i2), at(lat.gry, i2));
    return ord >= 0 ? i1 : nb;
}

// Index pair start of the global race line segment ONE LANE's object is projected on (calc_vel_profile_follow.py:172-176; the wave form is
// globrl_index_dev): closest race line point (first minimum, like np.argmin; the points are read with uniform indices, every lane compares
// with its own object), then the neighbour test of get_s_coord (closed = True). Every lane of the wave must call it.
__device__ __forceinline__ int lane_globrl_index(const DevLat& lat, double ox, double oy)
{
    const int G = lat.G - 1;
    double bd = INFINITY; int nb = 0;
#pragma unroll 8
    for (int i = 0; i < G; ++i) {
        const double dx = lat.grx[i] - ox, dy = lat.gry[i] - oy, d2 = dx * dx + dy * dy;
        if (d2 < bd) { bd = d2; nb = i; }
    }
    int i1 = nb - 1; if (i1 < 0) i1 += G;
    int i2 = nb + 1; if (i2 > G - 1) i2 = 0;
    const int ord = angle_order_dev(at(lat.grx, nb), at(lat.gry, nb), ox, oy, at(lat.grx, i1), at(lat.gry, i1), at(lat.grx, i2), at(lat.gry, i2));
    return ord >= 0 ? i1 : nb;
}

struct FollowIn { double v_start, v_ego, v_obj, safety_d, obj_dist, obj_x, obj_y; };

// calc_vel_profile_follow.py:78-313. Inputs: vs.kabs[n], vs.el[n_el >= n] (tailing zero), gg; result vs.w (v^2).
// `ext_sync`: when set, the unconstrained profile (:297-307) has been computed by ANOTHER wave of the workgroup into vs.w; the
// function then joins that wave at a workgroup barrier instead of computing it itself (k_tick: wave 3 works for wave 0).
template <int EM, bool AXM1, bool GGARR>
__device__ __forceinline__ void follow_profile(const DevLat& lat, int n, int n_el, const VelScratch& vs, double cax, double cay,
                               const DevVelParams& p, const FollowIn& fi, int lane, int* too_close, int* vel_bound,
                               bool ext_sync = false, bool skip_free = false)
{
    int vb = 1;
    const double control_d = p.c_p * fi.safety_d + p.len_veh;                            // :141
    const double safety_d = fi.safety_d + p.len_veh;                                     // :144
    const int tc = (fi.obj_dist - safety_d) < 0.0;                                       // :147-149
    const double v_max = p.v_max;

    dbg_stamp(vs.dbg, 4);
    brake_profile<EM, GGARR>(n, vs.wb, vs, cax, cay, fi.v_start, p, lane);   // :152-159
    dbg_stamp(vs.dbg, 5);
    // arc length s = [0, cumsum(el[:-1])] (:203) next to the ego stop distance (:162-166)
    wave_cumsum_seq(vs.el, vs.s, n_el, lane);                  // s[i] = sum of el[0 .. i-1], sequential order
    // first point at or below 0.1 m/s on the brake profile; the ego stop distance is the arc length up to it (:162-166)
    int idb = wave_find_first(n, lane, [&](int i) { return !(vs.wb[i] > W_STANDSTILL); });
    if (idb > n_el) idb = n_el;
    double ego_stop = 0.0;
    if (idb > 0) ego_stop = (idb < n_el) ? vs.s[idb] : vs.s[n_el - 1] + vs.el[n_el - 1];

    // opponent: closest point of the global race line (:172-179), brake scan with ggv [100, 14, 14] (:134,185-199)
    const int G = lat.G - 1;
    const double* grl = lat.glob_rl;
    dbg_stamp(vs.dbg, 6);
    const int idx_s_opp = globrl_index_dev(lat, fi.obj_x, fi.obj_y, lane);
    dbg_stamp(vs.dbg, 7);
    const double vel0 = grl[(size_t)idx_s_opp * 5 + 4];
    const double vel_start = fi.v_obj < vel0 ? fi.v_obj : vel0;                          // :182
    double opp_stop = 0.0, wopp = vel_start * vel_start;
    int stopped = (wopp > W_STANDSTILL) ? 0 : 1;                                                 // id_brake counts v > 0.1
    for (int c0 = 0; c0 < G && !stopped; c0 += 64) {
        const int i = c0 + lane;
        if (i < G) {
            int j = i + idx_s_opp; if (j >= G) j -= G;
            vs.chunk[lane] = fabs(grl[(size_t)j * 5 + 3]);
            vs.chunk[64 + lane] = grl[(size_t)(j + 1) * 5] - grl[(size_t)j * 5];
        }
        wave_sync_lds();
        if (lane == 0) {
            const int m = (G - c0) < 64 ? (G - c0) : 64;
            for (int k = 0; k < m; ++k) {
                // point c0 + k has v > 0.1: its element length counts towards the stop distance
                opp_stop += vs.chunk[64 + k];
                if (c0 + k + 1 >= G) { stopped = 1; break; }
                const double a = ax_poss_w<EM, true, VMODE_DECEL_FORW>(wopp, vs.chunk[k] * (1.0 / 14.0), 14.0, p, vs.axm, 0.0);
                const double r = wopp + 2.0 * a * vs.chunk[64 + k];
                wopp = r < 0.0 ? 0.0 : r;                                                // standstill: profile stays 0
                if (!(wopp > W_STANDSTILL)) { stopped = 1; break; }
            }
        }
        stopped = __shfl(stopped, 0);
        wave_sync_lds();
    }
    opp_stop = __shfl(opp_stop, 0);

    dbg_stamp(vs.dbg, 11);
    // characteristic indices (:201-221)
    const double s_stop = fi.obj_dist - safety_d + opp_stop;                             // :206
    int stop_idx = wave_find_first(n_el - 1, lane, [&](int i) { return !(vs.s[i] < s_stop); });   // :208-209
    double v_end = 0.0;
    if (lane == 0) {
        if (s_stop > vs.s[n_el - 1]) {                                                   // :212-221
            const double s_ends = opp_stop - (s_stop - vs.s[n_el - 1]);
            int idx = 0; double summed = 0.0;
            while (summed < s_ends && idx < G) {
                int j = idx + idx_s_opp; if (j >= G) j -= G;
                summed += grl[(size_t)(j + 1) * 5] - grl[(size_t)j * 5];
                ++idx;
            }
            int j = (idx % G) + idx_s_opp; if (j >= G) j -= G;
            v_end = grl[(size_t)j * 5 + 4];
        }
    }
    v_end = __shfl(v_end, 0);
    dbg_stamp(vs.dbg, 12);

    // control velocity (:232-239, get_control_vel :28-75)
    double v_control;
    if (p.ctrl == 0) v_control = (fi.v_obj - p.k_p * (control_d - fi.obj_dist) + p.k_d * (fi.v_obj - fi.v_ego));
    else {
        double a = (control_d - fi.obj_dist) * D_PI / 2 * 1 / p.tan_w;
        const double lo = -D_PI / 2 + 1e-5, hi = D_PI / 2 - 1e-5;
        a = a < lo ? lo : (a > hi ? hi : a);
        v_control = (fi.v_obj - tan(a) * p.k_p + p.k_d * (fi.v_obj - fi.v_ego));
    }
    if (v_control < 0.0) v_control = 0.0;
    if (v_control > v_max) v_control = v_max;

    // vs.wc <- "vx_profile" (:247-294)
    if (ego_stop < s_stop) {
        int idx_c = 0, n_decel = 0; double vcs = fi.v_start;      // vx_control_start
        if (fi.v_start > v_control && stop_idx >= 2) {                                   // :250-258
            const double wctl = v_control * v_control;
            int first = 0x7fffffff;
            for (int i = lane; i < n; i += 64) if (vs.wb[i] <= wctl) { first = i; break; }
            const int di = wave_min_i32(first);                                           // (first index over the lanes: an integer minimum)
            idx_c = (di == 0x7fffffff) ? 0 : di;                                          // np.argmax of an all-False mask
            if (idx_c > stop_idx) idx_c = stop_idx;
            if (idx_c == 0) idx_c = stop_idx;
            n_decel = idx_c + 1 < n ? idx_c + 1 : n;
            vcs = sqrt(vs.wb[n_decel - 1]);
        } else {
            if (!(stop_idx >= 2)) vb = 0;                                                // :260-261
        }
        // SEGMENT 2 (:267-286): FB profile on [idx_c, stop_idx] capped at v_control
        const int m = (stop_idx + 1 < n ? stop_idx + 1 : n) - idx_c;
        if (stop_idx - idx_c > 0) {
            VelScratch sub = vs;
            sub.w = vs.wc + idx_c; sub.kabs = vs.kabs + idx_c; sub.el = vs.el + idx_c;
            sub.gax = vs.gax ? vs.gax + idx_c : nullptr; sub.gay = vs.gay ? vs.gay + idx_c : nullptr;
            sub.igay = vs.igay ? vs.igay + idx_c : nullptr;
            fb_profile<EM, AXM1, GGARR>(m, sub, cax, cay, p, v_control, vcs, true, v_end, lane);
            if (fabs(sqrt(vs.wc[idx_c]) - vcs) > 1.0) vb = 0;
        } else if (stop_idx - idx_c == 0) {
            if (lane == 0) vs.wc[idx_c] = vcs * vcs;
        }
        // vx_decel[:-1] in front, zeros behind (:289)
        for (int i = lane; i < n; i += 64) {
            if (i < n_decel - 1) vs.wc[i] = vs.wb[i];
            else if (i > stop_idx) vs.wc[i] = 0.0;
        }
        wave_sync_lds();
        if (fabs(sqrt(vs.wc[0]) - fi.v_start) > 1.0) vb = 0;                             // :291-292
    } else {
        for (int i = lane; i < n; i += 64) vs.wc[i] = vs.wb[i];                          // :294
        wave_sync_lds();
    }
    // complete profile (:297-307) and intersection (:310)
    if (skip_free) {                                           // LTPL_VEL_FOLLOW_CONTROLLED: the caller intersects (:297-310)
        for (int i = lane; i < n; i += 64) vs.w[i] = vs.wc[i];
        wave_sync_lds();
        *too_close = tc; *vel_bound = vb;
        return;
    }
    if (ext_sync) __syncthreads();                             // the helper wave has written vs.w
    else fb_profile<EM, AXM1, GGARR>(n, vs, cax, cay, p, v_max, fi.v_start, false, 0.0, lane);
    for (int i = lane; i < n; i += 64) { const double a = vs.wc[i], b = vs.w[i]; vs.w[i] = a < b ? a : b; }
    wave_sync_lds();
    *too_close = tc; *vel_bound = vb;
}

// ---------------------------------------------------------------------------------------------------------------------
// kernels of the velocity seam and the fused tick
// ---------------------------------------------------------------------------------------------------------------------
struct DevVelJob {
    int mode, n, n_el, has_v_end;
    int off_kappa, off_el, off_gg, off_out;       // offsets (in doubles) into the pooled job arrays
    double v_start, v_end, v_ego, v_obj, safety_d, obj_dist, obj_x, obj_y;
    // the car of the job (fleet::VelJob, ABI v6): v_max <= 0 / n_axm == 0 -> the launch's parameter set (seam 2, host planner)
    double v_max;
    int axm_off, n_axm;                           // rows [axm_off, axm_off + n_axm) of the launch's stacked machine tables
    int gg_rows, lane_form;                       // gg_rows 1: off_gg holds n caller-supplied [ax, ay] rows (local_gg as a dict, OTH.py:649-666) instead of two
                                                  // constants; lane_form 1 (fleet): operands in the lane plane, the job belongs to a lane kernel
};

// seam (2): one wave per job. GG = false: the job's friction limits are constant along the path (the fleet's jobs: rows 0 of loc_gg hold
// them) -- three LDS arrays less per wave and no per-point loads of the limits. SEL (fleet): the occupancy of these launches is bound by
// the LDS a wave needs and the recurrences are latency chains (~200 cycles per point), so the fleet runs the forward-backward / brake jobs
// (SEL 1: three arrays, "lite" scratch) and the follow jobs (SEL 2: six arrays, job slot 0 of every planner) as two launches; a block
// whose job belongs to the other launch returns at once. SEL 3 (fleet, calls with location dependent friction): the forward-backward
// jobs whose limits are ROWS (DevVelJob::gg_rows) -- the lane kernel that solves a tick's other forward-backward jobs takes constants only.
// `job_stride`: block b works on job b * job_stride.
template <int EM, bool AXM1, bool GG = true, int SEL = 0>
__global__ __launch_bounds__(64) void k_vel_profile(DevLat lat, DevVelParams p_, const DevVelJob* jobs,
                                                    const double* pool, double* out_pool, int* out_flags, int cap,
                                                    long long* dbg, DoneSignal done, int job_stride)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x;
    dbg_stamp(dbg, 0);
    const int j = blockIdx.x * job_stride;
    const DevVelJob jb = jobs[j];
    if (jb.n <= 0) { signal_done(done); return; }          // unused slot of a fleet's job table (fleet_dev.hpp); seam (2) itself rejects empty jobs
    // the car of the job: its own vel_max / machine table (a fleet of different cars), else the launch's
    DevVelParams p = p_;
    if (jb.v_max > 0.0) p.v_max = jb.v_max;
    if (jb.n_axm > 0) { p.n_axm = jb.n_axm; p.axm = p_.axm + 2 * jb.axm_off; }
    const bool follow = jb.mode == LTPL_VEL_FOLLOW || jb.mode == LTPL_VEL_FOLLOW_CONTROLLED;
    if constexpr (SEL == 1) { if (follow) return; }
    if constexpr (SEL == 2) { if (!follow || jb.lane_form) return; }      // (fleet: follow jobs without friction rows run one lane per job, k_fleet_follow_lanes)
    if constexpr (SEL == 3) { if (follow || !jb.gg_rows) return; }
    constexpr bool LITE = SEL == 1 || SEL == 3;
    VelScratch vs = carve_vel_scratch(smem, cap, GG, false, nullptr, nullptr, LITE);
    vs.dbg = dbg;
    const int n = jb.n;
    for (int i = lane; i < n; i += 64) {
        vs.kabs[i] = fabs(pool[jb.off_kappa + i]);
        if constexpr (GG) {
            vs.gax[i] = pool[jb.off_gg + 2 * i];
            const double ay = pool[jb.off_gg + 2 * i + 1];
            vs.gay[i] = ay; vs.igay[i] = 1.0 / ay;
        }
    }
    const double cax = GG ? 1.0 : pool[jb.off_gg], cay = GG ? 1.0 : pool[jb.off_gg + 1];
    for (int i = lane; i < 2 * p.n_axm; i += 64) vs.axm[i] = p.axm[i];
    for (int i = lane; i < jb.n_el; i += 64) vs.el[i] = pool[jb.off_el + i];
    wave_sync_lds();
    dbg_stamp(dbg, 1);
    int too_close = 0, vel_bound = 1;
    if (jb.mode == LTPL_VEL_FB) {
        fb_profile<EM, AXM1, GG>(n, vs, cax, cay, p, p.v_max, jb.v_start, jb.has_v_end != 0, jb.v_end, lane);
    } else if (jb.mode == LTPL_VEL_BRAKE) {
        brake_profile<EM, GG>(n, vs.w, vs, cax, cay, jb.v_start, p, lane);
    } else if constexpr (!LITE) {
        FollowIn fi; fi.v_start = jb.v_start; fi.v_ego = jb.v_ego; fi.v_obj = jb.v_obj; fi.safety_d = jb.safety_d;
        fi.obj_dist = jb.obj_dist; fi.obj_x = jb.obj_x; fi.obj_y = jb.obj_y;
        follow_profile<EM, AXM1, GG>(lat, n, jb.n_el, vs, cax, cay, p, fi, lane, &too_close, &vel_bound, false,
                                     jb.mode == LTPL_VEL_FOLLOW_CONTROLLED);
    }
    dbg_stamp(dbg, 2);
    for (int i = lane; i < n; i += 64) out_pool[jb.off_out + i] = sqrt(vs.w[i]);
    if (lane == 0) { out_flags[2 * j] = too_close; out_flags[2 * j + 1] = vel_bound; }
    dbg_stamp(dbg, 3);
    signal_done(done);
}

struct DevTickVelIn {
    double gg_ax, gg_ay, safety_d, v_max_offset;
    const double* vel_plan; const double* vel_est; const double* pos_est_x; const double* pos_est_y;
    const double* veh_vel;
};
struct DevTickVelOut { double* vx; double* ax; int* vel_bound; int* too_close; };

// per-primitive velocity stage of OnlineTrajectoryHandler.calc_vel_profile (OTH.py:688-941) on a fresh path:
// cut_index_pos = 0, vel_course empty, no brake prefix (the host rejects vel_plan > v_max + 0.1, for which the
// reference itself fails at OTH.py:919 because the prefix it computes is never merged back)
template <int EM, bool AXM1>
__device__ __forceinline__ void tick_vel_stage(const DevLat& lat, const DevPathsIn& in, const DevPathsOut& out, const WavePath& wp,
                               const VelScratch& vs, const double* px, const double* py, const DevVelParams& p,
                               const DevTickVelIn& vin, const DevTickVelOut& vout, int s, int slot, int lane,
                               bool helper_wave)
{
    // vs.kabs already holds |kappa| (k_tick). helper_wave: another wave computes the unconstrained follow profile into vs.w
    const int n = wp.n_pts;
    const double vel_plan = vin.vel_plan[s];
    const double cax = vin.gg_ax, cay = vin.gg_ay;
    // s = [0, cumsum(el[:-1])] (OTH.py:743), one extra entry for get_s_coord's zero-prefixed cumsum (:777)
    wave_cumsum_seq(vs.el, vs.s, n + 1, lane);
    int too_close = 0, vel_bound = 1;
    bool have_follow = false;
    if (wp.name == LTPL_ACT_FOLLOW) {                                                    // OTH.py:763-830
        FollowIn fi; fi.v_start = vel_plan; fi.v_ego = vin.vel_est[s]; fi.safety_d = vin.safety_d;
        const int ci = out.closest_obj_index[s];
        const int v0 = in.veh_off[s];
        if (ci < 0 || ci >= in.veh_off[s + 1] - v0) {
            fi.obj_dist = 0.0; fi.v_obj = 0.0; fi.obj_x = vin.pos_est_x[s]; fi.obj_y = vin.pos_est_y[s];
        } else {
            const int pp = in.pos_off[v0 + ci];
            fi.obj_x = in.pos_x[pp]; fi.obj_y = in.pos_y[pp]; fi.v_obj = vin.veh_vel[v0 + ci];
            const double s_obj = get_s_coord_dev(n, px, py, 1, vs.s, 1, fi.obj_x, fi.obj_y, false, lane, nullptr);
            const double s_sta = get_s_coord_dev(n, px, py, 1, vs.s, 1, vin.pos_est_x[s], vin.pos_est_y[s], false, lane, nullptr);
            fi.obj_dist = s_obj - s_sta;
        }
        // follow_profile rebuilds vs.s as [0, cumsum(el[:-1])] for n_el = n: identical values
        follow_profile<EM, AXM1, false>(lat, n, n, vs, cax, cay, p, fi, lane, &too_close, &vel_bound, helper_wave);
        have_follow = true;
    }
    if (wp.name != LTPL_ACT_FOLLOW || wp.reduced) {                                      // OTH.py:834-923
        if (have_follow) { for (int i = lane; i < n; i += 64) vs.wb[i] = vs.w[i]; wave_sync_lds(); }
        const int rl = lat.rl_idx[wp.goal_layer];
        int dn = wp.end_node - rl; if (dn < 0) dn = -dn;
        const double raceline_offset = (double)dn * lat.lat_offset;
        double v_end; int v_idx;
        if (wp.reduced) {
            v_end = 0.0;
            const double spl_len = vs.s[n - 1];
            int first = 0x7fffffff;
            for (int i = lane; i < n - 1; i += 64) if (!(vs.s[i + 1] < (spl_len - 5.0))) { first = i; break; }
            const int di = wave_min_i32(first);
            v_idx = ((di == 0x7fffffff) ? 0 : di) + 1;
            if (v_idx == 1 && n > 1) v_idx = n;
        } else {
            v_end = lat.vel_rl[wp.goal_layer];
            const double red = v_end * lat.vel_decrease_lat * raceline_offset;
            v_end -= (red < v_end ? red : v_end);
            v_idx = n;
        }
        if (v_idx > 1) fb_profile<EM, AXM1, false>(v_idx, vs, cax, cay, p, p.v_max, vel_plan, true, v_end, lane);
        else { if (lane == 0) vs.w[0] = 0.0; }
        for (int i = (v_idx > 1 ? v_idx : 1) + lane; i < n; i += 64) vs.w[i] = 0.0;         // OTH.py:901-903
        wave_sync_lds();
        vel_bound = fabs(sqrt(vs.w[0]) - vel_plan) < vin.v_max_offset ? 1 : 0;           // OTH.py:906-911
        if (have_follow && n >= 6) {
            // OTH.py:923 compares ROW 5 of both arrays; only column 5 (vx) can differ, so the whole profile switches
            const bool take_follow = sqrt(vs.wb[5]) < sqrt(vs.w[5]);
            if (take_follow) { for (int i = lane; i < n; i += 64) vs.w[i] = vs.wb[i]; wave_sync_lds(); }
        }
    }
    // finalise (OTH.py:925-941): filt_window == 1 is the identity; ax from neighbouring points, -5 at standstill
    double* o_vx = vout.vx + (size_t)slot * out.cap_pts;
    double* o_ax = vout.ax + (size_t)slot * out.cap_pts;
    for (int i = lane; i < n; i += 64) {
        const double wi = vs.w[i];
        const double v = sqrt(wi);
        o_vx[i] = v;
        double a = 0.0;
        if (i < n - 1) {
            a = (vs.w[i + 1] - wi) / (2.0 * (vs.s[i + 1] - vs.s[i]));
            if (fabs(v) <= 1e-8 && fabs(a) <= 1e-8) a = -5.0;
        }
        o_ax[i] = a;
    }
    if (lane == 0) { vout.vel_bound[slot] = vel_bound; vout.too_close[slot] = too_close; }
}
