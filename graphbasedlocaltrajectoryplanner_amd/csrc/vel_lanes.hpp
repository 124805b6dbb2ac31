// vel_lanes.hpp -- the throughput form of the velocity stage, ONE LANE PER PROFILE over tiled planes in HBM (VelPlanes): k_vel_lanes,
// k_vel_final, k_follow_prep, and the compact trajectory export (k_compact_offsets, k_compact_rows). Included by ltpl_hip.hip behind the
// fused and the persistent tick kernels (needs vel_wave.hpp).
#pragma once
// ---------------------------------------------------------------------------------------------------------------------
// throughput form of the velocity stage: ONE LANE PER PROFILE
// ---------------------------------------------------------------------------------------------------------------------
// The recurrences are sequential per profile, so a wave that owns a single profile runs them with 1/64 of its lanes.
// For batches the velocity stage therefore runs as its own kernel in which every lane of a wave64 integrates its own
// profile: 64 independent dependent-chains per instruction stream. All per-row data a lane touches lives in TILED
// planes: element (slot, row) at ((slot / 64) * cap_pts + row) * 64 + slot % 64, so that the 64 lanes of a wave
// (64 consecutive slots) read / write row i as ONE coalesced 512-byte line. The path kernel writes |kappa| and the
// element lengths of every path into two such planes.
//   job type 0 (one lane per action slot):  'follow' -> the controlled profile (ego brake, opponent stop distance, segment
//            forward-backward profile; calc_vel_profile_follow.py:151-294); other primitives -> the generic
//            forward-backward profile with the race-line end velocity (OTH.py:834-903)
//   job type 1 (one lane per scenario):     the unconstrained profile of a 'follow' slot (calc_vel_profile_follow.py:297-307)
//            -- independent of type 0, so the two halves of the follow mode run on different lanes
// k_vel_final (lane per slot, no recurrence) intersects / selects the profiles, derives ax and writes the outputs.
struct DevVelPrep {             // per-slot scalars produced by k_follow_prep (follow action only)
    double* obj_dist; double* v_obj; double* obj_x; double* obj_y; int* idx_s_opp;
};

struct VelPlanes {              // tiled planes (doubles), tile index = job index: generic jobs [0, n_slots_pad), follow jobs behind
    ke_t* KE;                   // (|kappa|, element length) as an fp64 pair: ONE 16-byte load per row and lane   n_slots_pad + n_scen_pad tiles
    double* P0;                 // type 0 result: follow -> "vx_profile" (:289/:294), else the generic profile     (same size)
    double* P1;                 // type 1 result: unconstrained profile of a follow job                n_scen_pad tiles
    double* P2;                 // ego brake profile (follow)                                           n_scen_pad tiles
    double* P3;                 // segment profile (follow), afterwards the generic profile of a reduced-horizon follow job
    double* XY;                 // (x, y) pairs of the follow jobs' path points (written by the path kernel)   n_scen_pad tiles x 2
    int* flags;                 // per tile: VF_* bits
    int* fseg;                  // per follow job [2]: n_decel (-1: everything from the brake profile), stop_idx -- composition of
                                // "vx_profile" (:289 / :294) from P2 / P3 / zeros, done by k_vel_final (VF_COMPOSE)
    int cap_pts;
    int plane_rows;             // rows of the blocked planes KE / XY (kep_base / kep_row, paths_team.hpp)
};

__device__ __forceinline__ size_t tile_base(int idx, int cap_pts) { return ((size_t)(idx >> 6) * cap_pts) * 64 + (idx & 63); }

struct LaneProf {
    const ke_t* KE;                       // tile-strided: element i at [i * 64]
};

// a / b with the hardware reciprocal and two Newton steps (~1 ulp; the rows it produces are limit speeds, checked against the long-double
// reference at 3e-10 .. 5e-10 relative -- tests/vel_cases.py BOUNDS, class "regular" -- where one step fewer leaves 1e-15, none 2e-8). b = 0
// yields NaN, which the callers' `!(w < vmax2)` clamp treats like +inf.
__device__ __forceinline__ double fast_div(double a, double b)
{
    double r = __builtin_amdgcn_rcp(b);
    r = fma(fma(-b, r, 1.0), r, r);
    r = fma(fma(-b, r, 1.0), r, r);
    return a * r;
}

// Issue priority of the velocity kernels' waves (s_setprio 0 .. 3) inside a SIMD they share with path waves. EXPERIMENT (round 5, -DLTPL_VEL_PRIO=<n>):
// a velocity wave blocks the slot of a fourth path wave for as long as it lives; with a higher priority it issues whenever it is ready and
// lives shorter. Default 0 = off (the A/B is in DESIGN.md section 9).
#ifndef LTPL_VEL_PRIO
#define LTPL_VEL_PRIO 0
#endif
#define LTPL_VEL_SETPRIO() do { if (LTPL_VEL_PRIO > 0) __builtin_amdgcn_s_setprio(LTPL_VEL_PRIO); } while (0)
#define LCH 8      // rows per register chunk: all loads of a chunk are issued before the chunk's recurrence steps
#ifndef LCHF
#define LCHF 16    // forward sweep of lane_fb_profile: one 8-byte (|kappa|, el) load per row -> 16 rows per chunk in 32 registers
#endif
#ifndef LCHA
#define LCHA 16    // affine case, forward sweep: rows per register chunk
#endif
#ifndef LCHB
#define LCHB 12    // backward sweep: (|kappa|, el) + the fp64 profile state per row
#endif

// DIRECT OUTPUT OF THE GENERIC PROFILES (round 5). The rows of a generic job (every non-follow primitive) used to take a detour: the
// backward sweep rewrote the plane, k_vel_final read plane and element lengths again, took the root, differentiated and wrote vx / ax.
// Now the backward sweep of lane_fb_profile<.., EMIT = true> produces vx / ax of the rows it finalises (row r: v = sqrt(w_r),
// a = (w_r+1 - w_r) / (2 e_r), -5 at standstill, OTH.py:925-941 -- the operations of k_vel_final) and hands a chunk of LCHB rows per lane to
// lane_emit_flush, which transposes through LDS exactly like k_vel_final: lane = job writes its rows, lane = (job of a group of 8, pair of
// rows) stores 16 contiguous bytes of the slot's output row. The sweep runs wave-uniformly in this mode (all 64 lanes take part in every
// flush, lanes that have no rows left contribute none). k_vel_final only serves the follow jobs (compositions, intersections, row-5 choice).
struct LaneEmit {
    double* tbuf;                  // LDS [32 * LE_PITCH]
    int* s_cnt; int* s_rhi;        // LDS [64]: rows of the job's chunk, row of its first value (values run DOWNWARDS from there)
    unsigned long long* s_o;       // LDS [64]: vx row base of every lane's job (0: idle lane), written by the caller
    long long ax_delta;            // vout.ax - vout.vx in doubles: the ax row of a job lies at the same offset of the other array
    double w0;                     // out: v^2 of row 0 after the backward sweep
};
#define LE_PITCH (LCHB + 2)        // doubles per job row in LDS (16-byte aligned pairs); the buffer is sized for the longest chunk
#ifndef LCHC
#define LCHC 8                     // rows per chunk of the CAPPED backward sweep (follow jobs, round 6): three operands per row -- (|kappa|, el), the forward
                                   // value, the cap -- double-buffered next to the chunk's outputs: 8 rows keep the kernel at 256 registers
#endif
template <int NCH>
__device__ __forceinline__ void lane_emit_flush(const LaneEmit& E, int lane, int cnt, int r_hi, const double (&vv)[NCH], const double (&aa)[NCH])
{
    static_assert(NCH % 2 == 0 && NCH <= 16 && NCH <= LCHB, "pairs of rows, eight pieces per job, the LDS buffer of the longest chunk");
    constexpr int PITCH = NCH + 2;
    E.s_cnt[lane] = cnt; E.s_rhi[lane] = r_hi;
    const int q = lane >> 3, piece = lane & 7;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int half = pass & 1;                                      // jobs [32 half, 32 half + 32); passes 0, 1: vx, 2, 3: ax
        if ((lane >> 5) == half) {
#pragma unroll
            for (int c = 0; c < NCH; c += 2) store2(&E.tbuf[(lane & 31) * PITCH + c], pass < 2 ? vv[c] : aa[c], pass < 2 ? vv[c + 1] : aa[c + 1]);
        }
        wave_sync_lds();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int jl = k * 8 + q, jj = half * 32 + jl, c = 2 * piece;
            const int cn = E.s_cnt[jj];
            if (c >= cn || c >= NCH) continue;
            const dbl2 v = *reinterpret_cast<const dbl2*>(&E.tbuf[jl * PITCH + c]);     // rows r - c (x) and r - c - 1 (y)
            double* o = reinterpret_cast<double*>(E.s_o[jj]) + (pass < 2 ? 0 : E.ax_delta) + (E.s_rhi[jj] - c);
            if (c + 1 < cn) store2_u(o - 1, v.y, v.x); else o[0] = v.x;
        }
        wave_sync_lds();
    }
}

// tph.calc_vel_profile(closed=False) for one lane: rows [off, off + n) of the path, result into plane D (as v^2).
// Rows are processed in register chunks of LCH; the rows of the NEXT chunk are requested before the current chunk's recurrence
// steps run (double buffer). Two things keep the compiler's s_waitcnt placement tight (measured: a per-step vmcnt(0) -- i.e. a
// full store acknowledgement per row -- made the kernel 8x slower than its instruction count):
//   * the function is force-inlined into the kernel, so the planes are addressed with GLOBAL instructions (an out-of-line copy
//     takes them by reference as generic pointers -> FLAT loads / stores, which always wait on vmcnt(0) and lgkmcnt(0));
//   * a recurrence step is branch-free (selects instead of `if (active)`), so a chunk is one basic block and the waits are
//     counted exactly: the stores of a chunk stay in flight while the next chunk's operands are awaited.
// What the EMIT form puts out per finalised row: the profile's own v^2 (NoCap: the generic jobs), or -- FollowCap, round 6 -- the MINIMUM of it and
// the row of the follow job's "vx_profile" (calc_vel_profile_follow.py:289 / :294: ego brake profile P2 in front of row n_decel - 1, segment
// profile P3 up to stop_idx, zeros behind), i.e. what k_vel_final composed from four planes for every follow job: the unconstrained profile's
// backward sweep now finalises the follow job's rows itself and k_vel_final only serves the (rare) reduced-horizon follow jobs.
struct NoCap { static constexpr bool active = false; __device__ __forceinline__ double at(int) const { return INFINITY; } };
struct FollowCap {
    static constexpr bool active = true;
    const double* P2; const double* P3; int nd, stop_idx;          // nd < 0: every row from the brake profile
    __device__ __forceinline__ double at(int r) const
    {
        const bool from_b = nd < 0 || r < nd - 1;
        const double* src = from_b ? P2 : P3;
        const double v = src[(size_t)r * 64];
        return (!from_b && r > stop_idx) ? 0.0 : v;
    }
};

template <int EM, bool AXM1, bool EMIT = false, class CAP = NoCap>
__device__ __forceinline__ void lane_fb_profile(const LaneProf& L, double* D, int off, int n, double cax, double cay,
                                                const DevVelParams& p, const double* axm_tab, double v_max, double v_start,
                                                bool has_v_end, double v_end, long long* dbg = nullptr, int drow = -1, LaneEmit* em = nullptr, int lane = 0,
                                                const CAP& cap = CAP())
{
    if (v_start < 0.0) v_start = 0.0;
    if (has_v_end && v_end < 0.0) v_end = 0.0;
    const double vmax2 = v_max * v_max, icay = 1.0 / cay, axm1 = axm_tab[1], dm = p.drag_m, axa = fabs(cax);
    const double vend2 = has_v_end ? v_end * v_end : INFINITY;
    const ke_t* KEb = L.KE;                         // row r of this profile: KEb[kep_row(off + r)]
#define KE_AT(r) KEb[kep_row(off + (r))]
    double* Dp = D + (size_t)off * 64;
    const ke_t rec0 = KE_AT(0);
    double kabs_i = (double)rec0.x, e_i = (double)rec0.y;
    double wi = fmin(cay * ke_rcp(rec0), vmax2);
    if (wi > v_start * v_start) wi = v_start * v_start;
    Dp[0] = wi;
    if constexpr (!EMIT) { if (n < 2) return; }
    do {                                   // (EMIT: a lane without a profile -- n < 2 -- skips the forward sweep but takes part in the flushes below)
    if constexpr (EMIT) { if (n < 2) break; }
    // ---- lateral-limit speed + forward sweep (accel_forw) in one pass -------------------------------------------------
    if constexpr (EM == 1 && AXM1) {
        // Affine case (exponent 1, one-row machine table). A velocity wave is alone on its SIMD and issues one instruction every
        // ~13 cycles whether or not it depends on the previous one (measured: 610 cycles per row for ~50 instructions; splitting
        // a chunk into independent coefficient work and a short dependent chain changed nothing), so the step is written for
        // the smallest instruction COUNT:  w' = max(A0 w + te min(max(axa - g w, 0), axm), 0)  with te = 2 e, A0 = 1 - te dm,
        // g = axa |kappa| / ay  -- algebraically the reference's min(tyre, machine) - drag step; the limit speed comes from the
        // fp32 hardware reciprocal of |kappa| (no fp64 division), full chunks run without the `valid` selects (the partial chunk at the end has them).
        constexpr int CA = CAP::active ? LCHC : LCHA;             // rows per register chunk (the capped form carries more state through the sweeps)
        const double axg = axa * icay;
        double orig_p = wi, g_p = kabs_i * axg, e_p = e_i;      // operands of the row in front of the current step
        bool active = false, prev_acc = false;
        ke_t kr[CA], kn[CA];
        const int nst = n - 1;
#pragma unroll
        for (int c = 0; c < CA; ++c) { const int r = 1 + c < n ? 1 + c : n - 1; kr[c] = KE_AT(r); }
        auto step = [&](const ke_t& rec, int i, bool valid) {
            const double w0n = fmin(cay * ke_rcp(rec), vmax2);    // inf on straights
            const bool acc = w0n > orig_p;
            const bool act = active || (acc && !prev_acc);
            const double te = e_p + e_p;
            const double u = fmin(fmax(fma(-g_p, wi, axa), 0.0), axm1);
            const double wn = fmax(fma(te, u, fma(-(te * dm), wi, wi)), 0.0);
            const double wnext = (act && wn < w0n) ? wn : w0n;
            if (valid) {
                Dp[(size_t)(i + 1) * 64] = wnext;
                active = act && !(wn > vmax2); prev_acc = acc;
                wi = wnext; orig_p = w0n; g_p = (double)rec.x * axg; e_p = (double)rec.y;
            }
        };
        int base = 0;
        for (; base + CA <= nst; base += CA) {
#pragma unroll
            for (int c = 0; c < CA; ++c) {                   // operands of the next chunk (clamped rows: harmless re-reads at the end)
                const int r = base + CA + 1 + c < n ? base + CA + 1 + c : n - 1;
                kn[c] = KE_AT(r);
            }
#pragma unroll
            for (int c = 0; c < CA; ++c) step(kr[c], base + c, true);
#pragma unroll
            for (int c = 0; c < CA; ++c) kr[c] = kn[c];
        }
        if (base < nst) {
#pragma unroll
            for (int c = 0; c < CA; ++c) step(kr[c], base + c, base + c < nst);
        }
        if (wi > vend2) { wi = vend2; Dp[(size_t)(n - 1) * 64] = wi; }            // the end-velocity clamp of the last step
        kabs_i = (double)KE_AT(n - 1).x;                             // |kappa| of the last row (start of the backward sweep)
    } else {
        double orig_i = wi;
        bool active = false, prev_acc = false;
        ke_t kr[LCHF], kn[LCHF];
#pragma unroll
        for (int c = 0; c < LCHF; ++c) { const int r = 1 + c < n ? 1 + c : n - 1; kr[c] = KE_AT(r); }
        for (int base = 0; base < n - 1; base += LCHF) {
#pragma unroll
            for (int c = 0; c < LCHF; ++c) {                   // operands of the next chunk (clamped rows: harmless re-reads at the end)
                const int r = base + LCHF + 1 + c < n ? base + LCHF + 1 + c : n - 1;
                kn[c] = KE_AT(r);
            }
#pragma unroll
            for (int c = 0; c < LCHF; ++c) {
                const int i = base + c;
                const bool valid = i < n - 1;
                const double k_c = (double)kr[c].x, e_c = (double)kr[c].y;
                double w0n = fast_div(cay, k_c);
                w0n = (w0n < vmax2) ? w0n : vmax2;
                const bool acc = w0n - orig_i > 0.0;
                const bool act = active || (acc && !prev_acc);
                const double kq_i = kabs_i * icay;
                double wn;
                if constexpr (EM == 1 && AXM1) {
                    const double te = 2.0 * e_i;
                    const double A0 = 1.0 - te * dm, A1 = A0 - te * (axa * kq_i), B1 = te * axa, B2 = te * axm1;
                    wn = fmax(fmin(fmax(fma(A1, wi, B1), A0 * wi), fma(A0, wi, B2)), 0.0);
                } else {
                    const double a = ax_poss_w<EM, AXM1, VMODE_ACCEL_FORW>(wi, kq_i, cax, p, axm_tab, axm1);
                    wn = fmax(wi + 2.0 * a * e_i, 0.0);
                }
                double wnext = (act && wn < w0n) ? wn : w0n;
                const bool act_out = act && !(wn > vmax2);
                wnext = (i + 1 == n - 1 && wnext > vend2) ? vend2 : wnext;
                if (valid) Dp[(size_t)(i + 1) * 64] = wnext;
                active = valid ? act_out : active; prev_acc = valid ? acc : prev_acc;
                orig_i = valid ? w0n : orig_i; wi = valid ? wnext : wi; kabs_i = valid ? k_c : kabs_i; e_i = valid ? e_c : e_i;
            }
#pragma unroll
            for (int c = 0; c < LCHF; ++c) kr[c] = kn[c];
        }
    }
    } while (0);
    vl_stamp(dbg, drow, 8);
    // ---- backward sweep (decel_backw), mirrored indices; with a constant gg the unmirrored-gg quirk is void --------------
    if constexpr (EMIT) {
        // wave-uniform form with direct output (see LaneEmit): every lane walks the chunks of the LONGEST profile of the wave, its own steps
        // masked by `valid`; the plane is only read (forward values), vx / ax of the finalised rows go out through lane_emit_flush
        constexpr int CB = CAP::active ? LCHC : LCHB;             // rows per chunk
        const int nst = n >= 2 ? n - 1 : 0;
        const double axg = axa * icay;
        double orig_p = wi, g_p = kabs_i * axg;                       // affine form: operands of the row above
        double orig_i = wi;                                           // general form
        bool active = false, prev_acc = false;
        ke_t kr[CB], kn[CB]; double wr[CB], wq[CB];
        [[maybe_unused]] double cr[CB], cq[CB];                   // CAP: the cap's rows of the current / the next chunk
        [[maybe_unused]] double fprev = 0.0;                          // CAP: the value put out for the row above
        if constexpr (CAP::active) { if (n >= 1) fprev = fmin(cap.at(n - 1), wi); }
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            const int r = n - 2 - c >= 0 ? n - 2 - c : 0;
            kr[c] = KE_AT(r); wr[c] = Dp[(size_t)r * 64];
            if constexpr (CAP::active) cr[c] = cap.at(r);
        }
        for (int base = 0; __ballot(base < nst) != 0ull; base += CB) {
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                const int r = n - 2 - base - CB - c >= 0 ? n - 2 - base - CB - c : 0;
                kn[c] = KE_AT(r); wq[c] = Dp[(size_t)r * 64];
                if constexpr (CAP::active) cq[c] = cap.at(r);
            }
            double vv[CB], aa[CB];
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                const bool valid = base + c < nst;
                const double wold = wr[c], e_b = (double)kr[c].y, k_c = (double)kr[c].x;
                double wn; bool acc;
                if constexpr (EM == 1 && AXM1) {
                    acc = wold > orig_p;
                    const double te = 2.0 * e_b, tdm = te * dm, g_n = k_c * axg;
                    const double w1 = fmax(fma(te, fmax(fma(-g_p, wi, axa), 0.0), fma(tdm, wi, wi)), 0.0);
                    wn = fmin(fmax(fma(te, fmax(fma(-g_n, w1, axa), 0.0), fma(tdm, w1, wi)), 0.0), w1);
                } else {
                    acc = wold - orig_i > 0.0;
                    const double kq_i = kabs_i * icay, kq_n = k_c * icay;
                    const double a = ax_poss_w<EM, AXM1, VMODE_DECEL_BACKW>(wi, kq_i, cax, p, axm_tab, axm1);
                    wn = fmax(wi + 2.0 * a * e_b, 0.0);
                    const double a2 = ax_poss_w<EM, AXM1, VMODE_DECEL_BACKW>(wn, kq_n, cax, p, axm_tab, axm1);
                    wn = fmin(fmax(wi + 2.0 * a2 * e_b, 0.0), wn);
                }
                const bool act = active || (acc && !prev_acc);
                const double wnext = (act && wn < wold) ? wn : wold;
                double v = 0.0, a_out = 0.0;
                if (valid) {
                    if constexpr (CAP::active) {
                        const double f = fmin(cr[c], wnext);           // the follow job's row: min("vx_profile", unconstrained profile)
                        v = sqrt(f);
                        a_out = (fprev - f) / (2.0 * e_b);
                        fprev = f;
                    } else {
                        v = sqrt(wnext);
                        a_out = (wi - wnext) / (2.0 * e_b);            // (w_r+1 - w_r) / (2 e_r): the row above is the state before this step
                    }
                    if (fabs(v) <= 1e-8 && fabs(a_out) <= 1e-8) a_out = -5.0;
                    active = act && !(wn > vmax2); prev_acc = acc;
                    wi = wnext; orig_p = wold; orig_i = wold; g_p = k_c * axg; kabs_i = k_c;
                }
                vv[c] = v; aa[c] = a_out;
            }
            const int left = nst - base;
            lane_emit_flush(*em, lane, left < 0 ? 0 : (left < CB ? left : CB), n - 2 - base, vv, aa);
#pragma unroll
            for (int c = 0; c < CB; ++c) { kr[c] = kn[c]; wr[c] = wq[c]; if constexpr (CAP::active) cr[c] = cq[c]; }
        }
        em->w0 = wi;
    } else if constexpr (EM == 1 && AXM1) {
        // same form: w1 = max(A0 w + te max(axa - g_i w, 0), 0), w' = min(max(te dm w1 + w + te max(axa - g_n w1, 0), 0), w1),
        // A0 = 1 + te dm (no machine limit under braking)
        const double axg = axa * icay;
        double orig_p = wi, g_p = kabs_i * axg;
        bool active = false, prev_acc = false;
        ke_t kr[LCHB], kn[LCHB]; double wr[LCHB], wq[LCHB];
        const int nst = n - 1;
#pragma unroll
        for (int c = 0; c < LCHB; ++c) {
            const int r = n - 2 - c >= 0 ? n - 2 - c : 0;
            kr[c] = KE_AT(r); wr[c] = Dp[(size_t)r * 64];
        }
        auto step = [&](const ke_t& rec, double wold, int i, bool valid) {
            const bool acc = wold > orig_p;
            const bool act = active || (acc && !prev_acc);
            const double te = 2.0 * (double)rec.y, tdm = te * dm, g_n = (double)rec.x * axg;
            const double w1 = fmax(fma(te, fmax(fma(-g_p, wi, axa), 0.0), fma(tdm, wi, wi)), 0.0);
            const double wn = fmin(fmax(fma(te, fmax(fma(-g_n, w1, axa), 0.0), fma(tdm, w1, wi)), 0.0), w1);
            const bool take = act && wn < wold;
            const double wnext = take ? wn : wold;
            if (valid) {
                // only rows the sweep lowers are rewritten: an unconditional store per row made the sweep 1.5x slower (gfx9 counts
                // loads and stores in ONE in-order vmcnt, so every wait for prefetched rows also waits for the older stores)
                if (take) Dp[(size_t)(n - 2 - i) * 64] = wn;
                active = act && !(wn > vmax2); prev_acc = acc;
                wi = wnext; orig_p = wold; g_p = g_n;
            }
        };
        int base = 0;
        for (; base + LCHB <= nst; base += LCHB) {
            // rows of the next chunk are not written by this chunk's steps (a step only rewrites its own row n - 2 - i)
#pragma unroll
            for (int c = 0; c < LCHB; ++c) {
                const int r = n - 2 - base - LCHB - c >= 0 ? n - 2 - base - LCHB - c : 0;
                kn[c] = KE_AT(r); wq[c] = Dp[(size_t)r * 64];
            }
#pragma unroll
            for (int c = 0; c < LCHB; ++c) step(kr[c], wr[c], base + c, true);
#pragma unroll
            for (int c = 0; c < LCHB; ++c) { kr[c] = kn[c]; wr[c] = wq[c]; }
        }
        if (base < nst) {
#pragma unroll
            for (int c = 0; c < LCHB; ++c) step(kr[c], wr[c], base + c, base + c < nst);
        }
    } else {
        double orig_i = wi;
        bool active = false, prev_acc = false;
        ke_t kr[LCHB], kn[LCHB]; double wr[LCHB], wq[LCHB];
#pragma unroll
        for (int c = 0; c < LCHB; ++c) {
            const int r = n - 2 - c >= 0 ? n - 2 - c : 0;
            kr[c] = KE_AT(r); wr[c] = Dp[(size_t)r * 64];
        }
        for (int base = 0; base < n - 1; base += LCHB) {
            // rows of the next chunk are not written by this chunk's steps (a step only rewrites its own row n - 2 - i)
#pragma unroll
            for (int c = 0; c < LCHB; ++c) {
                const int r = n - 2 - base - LCHB - c >= 0 ? n - 2 - base - LCHB - c : 0;
                kn[c] = KE_AT(r); wq[c] = Dp[(size_t)r * 64];
            }
#pragma unroll
            for (int c = 0; c < LCHB; ++c) {
                const int i = base + c;
                const bool valid = i < n - 1;
                const double wold = wr[c], e_b = (double)kr[c].y, k_c = (double)kr[c].x;
                const bool acc = wold - orig_i > 0.0;
                const bool act = active || (acc && !prev_acc);
                const double kq_i = kabs_i * icay, kq_n = k_c * icay;
                double wn;
                if constexpr (EM == 1 && AXM1) {
                    const double te = 2.0 * e_b;
                    const double A0 = 1.0 + te * dm, A1 = A0 - te * (axa * kq_i), B1 = te * axa;
                    const double C0 = te * dm, C1 = C0 - te * (axa * kq_n), D1 = te * axa;
                    wn = fmax(fmax(fma(A1, wi, B1), A0 * wi), 0.0);
                    const double t0 = fma(C0, wn, wi), t1 = fma(C1, wn, wi + D1);
                    wn = fmin(fmax(fmax(t1, t0), 0.0), wn);
                } else {
                    const double a = ax_poss_w<EM, AXM1, VMODE_DECEL_BACKW>(wi, kq_i, cax, p, axm_tab, axm1);
                    wn = fmax(wi + 2.0 * a * e_b, 0.0);
                    const double a2 = ax_poss_w<EM, AXM1, VMODE_DECEL_BACKW>(wn, kq_n, cax, p, axm_tab, axm1);
                    wn = fmin(fmax(wi + 2.0 * a2 * e_b, 0.0), wn);
                }
                const bool take = act && wn < wold;
                const double wnext = take ? wn : wold;
                if (valid && take) Dp[(size_t)(n - 2 - i) * 64] = wn;
                const bool act_out = act && !(wn > vmax2);
                active = valid ? act_out : active; prev_acc = valid ? acc : prev_acc;
                orig_i = valid ? wold : orig_i; wi = valid ? wnext : wi; kabs_i = valid ? k_c : kabs_i;
            }
#pragma unroll
            for (int c = 0; c < LCHB; ++c) { kr[c] = kn[c]; wr[c] = wq[c]; }
        }
    }
}

#undef KE_AT

#define VF_BOUND_FOLLOW 1
#define VF_TOO_CLOSE    2
#define VF_HAS_GENERIC  4
#define VF_BOUND_GENERIC 8
#define VF_COMPOSE 16
#define VF_DONE 32                 // the lane kernel wrote the slot's vx / ax / flags itself (round 6: follow jobs of batches): nothing left for k_vel_final

// The CONTROLLED part of calc_vel_profile_follow.py:78-294 for one lane (= one follow job): ego brake profile -> plane P2, opponent stop
// distance on the global race line from index idx_s_opp, characteristic indices, segment profile -> plane P3. "vx_profile" (:289 / :294)
// is then: P2 in front of row n_decel - 1 (all rows when !two_seg), P3 up to stop_idx, zeros behind -- composed by the caller. Shared by the
// batch velocity stage (k_vel_lanes) and the fleet's lane kernel of the follow jobs (k_fleet_follow_lanes, round 5).
struct LaneFollowOut { int vel_bound, too_close, two_seg, n_decel, stop_idx; };
template <int EM, bool AXM1>
__device__ __forceinline__ LaneFollowOut lane_follow_controlled(const DevLat& lat, const LaneProf& L, double* P2, double* P3, int n, double cax, double cay,
                                                                const DevVelParams& p, const double* axm_tab, double v_start, double v_ego, double v_obj,
                                                                double obj_dist, double safety_d_in, int idx_s_opp, long long* dbg, int drow)
{
    const double icay = 1.0 / cay;
    int vel_bound = 1;
    const double control_d = p.c_p * safety_d_in + p.len_veh, safety_d = safety_d_in + p.len_veh;
    const int too_close = (obj_dist - safety_d) < 0.0 ? 1 : 0;
    const double v_max = p.v_max;
    double v_control;
    if (p.ctrl == 0) v_control = (v_obj - p.k_p * (control_d - obj_dist) + p.k_d * (v_obj - v_ego));
    else {
        double a = (control_d - obj_dist) * D_PI / 2 * 1 / p.tan_w;
        const double lo = -D_PI / 2 + 1e-5, hi = D_PI / 2 - 1e-5;
        a = a < lo ? lo : (a > hi ? hi : a);
        v_control = (v_obj - tan(a) * p.k_p + p.k_d * (v_obj - v_ego));
    }
    if (v_control < 0.0) v_control = 0.0;
    if (v_control > v_max) v_control = v_max;
    const double wctl = v_control * v_control;

    // opponent brake distance on the global race line (:169-199); rows are gathered in chunks
    const int G = lat.G - 1;
    const double* grl = lat.glob_rl;
    const double vel0 = grl[(size_t)idx_s_opp * 5 + 4];
    double wopp = fmin(v_obj, vel0); wopp *= wopp;
    double opp_stop = 0.0;
    for (int base = 0; base < G && wopp > W_STANDSTILL; base += LCH) {
        double kr[LCH], lr[LCH];
#pragma unroll
        for (int c = 0; c < LCH; ++c) {
            int j = base + c + idx_s_opp; j = j % G;
            kr[c] = fabs(grl[(size_t)j * 5 + 3]); lr[c] = grl[(size_t)(j + 1) * 5] - grl[(size_t)j * 5];
        }
#pragma unroll
        for (int c = 0; c < LCH; ++c) {
            const int k = base + c;
            if (k < G && wopp > W_STANDSTILL) {
                opp_stop += lr[c];
                if (k + 1 >= G) wopp = 0.0;
                else {
                    const double a = ax_poss_w<EM, true, VMODE_DECEL_FORW>(wopp, kr[c] * (1.0 / 14.0), 14.0, p, axm_tab, 0.0);
                    const double r = wopp + 2.0 * a * lr[c];
                    wopp = r < 0.0 ? 0.0 : r;
                }
            }
        }
    }
    vl_stamp(dbg, drow, 1);
    // one pass over the path rows: ego brake profile -> P2 (:152-159), ego stop distance (:162-166), first index at
    // or below the control speed (:254), arc length and stop index (:203-209)
    const double s_stop = obj_dist - safety_d + opp_stop;                            // :206
    double ego_stop = 0.0, s_run = 0.0, s_last = 0.0; int first_le = -1, stop_idx = 0;
    {
        double w = v_start * v_start; bool braking = true, counting = true, searching = true;
        double kr[LCH], er[LCH], kn[LCH], en[LCH];
        auto load_rows = [&](int base, double (&k)[LCH], double (&e)[LCH]) {
#pragma unroll
            for (int c = 0; c < LCH; ++c) {
                const int r = base + c < n ? base + c : n - 1;
                const ke_t ke = L.KE[kep_row(r)]; k[c] = (double)ke.x; e[c] = (double)ke.y;
            }
        };
        load_rows(0, kr, er);
        for (int base = 0; base < n; base += LCH) {
            if (base + LCH < n) load_rows(base + LCH, kn, en);         // next chunk in flight during this chunk's steps
#pragma unroll
            for (int c = 0; c < LCH; ++c) {
                const int i = base + c;
                if (i < n) {
                    const double wv = braking ? w : 0.0;
                    P2[(size_t)i * 64] = wv;
                    if (first_le < 0 && wv <= wctl) first_le = i;
                    if (counting) { if (wv > W_STANDSTILL) ego_stop += er[c]; else counting = false; }
                    if (searching) { if (i < n - 1 && s_run < s_stop) stop_idx = i + 1; else searching = false; }
                    if (i == n - 1) s_last = s_run; // s[n - 1]
                    s_run += er[c];                 // s[i + 1]
                    if (braking && i + 1 < n) {
                        const double kq = kr[c] * icay, e = er[c];
                        double r;
                        if constexpr (EM == 1) {
                            const double te = 2.0 * e, axa = fabs(cax);
                            const double A0 = 1.0 - te * p.drag_m, A1 = A0 + te * (axa * kq);
                            r = fmin(fma(A1, w, -te * axa), A0 * w);
                        } else {
                            r = w + 2.0 * ax_poss_w<EM, true, VMODE_DECEL_FORW>(w, kq, cax, p, axm_tab, 0.0) * e;
                        }
                        if (r < 0.0) braking = false; else w = r;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < LCH; ++c) { kr[c] = kn[c]; er[c] = en[c]; }
        }
    }
    vl_stamp(dbg, drow, 2);
    double v_end = 0.0;
    if (s_stop > s_last) {                                                           // :212-221
        // the stop point lies beyond the path: end velocity = race-line velocity where the opponent's remaining brake
        // distance is used up; the element lengths are fetched LCH at a time (one round trip per chunk, not per step)
        const double s_ends = opp_stop - (s_stop - s_last);
        int idx = 0; double summed = 0.0; bool run = summed < s_ends;
        while (run) {
            double dl[LCH];
#pragma unroll
            for (int c = 0; c < LCH; ++c) {
                int j = idx + c + idx_s_opp; j = j % G;
                dl[c] = grl[(size_t)(j + 1) * 5] - grl[(size_t)j * 5];
            }
#pragma unroll
            for (int c = 0; c < LCH; ++c)
                if (run) { if (summed < s_ends && idx < G) { summed += dl[c]; ++idx; } else run = false; }
            if (run && !(summed < s_ends && idx < G)) run = false;
        }
        int j = (idx % G) + idx_s_opp; if (j >= G) j -= G;
        v_end = grl[(size_t)j * 5 + 4];
    }
    vl_stamp(dbg, drow, 3);
    int idx_c = 0, n_decel = 0; const bool two_seg = ego_stop < s_stop;
    if (two_seg) {                                                                   // :247-292
        double vcs = v_start;
        if (v_start > v_control && stop_idx >= 2) {
            idx_c = first_le < 0 ? 0 : first_le;
            if (idx_c > stop_idx) idx_c = stop_idx;
            if (idx_c == 0) idx_c = stop_idx;
            n_decel = idx_c + 1 < n ? idx_c + 1 : n;
            vcs = sqrt(P2[(size_t)(n_decel - 1) * 64]);
        } else if (!(stop_idx >= 2)) vel_bound = 0;
        const int m = (stop_idx + 1 < n ? stop_idx + 1 : n) - idx_c;
        if (stop_idx - idx_c > 0) {
            lane_fb_profile<EM, AXM1>(L, P3, idx_c, m, cax, cay, p, axm_tab, v_control, vcs, true, v_end);
            if (fabs(sqrt(P3[(size_t)idx_c * 64]) - vcs) > 1.0) vel_bound = 0;
        } else if (stop_idx - idx_c == 0) P3[(size_t)idx_c * 64] = vcs * vcs;
        const double first_v = (n_decel - 1 > 0) ? sqrt(P2[0]) : sqrt(P3[0]);
        if (fabs(first_v - v_start) > 1.0) vel_bound = 0;
    }
    vl_stamp(dbg, drow, 4);
    LaneFollowOut o; o.vel_bound = vel_bound; o.too_close = too_close; o.two_seg = two_seg ? 1 : 0; o.n_decel = n_decel; o.stop_idx = stop_idx;
    return o;
}

// the generic forward-backward profile of a slot (OTH.py:834-903) into plane D; returns its vel_bound flag
template <int EM, bool AXM1>
__device__ __forceinline__ int lane_generic_profile(const DevLat& lat, const DevPathsOut& out, const LaneProf& L, double* D, int slot, int n,
                                    int reduced, double cax, double cay, const DevVelParams& p, const double* axm_tab,
                                    double vel_plan, double v_max_offset)
{
    const int goal = out.goal_layer[slot];
    const int end_node = out.nodes[(size_t)slot * out.cap_nodes + out.n_nodes[slot] - 1];
    int dn = end_node - lat.rl_idx[goal]; if (dn < 0) dn = -dn;
    const double raceline_offset = (double)dn * lat.lat_offset;
    double v_end; int v_idx;
    if (reduced) {
        v_end = 0.0;
        double spl_len = 0.0;
        for (int i = 0; i < n - 1; ++i) spl_len += (double)L.KE[kep_row(i)].y;
        int first = -1; double c = 0.0;
        for (int i = 0; i < n - 1; ++i) { c += (double)L.KE[kep_row(i)].y; if (first < 0 && !(c < (spl_len - 5.0))) first = i; }
        v_idx = (first < 0 ? 0 : first) + 1;
        if (v_idx == 1 && n > 1) v_idx = n;
    } else {
        v_end = lat.vel_rl[goal];
        const double red = v_end * lat.vel_decrease_lat * raceline_offset;
        v_end -= (red < v_end ? red : v_end);
        v_idx = n;
    }
    if (v_idx > 1) lane_fb_profile<EM, AXM1>(L, D, 0, v_idx, cax, cay, p, axm_tab, p.v_max, vel_plan, true, v_end);
    else D[0] = 0.0;
    for (int i = (v_idx > 1 ? v_idx : 1); i < n; ++i) D[(size_t)i * 64] = 0.0;
    return fabs(sqrt(D[0]) - vel_plan) < v_max_offset ? 1 : 0;
}

// The same with DIRECT OUTPUT (LaneEmit): vx / ax of the slot are written from here -- the rows the backward sweep finalises through the
// LDS transposition of lane_emit_flush, the rows it does not own (the profile's last row, the zero tail of a reduced horizon) by the lane
// itself. Called by ALL 64 lanes of the wave (`have` = the lane owns a job); returns the vel_bound flag.
template <int EM, bool AXM1>
__device__ __forceinline__ int lane_generic_profile_emit(const DevLat& lat, const DevPathsOut& out, const LaneProf& L, double* D, bool have, int slot, int n,
                                                         int reduced, double cax, double cay, const DevVelParams& p, const double* axm_tab,
                                                         double vel_plan, double v_max_offset, LaneEmit& E, int lane, double* o_vx)
{
    double v_end = 0.0; int v_idx = 0;
    if (have) {
        const int goal = out.goal_layer[slot];
        const int end_node = out.nodes[(size_t)slot * out.cap_nodes + out.n_nodes[slot] - 1];
        int dn = end_node - lat.rl_idx[goal]; if (dn < 0) dn = -dn;
        const double raceline_offset = (double)dn * lat.lat_offset;
        if (reduced) {
            double spl_len = 0.0;
            for (int i = 0; i < n - 1; ++i) spl_len += (double)L.KE[kep_row(i)].y;
            int first = -1; double c = 0.0;
            for (int i = 0; i < n - 1; ++i) { c += (double)L.KE[kep_row(i)].y; if (first < 0 && !(c < (spl_len - 5.0))) first = i; }
            v_idx = (first < 0 ? 0 : first) + 1;
            if (v_idx == 1 && n > 1) v_idx = n;
        } else {
            v_end = lat.vel_rl[goal];
            const double red = v_end * lat.vel_decrease_lat * raceline_offset;
            v_end -= (red < v_end ? red : v_end);
            v_idx = n;
        }
    }
    const int n_prof = v_idx > 1 ? v_idx : 0;                   // rows of the profile proper (0: the path has none, everything is zero)
    lane_fb_profile<EM, AXM1, true>(L, D, 0, n_prof, cax, cay, p, axm_tab, p.v_max, vel_plan, true, v_end, nullptr, -1, &E, lane);
    if (!have) return 0;
    // rows n_prof - 1 .. n - 1: the profile's last row (its v^2 is in the plane: the backward sweep starts below it) and the zero tail;
    // ax of a row differentiates towards the row above, which is zero (or absent: last row of the path, ax = 0) for all of them
    const double w0 = n_prof >= 2 ? E.w0 : 0.0;
    double* o_ax = o_vx + E.ax_delta;
    for (int i = (n_prof >= 2 ? n_prof - 1 : 0); i < n; ++i) {
        const double w = (n_prof >= 2 && i == n_prof - 1) ? D[(size_t)i * 64] : 0.0;
        const double v = sqrt(w);
        double a = 0.0;
        if (i < n - 1) {
            a = (0.0 - w) / (2.0 * (double)L.KE[kep_row(i)].y);
            if (fabs(v) <= 1e-8 && fabs(a) <= 1e-8) a = -5.0;
        }
        o_vx[i] = v; o_ax[i] = a;
    }
    return fabs(sqrt(w0) - vel_plan) < v_max_offset ? 1 : 0;
}

// amdgpu_waves_per_eu(2): at most 256 registers. A velocity wave shares its SIMD with path waves of 128 registers each (4 x 128 = the whole
// file): one of up to 256 registers waits for TWO of them to retire, one of 257+ for THREE. Same-box A/B of this kernel at 265 registers
// (what the allocator takes when left alone, round 6) against 256 with four values parked in scratch: 38.4 against 40.6 M ticks/s
// (profiles/r06j_ab_follow_emit.txt) -- the footprint of a velocity wave is what the path kernel pays for.
template <int EM, bool AXM1>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_vel_lanes(DevLat lat, DevPathsIn in, DevPathsOut out, DevVelParams p,
                                                  DevTickVelIn vin, DevVelPrep prep, VelPlanes vp, int n_slots, int n_scen,
                                                  int n_blocks0, long long* dbg, DevTickVelOut vout, int emit)
{
    LTPL_VEL_SETPRIO();
    __shared__ __align__(16) double le_tbuf[32 * LE_PITCH];        // direct output of the generic jobs (LaneEmit)
    __shared__ int le_cnt[64], le_rhi[64];
    __shared__ unsigned long long le_o[64];
    // blocks [0, nbG): generic jobs; [nbG, nbG + nbF): follow jobs, controlled part; [nbG + nbF, nbG + 2 nbF): follow jobs,
    // unconstrained profile. Waves beyond the job counters (known only on the device) exit at once.
    __shared__ double axm_tab[128];
    const int lane = threadIdx.x;
    const int nbG = n_blocks0, nbF = (n_scen + 63) / 64;
    const int cntG = out.job_cnt[0], cntF = out.job_cnt[1];
    const int b = blockIdx.x;
    if ((b < nbG && b * 64 >= cntG) || (b >= nbG && ((b - nbG) % nbF) * 64 >= cntF)) return;
    for (int i = lane; i < 2 * p.n_axm; i += 64) axm_tab[i] = p.axm[i];
    __syncthreads();
    const int drow = b < nbG ? (b < 64 ? b : -1) : (b < nbG + nbF ? (b - nbG < 64 ? 64 + b - nbG : -1) : (b - nbG - nbF < 64 ? 128 + b - nbG - nbF : -1));
    vl_stamp(dbg, drow, 0);
    const double cax = vin.gg_ax, cay = vin.gg_ay;
    const int fbase = out.n_slots_pad;
    if (b >= nbG + nbF) {
        // ---- follow jobs, unconstrained profile (calc_vel_profile_follow.py:297-307) -------------------------------------
        const int j = (b - nbG - nbF) * 64 + lane;
        if (j >= cntF) return;
        const int2 js = out.job_slot[fbase + j];
        const int slot = js.x;
        if ((emit & 2) && !out.reduced[slot]) return;                 // (large batches: the follow block below runs this profile itself and puts the job's rows out)
        LaneProf L; L.KE = vp.KE + kep_base(fbase + j, vp.plane_rows);
        lane_fb_profile<EM, AXM1>(L, vp.P1 + tile_base(j, vp.cap_pts), 0, js.y, cax, cay, p, axm_tab, p.v_max,
                                  vin.vel_plan[slot / LTPL_MAX_ACTIONS], false, 0.0, dbg, drow);
        vl_stamp(dbg, drow, 6);
        return;
    }
    const bool emit_generic = (emit & 1) != 0;                       // emit bit 0: generic jobs write their outputs here; bit 1: follow jobs do
    if (b < nbG && emit_generic) {
        // ---- generic jobs (every non-follow primitive, OTH.py:834-941): profile AND outputs, all 64 lanes stay for the output transposition.
        //      Batches only (emit_generic = the launch has >= LTPL_EMIT_MIN_SCEN scenarios): the transposition is ~160 instructions per chunk
        //      of 12 rows on the lane kernel's serial chain -- with a handful of jobs (single ticks on the long-horizon lattice: C5, 1 200
        //      rows) k_vel_final's many short waves do that work faster (measured: +100 us on a 1.5 ms tick) ----
        const int j = b * 64 + lane;
        const bool have = j < cntG;
        const int2 js = have ? out.job_slot[j] : make_int2(0, 0);
        const int slot = js.x, n = have ? js.y : 0;
        {   // longest profile of the launch (k_vel_final skips row chunks beyond it): one atomic per wave
            const int nmax = wave_max_i32(n);
            if (lane == 0) atomicMax(&out.job_cnt[2], nmax);
        }
        LaneProf L; L.KE = vp.KE + kep_base(j, vp.plane_rows);
        double* o_vx = vout.vx + (size_t)slot * out.cap_pts;
        le_o[lane] = have ? (unsigned long long)o_vx : 0ull;
        LaneEmit E; E.tbuf = le_tbuf; E.s_cnt = le_cnt; E.s_rhi = le_rhi; E.s_o = le_o; E.ax_delta = (long long)(vout.ax - vout.vx); E.w0 = 0.0;
        wave_sync_lds();
        const int bound = lane_generic_profile_emit<EM, AXM1>(lat, out, L, vp.P0 + tile_base(j, vp.cap_pts), have, slot, n, have ? out.reduced[slot] : 0,
                                                              cax, cay, p, axm_tab, have ? vin.vel_plan[slot / LTPL_MAX_ACTIONS] : 0.0, vin.v_max_offset, E, lane, o_vx);
        if (have) {
            vout.vel_bound[slot] = bound; vout.too_close[slot] = 0;
            vp.flags[j] = VF_BOUND_FOLLOW | (bound ? VF_BOUND_GENERIC : 0);
        }
        vl_stamp(dbg, drow, 6);
        return;
    }
    if (b >= nbG && (emit & 2)) {
        // ---- follow jobs of LARGE batches (round 6): the controlled part, then the UNCONSTRAINED profile in the same lane, whose backward sweep puts
        //      out min("vx_profile", unconstrained profile) -- the follow job's rows (FollowCap) -- with vx / ax through the same LDS transposition as
        //      the generic jobs. Otherwise the two halves run on two waves and k_vel_final reads four planes per follow job to compose, intersect,
        //      differentiate and transpose: as much wave-time as the lane kernel itself (profiles/r06f_vel_pmc.txt). Same operations on the same
        //      values in the same order: results unchanged bit for bit. Reduced-horizon follow jobs (rare) keep the old route inside this block.
        //      Large batches only (ltpl_handle::follow_emit_min_scen): the lane now runs five sweeps one after the other instead of three next to
        //      two -- neutral on the throughput of 32 768 scenarios per step, 135 against 117 us for a step of 1 024 (profiles/r06z_bench.json).
        const int j = (b - nbG) * 64 + lane;
        const bool have = j < cntF;
        const int tile = fbase + j;                                   // (the planes hold n_scen_pad follow tiles: a lane without a job has one too)
        const int2 js = have ? out.job_slot[tile] : make_int2(0, 0);
        const int slot = js.x, n = have ? js.y : 0;
        {
            const int nmax = wave_max_i32(n);
            if (lane == 0) atomicMax(&out.job_cnt[2], nmax);
        }
        const int s = slot / LTPL_MAX_ACTIONS;
        LaneProf L; L.KE = vp.KE + kep_base(tile, vp.plane_rows);
        double* P2 = vp.P2 + tile_base(j, vp.cap_pts);
        double* P3 = vp.P3 + tile_base(j, vp.cap_pts);
        const double vel_plan = have ? vin.vel_plan[s] : 0.0;
        const int reduced = have ? out.reduced[slot] : 0;
        FollowCap cap; cap.P2 = P2; cap.P3 = P3; cap.nd = -1; cap.stop_idx = 0;
        bool direct = false;
        int o_bound = 0, o_close = 0;
        if (have) {
            const LaneFollowOut fo = lane_follow_controlled<EM, AXM1>(lat, L, P2, P3, n, cax, cay, p, axm_tab, vel_plan, vin.vel_est[s], prep.v_obj[slot],
                                                                      prep.obj_dist[slot], vin.safety_d, prep.idx_s_opp[slot], dbg, drow);
            o_bound = fo.vel_bound; o_close = fo.too_close;
            if (!reduced) { direct = true; cap.nd = fo.two_seg ? fo.n_decel : -1; cap.stop_idx = fo.stop_idx; }
            else {
                // reduced horizon: "vx_profile" materialised in P0, the generic profile on top of it in P3 (OTH.py:834-923), k_vel_final chooses by
                // row 5; the unconstrained profile of such a job comes from its own wave below
                double* P0 = vp.P0 + tile_base(tile, vp.cap_pts);
                int flags = VF_BOUND_FOLLOW | VF_HAS_GENERIC;
                if (fo.too_close) flags |= VF_TOO_CLOSE;
                if (!fo.vel_bound) flags &= ~VF_BOUND_FOLLOW;
                const bool two_seg = fo.two_seg != 0;
                for (int i = 0; i < n; ++i) {
                    const bool from_b = !two_seg || i < fo.n_decel - 1;
                    P0[(size_t)i * 64] = from_b ? P2[(size_t)i * 64] : ((i > fo.stop_idx) ? 0.0 : P3[(size_t)i * 64]);
                }
                if (lane_generic_profile<EM, AXM1>(lat, out, L, P3, slot, n, reduced, cax, cay, p, axm_tab, vel_plan, vin.v_max_offset))
                    flags |= VF_BOUND_GENERIC;
                vp.flags[tile] = flags;
            }
        }
        double* o_vx = vout.vx + (size_t)slot * out.cap_pts;
        le_o[lane] = direct ? (unsigned long long)o_vx : 0ull;
        LaneEmit E; E.tbuf = le_tbuf; E.s_cnt = le_cnt; E.s_rhi = le_rhi; E.s_o = le_o; E.ax_delta = (long long)(vout.ax - vout.vx); E.w0 = 0.0;
        wave_sync_lds();
        // (a lane that puts nothing out walks the sweep with zero rows; its one store -- the start value of row 0 -- goes to its brake plane, not to the
        //  unconstrained plane another wave may be writing for a reduced-horizon job)
        double* D = direct ? vp.P1 + tile_base(j, vp.cap_pts) : P2;
        lane_fb_profile<EM, AXM1, true, FollowCap>(L, D, 0, direct && n >= 2 ? n : 0, cax, cay, p, axm_tab, p.v_max, vel_plan, false, 0.0, nullptr, -1, &E, lane, cap);
        if (direct) {
            // the top row: the backward sweep starts below it; its ax differentiates towards nothing (last row of the path)
            const int i = n - 1;
            const double w = fmin(cap.at(i), D[(size_t)i * 64]);
            o_vx[i] = sqrt(w); o_vx[i + E.ax_delta] = 0.0;
            vout.vel_bound[slot] = o_bound; vout.too_close[slot] = o_close;
            vp.flags[tile] = VF_DONE;
        }
        vl_stamp(dbg, drow, 6);
        return;
    }
    const bool fjob = b >= nbG;                                 // (follow jobs, controlled part; generic jobs of small launches: profile into P0, outputs by k_vel_final)
    const int j = (fjob ? b - nbG : b) * 64 + lane;
    if (j >= (fjob ? cntF : cntG)) return;
    const int tile = fjob ? fbase + j : j;
    const int2 js = out.job_slot[tile];
    const int slot = js.x;
    {
        // longest profile of the launch (k_vel_final skips row chunks beyond it): one atomic per wave
        int nmax = js.y;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(nmax, m); nmax = o > nmax ? o : nmax; }   // (lanes beyond the job count have left: no DPP form here)
        if (lane == 0) atomicMax(&out.job_cnt[2], nmax);
    }
    const int s = slot / LTPL_MAX_ACTIONS;
    const int n = js.y;
    LaneProf L; L.KE = vp.KE + kep_base(tile, vp.plane_rows);
    double* P0 = vp.P0 + tile_base(tile, vp.cap_pts);
    double* P2 = vp.P2 + tile_base(fjob ? j : 0, vp.cap_pts);
    double* P3 = vp.P3 + tile_base(fjob ? j : 0, vp.cap_pts);
    const double vel_plan = vin.vel_plan[s];
    const int name = out.action_id[slot], reduced = out.reduced[slot];
    int flags = VF_BOUND_FOLLOW;

    if (name == LTPL_ACT_FOLLOW) {                                                       // OTH.py:763-830
        // calc_vel_profile_follow.py:78-294 for this lane
        const LaneFollowOut fo = lane_follow_controlled<EM, AXM1>(lat, L, P2, P3, n, cax, cay, p, axm_tab, vel_plan, vin.vel_est[s], prep.v_obj[slot],
                                                                  prep.obj_dist[slot], vin.safety_d, prep.idx_s_opp[slot], dbg, drow);
        if (fo.too_close) flags |= VF_TOO_CLOSE;
        int vel_bound = fo.vel_bound;
        const bool two_seg = fo.two_seg != 0; const int n_decel = fo.n_decel, stop_idx = fo.stop_idx;
        // "vx_profile" (:289 / :294) = brake profile in front, segment profile up to the stop index, zeros behind. Normally only
        // described (two indices) and composed by the row-parallel final kernel; a reduced-horizon follow job needs P3 for its
        // generic profile, so there the composition is materialised in P0 here.
        if (!reduced) { vp.fseg[2 * j] = two_seg ? n_decel : -1; vp.fseg[2 * j + 1] = stop_idx; flags |= VF_COMPOSE; }
        else for (int base = 0; base < n; base += LCH) {
            double a[LCH];
#pragma unroll
            for (int c = 0; c < LCH; ++c) {
                const int i = base + c < n ? base + c : n - 1;
                const bool from_b = !two_seg || i < n_decel - 1;
                a[c] = from_b ? P2[(size_t)i * 64] : ((i > stop_idx) ? 0.0 : P3[(size_t)i * 64]);
            }
#pragma unroll
            for (int c = 0; c < LCH; ++c) if (base + c < n) P0[(size_t)(base + c) * 64] = a[c];
        }
        vl_stamp(dbg, drow, 5);
        if (!vel_bound) flags &= ~VF_BOUND_FOLLOW;
        if (reduced) {                                                                   // OTH.py:834-923 on top of follow
            flags |= VF_HAS_GENERIC;
            if (lane_generic_profile<EM, AXM1>(lat, out, L, P3, slot, n, reduced, cax, cay, p, axm_tab, vel_plan, vin.v_max_offset))
                flags |= VF_BOUND_GENERIC;
        }
    } else {
        if (lane_generic_profile<EM, AXM1>(lat, out, L, P0, slot, n, reduced, cax, cay, p, axm_tab, vel_plan, vin.v_max_offset))
            flags |= VF_BOUND_GENERIC;
    }
    vp.flags[tile] = flags;
    vl_stamp(dbg, drow, 6);
}

// final step of the batch velocity stage, no recurrence: intersection of the two follow profiles
// (calc_vel_profile_follow.py:310), choice between follow and generic profile for reduced horizons (OTH.py:923, row 5),
// vx = sqrt(w), ax from neighbouring points with -5 at standstill (OTH.py:925-941). Rows are independent of each other
// (ax_i only needs w_i, w_i+1 and the element length e_i), so the work is spread over (tile of 64 jobs, chunk of FCH rows).
// Two lane mappings in one wave: the planes are tiled by job, so they are READ with lane = job (one coalesced 512-byte line per
// row); the outputs are rows of a slot, so they are WRITTEN with lane = (job, pair of rows) after a transposition through LDS: one
// store instruction covers 8 jobs x 128 contiguous bytes instead of 64 jobs x 16 bytes on 64 different lines (round 2: 122 us ->
// see DESIGN.md section 6; the stores of the lane = job form kept the address units busy, not HBM).
#define FCH 16
#define FPITCH (FCH + 2)           // doubles per job row in LDS (16-byte aligned pairs, odd multiple of 16 bytes: conflict-free b128 access)
__global__ __launch_bounds__(64) void k_vel_final(DevPathsOut out, DevTickVelIn vin, DevTickVelOut vout, VelPlanes vp, int n_slots,
                                                  int n_scen, int first_block)
{
    LTPL_VEL_SETPRIO();
    __shared__ __align__(16) double tbuf[32 * FPITCH];     // 32 jobs at a time: 4.5 KB, so that many blocks fit next to a resident path kernel
    __shared__ int s_slot[64], s_n[64];
    // blocks [0, nbG): generic jobs, [nbG, nbG + nbF): follow jobs; slots without a path were initialised by the path kernel
    // (round 5: launched for the follow tiles only -- first_block = nbG; the generic jobs' outputs come from the lane kernel's backward sweep)
    const int nbG = (n_slots + 63) / 64;
    const int bx = (int)blockIdx.x + first_block;
    const bool fjob = bx >= nbG;
    const int lane = threadIdx.x;
    const int j = (fjob ? bx - nbG : bx) * 64 + lane;
    const int cnt = out.job_cnt[fjob ? 1 : 0];
    if ((j - lane) >= cnt) return;                                      // whole tile without jobs (uniform)
    const bool have = j < cnt;
    const int tile = fjob ? out.n_slots_pad + j : j;
    const int nmax_all = out.job_cnt[2];                                // longest profile of the launch (lane kernel)
    const int2 js = have ? out.job_slot[tile] : make_int2(0, 0);
    const int slot = js.x;
    // (round 6: a follow job of a batch is finished by the lane kernel -- VF_DONE -- unless its horizon is reduced; such a job counts zero rows here,
    //  and a tile without anything left leaves at once)
    const int tflags = have ? vp.flags[tile] : VF_DONE;
    const int n = (tflags & VF_DONE) ? 0 : js.y;
    if (__ballot(n > 0) == 0ull) return;
    s_slot[lane] = slot; s_n[lane] = n;
    // blockIdx.y strides over the row chunks: a few long-lived blocks per tile instead of one block per (tile, chunk), most of
    // which used to find nothing to do
    for (int base = (int)blockIdx.y * FCH; base < nmax_all; base += (int)gridDim.y * FCH) {
    const bool act = have && base < n;
    if (__ballot(act) == 0ull) continue;                                // uniform
    double vv[FCH], aa[FCH];
    if (act) {
        const int flags = tflags;
        const bool follow = fjob;
        const double* P0 = vp.P0 + tile_base(tile, vp.cap_pts);
        const double* P1 = vp.P1 + tile_base(fjob ? j : 0, vp.cap_pts);
        const double* P2 = vp.P2 + tile_base(fjob ? j : 0, vp.cap_pts);
        const double* P3 = vp.P3 + tile_base(fjob ? j : 0, vp.cap_pts);
        const ke_t* KE = vp.KE + kep_base(tile, vp.plane_rows);
        const bool compose = follow && (flags & VF_COMPOSE);
        const int nd = compose ? vp.fseg[2 * j] : 0, stop_idx = compose ? vp.fseg[2 * j + 1] : 0;
        int vel_bound = follow ? ((flags & VF_BOUND_FOLLOW) ? 1 : 0) : ((flags & VF_BOUND_GENERIC) ? 1 : 0);
        int sel = follow ? 1 : 0;                     // 0: P0, 1: min(P0, P1), 2: P3
        if (follow && (flags & VF_HAS_GENERIC)) {
            vel_bound = (flags & VF_BOUND_GENERIC) ? 1 : 0;
            sel = 2;
            if (n >= 6) {
                const double f5 = fmin(P0[5 * 64], P1[5 * 64]);
                if (sqrt(f5) < sqrt(P3[5 * 64])) sel = 1;
            }
        }
        auto value = [&](int i) {
            const size_t o = (size_t)i * 64;
            if (compose) {                                     // sel == 1: min("vx_profile", unconstrained profile)
                const double a = (nd < 0 || i < nd - 1) ? P2[o] : (i > stop_idx ? 0.0 : P3[o]);
                return fmin(a, P1[o]);
            }
            return sel == 0 ? P0[o] : (sel == 1 ? fmin(P0[o], P1[o]) : P3[o]);
        };
        double w[FCH + 1], er[FCH];
#pragma unroll
        for (int c = 0; c <= FCH; ++c) w[c] = value(base + c < n ? base + c : n - 1);
        // element lengths: two rows per 16-byte load (rows 2m, 2m + 1 are adjacent in the blocked plane and `base` is a multiple of 16;
        // rows beyond n - 1 are unused padding of the block -- never NaN-sensitive: their ax is discarded)
#pragma unroll
        for (int c = 0; c < FCH; c += 2) {
#ifndef LTPL_VEL_F32_OPERANDS
            er[c] = KE[kep_row(base + c)].y; er[c + 1] = KE[kep_row(base + c + 1)].y;
#else
            static_assert(KE_RB >= 2, "pairs of rows in one load");
            const float4 v = *reinterpret_cast<const float4*>(&KE[kep_row(base + c)]);
            er[c] = (double)v.y; er[c + 1] = (double)v.w;
#endif
        }
#pragma unroll
        for (int c = 0; c < FCH; ++c) {
            const int i = base + c;
            const double v = sqrt(w[c]);
            double a = 0.0;
            if (i < n - 1) {
                // the reference divides by 2 (s_i+1 - s_i) with s the running sum of the element lengths; e_i differs from that
                // difference by rounding only (~1e-13 relative, tolerance of ax: 1e-5)
                a = (w[c + 1] - w[c]) / (2.0 * er[c]);
                if (fabs(v) <= 1e-8 && fabs(a) <= 1e-8) a = -5.0;
            }
            vv[c] = v; aa[c] = a;
        }
        if (base == 0) { vout.vel_bound[slot] = vel_bound; vout.too_close[slot] = (flags & VF_TOO_CLOSE) ? 1 : 0; }
    } else {
#pragma unroll
        for (int c = 0; c < FCH; ++c) { vv[c] = 0.0; aa[c] = 0.0; }
    }
    // transposition: lane = job writes its FCH values as one LDS row; lane = (job q of a group of 8, pair of rows) reads 16 bytes
    // and stores them to the slot's row (8-byte aligned 16-byte stores; rows of a slot are contiguous)
    const int q = lane >> 3, piece = lane & 7;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int half = pass & 1;                                      // jobs [32 half, 32 half + 32)
        double* dst_base = pass < 2 ? vout.vx : vout.ax;
        if ((lane >> 5) == half) {
#pragma unroll
            for (int c = 0; c < FCH; c += 2) store2(&tbuf[(lane & 31) * FPITCH + c], pass < 2 ? vv[c] : aa[c], pass < 2 ? vv[c + 1] : aa[c + 1]);
        }
        wave_sync_lds();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int jl = k * 8 + q, jj = half * 32 + jl;
            const int nn = s_n[jj], i = base + 2 * piece;
            if (i >= nn) continue;
            const dbl2 v = *reinterpret_cast<const dbl2*>(&tbuf[jl * FPITCH + 2 * piece]);
            double* o = dst_base + (size_t)s_slot[jj] * out.cap_pts + i;
            if (i + 1 < nn) store2_u(o, v.x, v.y); else o[0] = v.x;
        }
        wave_sync_lds();
    }
    }
}

// follow preparation (projection of the object and of the ego position on the path, OTH.py:774-784; projection of the object
// on the global race line, calc_vel_profile_follow.py:172-176), ONE LANE PER FOLLOW JOB like the lane kernel. Round 2 history: the
// wave-per-job form spent ~1 900 instructions per job on cross-lane reductions and half-empty lanes (47 M instructions per
// 32 768-scenario step, 8 % of the path kernel's -- 118 us of the overlapped step); a lane that scans its own job serially needs
// ~190: the race line is read with scalar loads (uniform index), the path points come from a tiled (x, y) plane the path kernel
// writes for follow jobs (coalesced rows), closest point, arc length at the foot point (a running prefix: np.cumsum's order) and
// the element in front of it are picked up in ONE pass for both query points.
#define PCH 8
__global__ __launch_bounds__(64) void k_follow_prep(DevLat lat, DevPathsIn in, DevPathsOut out, DevTickVelIn vin,
                                                    DevVelPrep prep, VelPlanes vp, int n_slots, long long* dbg)
{
    LTPL_VEL_SETPRIO();
    const int lane = threadIdx.x, cnt = out.job_cnt[1];
    if ((int)blockIdx.x * 64 >= cnt) return;
    const int drow = blockIdx.x < 64 ? 192 + (int)blockIdx.x : -1;      // LTPL_DEBUG_TIMING: rows 192 .. 255 of the stamp table
    vl_stamp(dbg, drow, 0);
    const int j0 = (int)blockIdx.x * 64 + lane;
    const bool have_job = j0 < cnt;
    const int j = have_job ? j0 : cnt - 1;                  // idle lanes repeat the last job (uniform control flow), nothing stored
    const int2 js = out.job_slot[out.n_slots_pad + j];
    const int slot = js.x, s = slot / LTPL_MAX_ACTIONS, n = js.y;
    const int ci = out.closest_obj_index[s], v0 = in.veh_off[s];
    const bool have = !(ci < 0 || ci >= in.veh_off[s + 1] - v0);
    const double ex = vin.pos_est_x[s], ey = vin.pos_est_y[s];
    double ox = ex, oy = ey, vobj = 0.0, odist = 0.0;
    if (have) { const int q = in.pos_off[v0 + ci]; ox = in.pos_x[q]; oy = in.pos_y[q]; vobj = vin.veh_vel[v0 + ci]; }
    vl_stamp(dbg, drow, 1);
    const int idx = lane_globrl_index(lat, ox, oy);
    vl_stamp(dbg, drow, 2);
    if (__ballot(have) != 0ull) {
        const double* xy = vp.XY + 2 * kep_base(j, vp.plane_rows);         // pairs: row r of this lane's job at xy + 2 * kep_row(r)
        const ke_t* KE = vp.KE + kep_base(out.n_slots_pad + j, vp.plane_rows);
        int nmax = n;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(nmax, m); nmax = o > nmax ? o : nmax; }   // (lanes beyond the job count have left: no DPP form here)
        // one pass: closest path point of the object (o) and of the ego position (e), arc length in front of it and the element before
        double bo = INFINITY, be = INFINITY, so = 0.0, se = 0.0, po = 0.0, pe = 0.0, run = 0.0, e_prev = 0.0;
        int no = 0, ne = 0;
        dbl2 pr[PCH], pn[PCH]; ke_t kr[PCH], kn[PCH];
        auto load_rows = [&](int base, dbl2 (&p)[PCH], ke_t (&k)[PCH]) {
#pragma unroll
            for (int c = 0; c < PCH; ++c) {
                const int r = base + c < n ? base + c : n - 1;
                p[c] = *reinterpret_cast<const dbl2*>(xy + 2 * kep_row(r)); k[c] = KE[kep_row(r)];
            }
        };
        load_rows(0, pr, kr);
        for (int base = 0; base < nmax; base += PCH) {
            load_rows(base + PCH, pn, kn);
#pragma unroll
            for (int c = 0; c < PCH; ++c) {
                const int i = base + c;
                const bool valid = i < n;
                const double x = pr[c].x, y = pr[c].y, e = (double)kr[c].y;
                const double ao = (x - ox) * (x - ox) + (y - oy) * (y - oy), ae = (x - ex) * (x - ex) + (y - ey) * (y - ey);
                if (valid && ao < bo) { bo = ao; no = i; so = run; po = e_prev; }
                if (valid && ae < be) { be = ae; ne = i; se = run; pe = e_prev; }
                if (valid) { run += e; e_prev = e; }
            }
#pragma unroll
            for (int c = 0; c < PCH; ++c) { pr[c] = pn[c]; kr[c] = kn[c]; }
        }
        vl_stamp(dbg, drow, 3);
        // get_s_coord.py:34-99 (closed = False) for one query: arc length of the foot point
        auto foot = [&](int nb, double s_nb, double e_before, double px, double py) {
            const int i1 = nb - 1 > 0 ? nb - 1 : 0, i2 = nb + 1 < n - 1 ? nb + 1 : n - 1;
            const dbl2 pN = *reinterpret_cast<const dbl2*>(xy + 2 * kep_row(nb)), p1 = *reinterpret_cast<const dbl2*>(xy + 2 * kep_row(i1)),
                       p2 = *reinterpret_cast<const dbl2*>(xy + 2 * kep_row(i2));
            const int ord = angle_order_dev(pN.x, pN.y, px, py, p1.x, p1.y, p2.x, p2.y, i1 == nb, i2 == nb);
            double ax, ay, bx, by;
            if (ord > 0) { ax = p1.x; ay = p1.y; bx = pN.x; by = pN.y; } else { ax = pN.x; ay = pN.y; bx = p2.x; by = p2.y; }
            const double t = ((px - ax) * (bx - ax) + (py - ay) * (by - ay)) / ((bx - ax) * (bx - ax) + (by - ay) * (by - ay));
            const double fx = ax + t * (bx - ax), fy = ay + t * (by - ay);
            const double ds = sqrt((ax - fx) * (ax - fx) + (ay - fy) * (ay - fy));
            return (ord > 0 ? (nb > 0 ? s_nb - e_before : 0.0) : s_nb) + ds;        // s[i1] = s[nb] - el[nb - 1]; s[0] = 0
        };
        const double s_obj = foot(no, so, po, ox, oy), s_sta = foot(ne, se, pe, ex, ey);
        if (have) odist = s_obj - s_sta;
        vl_stamp(dbg, drow, 4);
    }
    if (have_job) { prep.obj_dist[slot] = odist; prep.v_obj[slot] = vobj; prep.obj_x[slot] = ox; prep.obj_y[slot] = oy; prep.idx_s_opp[slot] = idx; }
    vl_stamp(dbg, drow, 5);
}

// ---------------------------------------------------------------------------------------------------------------------
// compact trajectory export (ltpl_tick_batch_compact): rows [s, x, y, psi, kappa, vx, ax] of the valid slots, back to back
// ---------------------------------------------------------------------------------------------------------------------
// rows kept per slot and their exclusive prefix (one block; n_slots <= a few hundred thousand)
__global__ __launch_bounds__(1024) void k_compact_offsets(const int* valid, const int* n_pts, int n_slots, int max_rows,
                                                          int* rows_out, long long* off_out, long long* total)
{
    __shared__ long long part[1024];
    const int t = threadIdx.x, per = (n_slots + 1023) / 1024;
    const int a = t * per, b = a + per < n_slots ? a + per : n_slots;
    long long sum = 0;
    for (int i = a; i < b; ++i) {
        int r = valid[i] ? n_pts[i] : 0;
        if (max_rows > 0 && r > max_rows) r = max_rows;
        rows_out[i] = r; sum += r;
    }
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = part[t] - sum;
    for (int i = a; i < b; ++i) { off_out[i] = run; run += rows_out[i]; }
    if (t == 1023) *total = part[1023];
}

// one wave per slot: s = [0, cumsum(el[:-1])] (OTH.py:743, wave-parallel prefix), then the seven columns of every kept row
__global__ __launch_bounds__(64) void k_compact_rows(DevPathsOut out, DevTickVelOut vout, const int* rows_kept, const long long* off,
                                                     double* dst, long long capacity_rows)
{
    const int slot = blockIdx.x, lane = threadIdx.x;
    const int n = rows_kept[slot];
    if (n <= 0) return;
    const long long o = off[slot];
    if (o + n > capacity_rows) return;
    const double* pp = out.path_param + (size_t)slot * out.cap_pts * 5;
    const double* vx = vout.vx + (size_t)slot * out.cap_pts;
    const double* ax = vout.ax + (size_t)slot * out.cap_pts;
    double carry = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const double e = (i < n) ? pp[(size_t)i * 5 + 4] : 0.0;
        double x = e;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const double y = __shfl_up(x, d); if (lane >= d) x += y; }
        if (i < n) {
            double* r = dst + (size_t)(o + i) * 7;
            r[0] = carry + (x - e);
            r[1] = pp[(size_t)i * 5]; r[2] = pp[(size_t)i * 5 + 1]; r[3] = pp[(size_t)i * 5 + 2]; r[4] = pp[(size_t)i * 5 + 3];
            r[5] = vx[i]; r[6] = ax[i];
        }
        carry += __shfl(x, 63);
    }
}
