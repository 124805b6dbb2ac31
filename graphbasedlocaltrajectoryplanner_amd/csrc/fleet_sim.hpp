// fleet_sim.hpp -- closed-loop simulation of the fleet on the device (ltpl_fleet_sim_*, include/ltpl_hip.h): the example driver's loop
// (main_std_example.py:98-135) around every planner -- opponents on the race line (ObjectlistDummy, objectlist_dummy.py:148-170), object
// ingestion (ObjectListInterface.py:75-153, the device code of ltpl_process_objects), the ideal ego tracker (vdc_dummy.py:5-58) -- in
// front of the fleet's own tick (fleet_dev.hpp), with no host work per tick. Per tick:
//   k_fleet_sim_step     one wave64 per planner: clock, action choice, opponents (one lane each), ingestion (one lane per object, ballot
//                        compaction inside the planner's range), ego tracker (trajectory staged in LDS, two-nearest search across the wave,
//                        the 1 ms loop on lane 0)
//                        and its heading (psi of the two rows around the same s, read in place, interpolated across the +-pi wrap)
//                        With sensor noise set (ltpl_fleet_sim_noise; the generator: fleet_noise.hpp) the tick launches k_fleet_sim_step_noise
//                        and k_fleet_sim_mates_noise instead: the same bodies, every object perturbed in its ingestion lane before
//                        process_object_dev and the planner's pos_est / vel_est written behind the tracker (registers only, no LDS added)
//                        With a vehicle model set (ltpl_fleet_sim_vehicle; the model: fleet_vehicle.hpp) it launches k_fleet_sim_step_veh /
//                        k_fleet_sim_step_noise_veh: the same body with column ax staged as well; a planner with model 1 (wave-uniform)
//                        drives the car instead of the ideal tracker -- every lane runs the 1 ms loop on the same values, the
//                        projection of a control step walks the segments with one lane each and ends in sim_wave_min
//   k_fleet_sim_mates    (races with more than one planner only: ltpl_fleet_sim_race) one wave64 per planner, one lane per mate: every
//                        other planner of the race, at the pose / speed / heading its tracker wrote above, through the same ingestion,
//                        appended behind the planner's opponents and statics. Its own launch: every tracker of the tick is done first
//   k_fleet_sim_tele     (telemetry on only: ltpl_fleet_sim_telemetry) one wave64 per planner: the tracked pose projected on the race line
//                        (get_s_coord_dev, closed), the clearance to every on-track object of the tick (one lane per object, DPP wave
//                        minimum, ties to the lower slot), then lane 0 updates the planner's 22-double record and writes its progress
//   k_fleet_sim_rank     (telemetry on and races with more than one planner) one wave64 per planner, one lane per mate: rank by ballot /
//                        popcount over every mate's progress of this tick, gap to the nearest car ahead by a wave minimum. Its own
//                        launch: every planner's progress of the tick is written first
//   k_fleet_sim_sense    (sensor model set only: ltpl_fleet_sim_sensor; the rule: fleet_sensor.hpp) one wave64 per planner: the geometry of
//                        the tick's on-track objects at their TRUE positions staged in LDS, one lane per object (two passes above 64)
//                        through range, near field, cone, occlusion (every lane walks the same LDS entry: a broadcast) and dropout;
//                        the staged arrays ballot-compacted in place, sd.cnt and trace [5] .. [7] rewritten, lane 0 updates the
//                        planner's 10-double record. Behind telemetry, which measured against the complete list
//   k_fleet_sim_track    (object tracker set only: ltpl_fleet_sim_tracker; the rule: fleet_track.hpp) one wave64 per planner behind the
//                        sensor: the planner's track table predicted, associated with the staged detections (greedy nearest neighbour,
//                        one wave minimum per accepted pair), updated, coasted, compacted and extended by births; the staged arrays,
//                        sd.cnt and trace [5] .. [7] rewritten with the list handed on, lane 0 updates the planner's 12-double record
//   k_fleet_sim_offsets  exclusive scan of the on-track counts -> veh_off (one workgroup)
//   k_fleet_sim_compact  survivors into the fleet's object layout (one lane per planner)
//   k_fleet_sim_predict  (prediction model set only: ltpl_fleet_sim_predictor; the rule: fleet_predict.hpp) in k_fleet_sim_compact's place,
//                        one wave64 per planner: the staged survivors in LDS, per object the nearest race-line row (the wave strides
//                        the rows, one wave minimum over (d2, row)), one lane per object for segment, offset and outcome, one lane per
//                        (object, point) pair for the K points; own position + K points per object into the fleet's object layout
//                        (pos_off[v] = (1 + K) v), lane 0 updates the planner's 11-double record
//   k_fleet_sim_select   (behaviour selector set only: ltpl_fleet_sim_selector; the rule: fleet_select.hpp) at the HEAD of the tick, in front
//                        of k_fleet_sim_step, one wave64 per planner: the previous exported set's rows (x, y, t) of up to four actions and
//                        the previous tick's staged objects in LDS, time columns serially by one lane per action, row x object pairs over
//                        the lanes, one wave minimum per action; the ORDERED preference list into a buffer of the selector's own, which
//                        the step and mates kernels then get as SimDev::pref; lane 0 updates the planner's 12-double record
//   k_fleet_sim_safety   (safety monitor set only: ltpl_fleet_sim_safety; the rule: fleet_safety.hpp) behind k_fleet_sim_tele / k_fleet_sim_rank,
//                        in front of k_fleet_sim_sense, one wave64 per planner: one lane per staged object (blocks of 64), time to
//                        collision, required deceleration, headway, gap and closing speed against the TRUE pose and its displacement
//                        since the previous live tick; wave reductions, lane 0 updates the planner's 31-double record and its incident
//                        ring. Registers only; reads what the tick staged and writes nothing another kernel reads
//   k_fleet_sim_react    (reactive opponents set only: ltpl_fleet_sim_react; the rule: fleet_react.hpp) behind the events kernels and
//                        k_fleet_sim_select, in front of the step kernel, one wave64 per planner: the ego projected onto the race line
//                        (rows strided over the wave, sim_wave_min), s, leader speed and length of the opponents staged in LDS, one lane
//                        per opponent (blocks of 64) with a serial leader scan; the EFFECTIVE vel_scale of every opponent into a buffer of
//                        the model's own, which the step kernels then get as SimDev::opp_scale; lane 0 updates the 16-double record
//   k_fleet_sim_rec_paths / k_fleet_sim_rec_vel   (flight recorder on only: ltpl_fleet_sim_record) one wave64 per RECORDED planner: the
//                        tick's paths behind paths_post, and its head, objects and trajectories behind the last velocity kernel, into
//                        the planner's record of ring slot tick % depth. The tick then takes the unfused launch sequence
//   then paths_pre | path kernel | paths_post (+ vel_a) | velocity stages as in ltpl_fleet_tape_run. Tick k + 1's inputs depend on tick k's
//   trajectories, so the tape's "next paths_pre inside the last kernel" fusion does not apply: paths_pre is launched on its own.
//   k_fleet_sim_stats_chunk / k_fleet_sim_stats_merge   (a statistics plan with a period only: ltpl_fleet_sim_stats; the rule: fleet_stats.hpp)
//                        at the TAIL of every period-th tick, behind every kernel above: one wave64 per (group, chunk of 1024 members)
//                        walks the plan's measures over the planners' records, one wave64 per (group, measure) folds the chunks'
//                        partials into a row of the plan's ring. They read records and write buffers of the plan's own
// The host mirrors of the same arithmetic are graphbasedlocaltrajectoryplanner_amd/sim.py.
#pragma once

#include "fleet_noise.hpp"
#include "fleet_predict.hpp"
#include "fleet_react.hpp"
#include "fleet_safety.hpp"
#include "fleet_select.hpp"
#include "fleet_sensor.hpp"
#include "fleet_stats.hpp"
#include "fleet_track.hpp"
#include "fleet_vehicle.hpp"

namespace fleet {

// np.interp (numpy's arr_interp) for a scalar x on segment j = the largest index with xp[j] <= x (-1 below xp[0]; n - 1 at or above
// xp[n - 1]): clamping at both ends, fp[j] on a knot, slope * (x - xp[j]) + fp[j], the right end of the segment when that is NaN.
// `fp(i)` yields the table value of row i (the opponents' scaled speeds are formed there: vel_rl[i] * vel_scale, objectlist_dummy.py:121).
template <class FP>
__device__ __forceinline__ double sim_interp(double x, const double* xp, int n, int j, FP fp)
{
    if (isnan(x)) return x;
    if (j < 0) return fp(0);
    if (j >= n - 1) return fp(n - 1);
    const double xj = xp[j], f0 = fp(j);
    if (xj == x) return f0;
    const double f1 = fp(j + 1);
    const double slope = (f1 - f0) / (xp[j + 1] - xj);
    double r = slope * (x - xj) + f0;
    if (isnan(r)) {
        r = slope * (x - xp[j + 1]) + f1;
        if (isnan(r) && f0 == f1) r = f0;
    }
    return r;
}
// segment of x by bisection (the same index numpy's binary_search_with_guess finds: the largest j with xp[j] <= x)
__device__ __forceinline__ int sim_segment(double x, const double* xp, int n)
{
    if (!(x >= xp[0])) return -1;
    int lo = 0, hi = n;                 // xp[lo] <= x; hi == n or xp[hi] > x
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (xp[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}
// the same from a segment valid for a smaller x: s only grows between two wraps, so the integration loops walk forward
__device__ __forceinline__ int sim_advance(double x, const double* xp, int n, int j)
{
    while (j + 1 < n && xp[j + 1] <= x) ++j;
    return j;
}

// heading at s on segment j of the trimmed trajectory (`psi(i)`: column psi of row i): np.interp's clamping, the step taken the short way
// round the circle, the result wrapped into (-pi, pi]. The operation order is the one of sim.peer_heading.
template <class PSI>
__device__ __forceinline__ double sim_heading(double s, const double* ts, int n, int j, PSI psi)
{
    if (j < 0) return psi(0);
    if (j >= n - 1) return psi(n - 1);
    if (ts[j + 1] == ts[j]) return psi(j);
    const double p0 = psi(j);
    double d = psi(j + 1) - p0;
    if (d > kPi) d -= 2 * kPi;
    else if (d < -kPi) d += 2 * kPi;
    double th = p0 + d * ((s - ts[j]) / (ts[j + 1] - ts[j]));
    if (th > kPi) th -= 2 * kPi;
    else if (th <= -kPi) th += 2 * kPi;
    return th;
}

}  // namespace fleet

#define SIM_OBJ_CAP MAX_VEH                // objects (opponents + static) per planner
#define SIM_DT_STEP 0.001                  // integration step of both simulators (objectlist_dummy.py:149, vdc_dummy.py:46)

struct SimDev {
    int n_rl; const double* race;          // [5][n_rl] column-major: s_rl, x, y, psi, vel_rl
    const int* opp_off; double* opp_s; double* opp_tic; const double* opp_scale; const double* opp_len;
    const int* st_off; const double* st_x; const double* st_y; const double* st_th; const double* st_v; const double* st_len;
    const int* pref_off; const int* pref;
    double dt; int n_export;
    double* now; int* sel; int* started; double* pos_x; double* pos_y; double* vel;
    double* theta;                         // [N] heading of the tracked pose (heading0 of ltpl_fleet_sim_race until the first trajectory)
    int* live;                             // [N] 1: the planner ran this tick's step (no error word): it takes its mates in
    int* cnt;                              // [N] on-track objects of the tick
    const int* obj_base;                   // [N] first staging slot of planner p: opponents, statics and mates of the planners before p
    double* g_x; double* g_y; double* g_px; double* g_py; double* g_r; double* g_v;   // survivors, planner p's from obj_base[p] on
    const int* mate_lo; const int* mate_hi; const double* mate_len;   // [N] race of planner p: planners mate_lo .. mate_hi - 1; length
    int* prev_action; double* t_now; int* veh_off; double* o_r; double* o_v; double* o_px; double* o_py;   // the tick's fleet::FObj arrays
};

// sensor noise (ltpl_fleet_sim_noise): what the noisy forms of k_fleet_sim_step / k_fleet_sim_mates get besides SimDev. The plain kernels
// carry none of it.
struct SimNoise {
    const uint64_t* seed;                  // [N]
    const double* sigma;                   // [5][N]: pos, vel, obj_pos, obj_theta, obj_vel
    double* est_x; double* est_y; double* est_v;   // [N] the planner's pos_est / vel_est of the tick (ltpl_fleet_sim_estimate)
    double* g_tx; double* g_ty;            // true x, y of every kept object, next to the perceived g_x / g_y (telemetry measures against truth)
    uint32_t tick;                         // tick0 + fleet ticks since the noise was set
};
enum { NZ_POS = 0, NZ_VEL, NZ_OBJ_POS, NZ_OBJ_THETA, NZ_OBJ_VEL, NZ_SIGMAS };

struct SimBest { double d; int i; };
__device__ __forceinline__ SimBest sim_better(SimBest a, SimBest b) { return (b.d < a.d || (b.d == a.d && b.i < a.i)) ? b : a; }
__device__ __forceinline__ SimBest sim_wave_min(SimBest v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { SimBest o; o.d = __shfl_xor(v.d, m); o.i = __shfl_xor(v.i, m); v = sim_better(v, o); }
    return v;
}

// vehicle model (ltpl_fleet_sim_vehicle): what the _veh forms of k_fleet_sim_step get besides SimDev. The other kernels carry none of it.
#define VEH_PARAMS 9                       // fleet::VehParams
struct SimVeh {
    const int* model;                      // [N] 0: the ideal tracker, 1: the model
    const double* par;                     // [N][VEH_PARAMS] in the order of fleet::VehParams
    double* rec;                           // [N][LTPL_FLEET_SIM_VEH_DOUBLES] state and statistics (NaN for a planner on the ideal tracker)
    int ctl_steps;                         // control period in plant steps
};
enum { VEH_X = 0, VEH_Y, VEH_C, VEH_S, VEH_V, VEH_A, VEH_KAPPA, VEH_E, VEH_E_MAX, VEH_E2_SUM, VEH_DV_MAX, VEH_CTL, VEH_SAT_LAT, VEH_SAT_LON,
       VEH_OFF_TRACK };
static_assert(VEH_OFF_TRACK + 1 == LTPL_FLEET_SIM_VEH_DOUBLES && sizeof(fleet::VehParams) == VEH_PARAMS * sizeof(double), "vehicle record layout");

__device__ __forceinline__ fleet::VehParams sim_vehicle_params(const double* q)
{
    return fleet::VehParams{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]};
}
// a tick of the model by a whole wave: every lane holds the same state and runs the same loop; the projection of a control step is
// lane-parallel over the segments (fleet::veh_seg) and ends in the wave-wide minimum, ties to the lower segment (sim_better)
__device__ __forceinline__ void sim_vehicle_tick(int lane, fleet::VehState& S, const fleet::VehParams& P, const fleet::VehRows& R, double dt,
                                                 int ctl_steps, fleet::VehStats& st)
{
    fleet::veh_tick(S, P, R, dt, ctl_steps, st, [&](double px, double py) {
        SimBest b{INFINITY, fleet::kVehNone};
        for (int i = lane; i + 1 < R.n; i += 64) {
            double d2;
            if (fleet::veh_seg(R, i, px, py, &d2)) b = sim_better(b, SimBest{d2, i});
        }
        b = sim_wave_min(b);
        return fleet::VehBest{b.d, b.i};
    });
}

// the body of k_fleet_sim_step (NOISE false: `nz` is not touched and the code is the one without noise) and of k_fleet_sim_step_noise: every
// object perturbed in its ingestion lane (registers only: no LDS is added), the ego estimate written behind the tracker by lane 0.
// VEH (k_fleet_sim_step_veh, k_fleet_sim_step_noise_veh): column ax staged too; a planner with vh.model[p] != 0 drives the vehicle model
template <bool NOISE, bool VEH>
__device__ __forceinline__ void sim_step_body(const FleetArgs& F, const DevLat& lat, const SimDev& sd, double* trace, const SimNoise& nz,
                                              const SimVeh& vh)
{
    const int p = blockIdx.x, lane = threadIdx.x; const WaveX x{lane};
    const fleet::Block B{F.state + F.D.stride * (size_t)p, F.D, nullptr};
    __shared__ fleet::PlannerS S;
    __shared__ double ts[LTPL_FLEET_SIM_MAX_EXPORT], tx[LTPL_FLEET_SIM_MAX_EXPORT], ty[LTPL_FLEET_SIM_MAX_EXPORT], tv[LTPL_FLEET_SIM_MAX_EXPORT];
    __shared__ double ox[SIM_OBJ_CAP], oy[SIM_OBJ_CAP], oth[SIM_OBJ_CAP], ov[SIM_OBJ_CAP], ol[SIM_OBJ_CAP];
    __shared__ double first_xy[2];
    double* ta = nullptr;                  // column ax: LDS of the _veh forms only
    if constexpr (VEH) { __shared__ double ta_lds[LTPL_FLEET_SIM_MAX_EXPORT]; ta = ta_lds; }
    fleet_load(x, B, &S);
    double now = sd.now[p], pos_x = sd.pos_x[p], pos_y = sd.pos_y[p], vel = sd.vel[p], theta = sd.theta[p];
    int sel = sd.sel[p], cnt = 0;
    bool failed = false;
    if (lane == 0) { first_xy[0] = NAN; first_xy[1] = NAN; }
    if (!S.err) {
        now += sd.dt;
        // action choice (run_loop: the first preferred key of the previous exported set; before the first tick {'straight': None})
        const int started = sd.started[p];
        int slot = -1;
        bool found = false;
        for (int i = sd.pref_off[p]; i < sd.pref_off[p + 1] && !found; ++i) {
            sel = sd.pref[i];
            if (!started) found = sel == LTPL_ACT_STRAIGHT;
            else for (int k = 0; k < S.n_bp && !found; ++k) if (S.bp_id[k] == sel) { found = true; slot = k; }
        }
        if (!found) {
            fleet::fail(S, LTPL_ERR_INVALID_ARG, fleet::E_SIM_ACTION);
            failed = true;
        } else {
            const int o0 = sd.opp_off[p], no = sd.opp_off[p + 1] - o0, s0 = sd.st_off[p], ns = sd.st_off[p + 1] - s0;
            const int n_rl = sd.n_rl;
            const double* s_rl = sd.race;
            // opponents: one lane each (objectlist_dummy.py:148-170)
            for (int q = lane; q < no; q += 64) {
                const double scale = sd.opp_scale[o0 + q];
                const double* vrl = s_rl + (size_t)4 * n_rl;
                auto vel_s = [&](int i) { return vrl[i] * scale; };
                double s = sd.opp_s[o0 + q];
                const double toc = now - sd.opp_tic[o0 + q];
                double t = 0.0;
                int j = fleet::sim_segment(s, s_rl, n_rl);
                while (t < toc) {
                    s += fleet::sim_interp(s, s_rl, n_rl, j, vel_s) * SIM_DT_STEP;
                    t += SIM_DT_STEP;
                    if (s >= s_rl[n_rl - 1]) { s = 0.0; j = fleet::sim_segment(s, s_rl, n_rl); }
                    else j = fleet::sim_advance(s, s_rl, n_rl, j);
                }
                sd.opp_s[o0 + q] = s; sd.opp_tic[o0 + q] = now;
                const double* cx = s_rl + n_rl; const double* cy = cx + n_rl; const double* cpsi = cy + n_rl;
                ox[q] = fleet::sim_interp(s, s_rl, n_rl, j, [&](int i) { return cx[i]; });
                oy[q] = fleet::sim_interp(s, s_rl, n_rl, j, [&](int i) { return cy[i]; });
                double psi = fleet::sim_interp(s, s_rl, n_rl, j, [&](int i) { return cpsi[i]; });
                if (psi > fleet::kPi) psi -= 2 * fleet::kPi;
                oth[q] = psi; ov[q] = fleet::sim_interp(s, s_rl, n_rl, j, vel_s); ol[q] = sd.opp_len[o0 + q];
            }
            for (int q = lane; q < ns; q += 64) {
                ox[no + q] = sd.st_x[s0 + q]; oy[no + q] = sd.st_y[s0 + q]; oth[no + q] = sd.st_th[s0 + q]; ov[no + q] = sd.st_v[s0 + q];
                ol[no + q] = sd.st_len[s0 + q];
            }
            __syncthreads();
            // ingestion: survivors in list order (ballot + prefix count), staged from the planner's first object slot on
            const int base = sd.obj_base[p], nobj = no + ns;
            for (int b0 = 0; b0 < nobj; b0 += 64) {
                const int k = b0 + lane;
                ObjIngest r{0, 0.0, 0.0, 0.0};
                double kx = 0.0, ky = 0.0, kth = 0.0, kv = 0.0;          // the object as the planner perceives it
                if (k < nobj) {
                    kx = ox[k]; ky = oy[k]; kth = oth[k]; kv = ov[k];
                    if constexpr (NOISE) {
                        const uint64_t seed = nz.seed[p]; const int N = (int)gridDim.x;
                        const double sp = nz.sigma[(size_t)NZ_OBJ_POS * N + p];
                        kx = fleet::noise_add(kx, sp, seed, nz.tick, (uint32_t)k, 0);
                        ky = fleet::noise_add(ky, sp, seed, nz.tick, (uint32_t)k, 1);
                        kth = fleet::noise_add(kth, nz.sigma[(size_t)NZ_OBJ_THETA * N + p], seed, nz.tick, (uint32_t)k, 2);
                        kv = fleet::noise_add_speed(kv, nz.sigma[(size_t)NZ_OBJ_VEL * N + p], seed, nz.tick, (uint32_t)k, 3);
                    }
                    r = process_object_dev(lat, 0.2, kx, ky, kth, kv, ol[k]);     // ObjectListInterface.py:121
                }
                const bool keep = k < nobj && r.on_track;
                const unsigned long long m = __ballot(keep);
                const int idx = cnt + __popcll(m & ((1ull << lane) - 1ull));
                if (keep) {
                    sd.g_x[base + idx] = kx; sd.g_y[base + idx] = ky; sd.g_px[base + idx] = r.pred_x; sd.g_py[base + idx] = r.pred_y;
                    sd.g_r[base + idx] = r.radius; sd.g_v[base + idx] = kv;
                    if constexpr (NOISE) { nz.g_tx[base + idx] = ox[k]; nz.g_ty[base + idx] = oy[k]; }
                    if (idx == 0) { first_xy[0] = kx; first_xy[1] = ky; }
                }
                cnt += __popcll(m);
            }
            // ego tracker on the previous trajectory of the selected action (vdc_dummy.py:5-58), trimmed to the exported rows
            if (started) {
                const fleet::Rows tr = B.bp(S.bp_slot[slot]);
                const int n = S.bp_rows[slot] < sd.n_export ? S.bp_rows[slot] : sd.n_export;
                for (int i = lane; i < n; i += 64) { ts[i] = tr.at(i, 0); tx[i] = tr.at(i, 1); ty[i] = tr.at(i, 2); tv[i] = tr.at(i, 5); }
                if constexpr (VEH) for (int i = lane; i < n; i += 64) ta[i] = tr.at(i, 6);
                __syncthreads();
                if (VEH && vh.model[p] != 0) {
                    // the vehicle model in place of the ideal tracker (fleet_vehicle.hpp): the record is the state, pos / vel / theta its outputs
                    double* r = vh.rec + (size_t)p * LTPL_FLEET_SIM_VEH_DOUBLES;
                    fleet::VehState V{r[VEH_X], r[VEH_Y], r[VEH_C], r[VEH_S], r[VEH_V], r[VEH_A], r[VEH_KAPPA]};
                    fleet::VehStats st{r[VEH_E], r[VEH_E_MAX], r[VEH_E2_SUM], r[VEH_DV_MAX], r[VEH_CTL], r[VEH_SAT_LAT], r[VEH_SAT_LON]};
                    sim_vehicle_tick(lane, V, sim_vehicle_params(vh.par + (size_t)p * VEH_PARAMS), fleet::VehRows{ts, tx, ty, tv, ta, n}, sd.dt,
                                     vh.ctl_steps, st);
                    pos_x = V.x; pos_y = V.y; vel = V.v; theta = heading_atan2(-V.c, V.s);
                    if (lane == 0) {
                        r[VEH_X] = V.x; r[VEH_Y] = V.y; r[VEH_C] = V.c; r[VEH_S] = V.s; r[VEH_V] = V.v; r[VEH_A] = V.a; r[VEH_KAPPA] = V.kappa;
                        r[VEH_E] = st.e; r[VEH_E_MAX] = st.e_max; r[VEH_E2_SUM] = st.e2_sum; r[VEH_DV_MAX] = st.dv_max; r[VEH_CTL] = st.ctl;
                        r[VEH_SAT_LAT] = st.sat_lat; r[VEH_SAT_LON] = st.sat_lon;
                        if (!process_object_dev(lat, 0.2, V.x, V.y, 0.0, 0.0, 0.0).on_track) r[VEH_OFF_TRACK] += 1.0;   // the ingestion's track test
                    }
                } else if (n <= 2) {
                    vel = n > 0 ? tv[0] : vel;
                } else {
                    const double ex = pos_x, ey = pos_y;
                    SimBest b1{INFINITY, 0x7fffffff};
                    for (int i = lane; i < n; i += 64) b1 = sim_better(b1, SimBest{(tx[i] - ex) * (tx[i] - ex) + (ty[i] - ey) * (ty[i] - ey), i});
                    b1 = sim_wave_min(b1);
                    SimBest b2{INFINITY, 0x7fffffff};
                    for (int i = lane; i < n; i += 64)
                        if (i != b1.i) b2 = sim_better(b2, SimBest{(tx[i] - ex) * (tx[i] - ex) + (ty[i] - ey) * (ty[i] - ey), i});
                    b2 = sim_wave_min(b2);
                    int i0 = b1.i < b2.i ? b1.i : b2.i;
                    if (i0 < 0 || i0 >= n) i0 = 0;               // (NaN distances only)
                    if (lane == 0) {
                        const double dx = tx[i0] - ex, dy = ty[i0] - ey;
                        double s = sqrt(dx * dx + dy * dy) + ts[i0];
                        auto vx = [&](int i) { return tv[i]; };
                        int j = fleet::sim_segment(s, ts, n);
                        double t = 0.0;
                        while (t < sd.dt) {
                            const double step = fleet::sim_interp(s, ts, n, j, vx) * SIM_DT_STEP;
                            s += 0.0001 > step ? 0.0001 : step;      // Python's max(step, 0.0001): the second only where it is larger (NaN stays)
                            t += SIM_DT_STEP;
                            j = fleet::sim_advance(s, ts, n, j);
                        }
                        pos_x = fleet::sim_interp(s, ts, n, j, [&](int i) { return tx[i]; });
                        pos_y = fleet::sim_interp(s, ts, n, j, [&](int i) { return ty[i]; });
                        vel = fleet::sim_interp(s, ts, n, j, vx);
                        theta = fleet::sim_heading(s, ts, n, j, [&](int i) { return tr.at(i, 3); });   // (two rows: read in place)
                    }
                }
            }
        }
    }
    __syncthreads();
    if (lane == 0) {
        if (!failed && !S.err) {
            sd.now[p] = now; sd.sel[p] = sel; sd.started[p] = 1; sd.pos_x[p] = pos_x; sd.pos_y[p] = pos_y; sd.vel[p] = vel;
            sd.theta[p] = theta;
            if constexpr (NOISE) {          // the estimate the fleet's tick reads as pos_est / vel_est; the true pose stays in sd
                const uint64_t seed = nz.seed[p]; const int N = (int)gridDim.x;
                const double sp = nz.sigma[(size_t)NZ_POS * N + p];
                nz.est_x[p] = fleet::noise_add(pos_x, sp, seed, nz.tick, fleet::kNoiseEgo, 0);
                nz.est_y[p] = fleet::noise_add(pos_y, sp, seed, nz.tick, fleet::kNoiseEgo, 1);
                nz.est_v[p] = fleet::noise_add_speed(vel, nz.sigma[(size_t)NZ_VEL * N + p], seed, nz.tick, fleet::kNoiseEgo, 2);
            }
        }
        sd.live[p] = !failed && !S.err;
        sd.cnt[p] = cnt; sd.prev_action[p] = sd.sel[p]; sd.t_now[p] = sd.now[p];
        if (trace) {
            double* o = trace + (size_t)p * LTPL_FLEET_SIM_TRACE_DOUBLES;
            o[0] = (double)sel; o[1] = now; o[2] = pos_x; o[3] = pos_y; o[4] = vel; o[5] = (double)cnt; o[6] = first_xy[0]; o[7] = first_xy[1];
        }
    }
    if (failed) fleet_store(x, B, &S, p, F.err_word);
}
__global__ __launch_bounds__(64) void k_fleet_sim_step(FleetArgs F, DevLat lat, SimDev sd, double* trace /* this tick's records or null */)
{
    sim_step_body<false, false>(F, lat, sd, trace, SimNoise{}, SimVeh{});
}
__global__ __launch_bounds__(64) void k_fleet_sim_step_noise(FleetArgs F, DevLat lat, SimDev sd, double* trace, SimNoise nz)
{
    sim_step_body<true, false>(F, lat, sd, trace, nz, SimVeh{});
}
__global__ __launch_bounds__(64) void k_fleet_sim_step_veh(FleetArgs F, DevLat lat, SimDev sd, double* trace, SimVeh vh)
{
    sim_step_body<false, true>(F, lat, sd, trace, SimNoise{}, vh);
}
__global__ __launch_bounds__(64) void k_fleet_sim_step_noise_veh(FleetArgs F, DevLat lat, SimDev sd, double* trace, SimNoise nz, SimVeh vh)
{
    sim_step_body<true, true>(F, lat, sd, trace, nz, vh);
}

// the planner's mates (every other planner of its race, ascending) as objects at their tracked pose, speed and heading: the ingestion of
// k_fleet_sim_step, appended behind the opponents and statics that step kept. A failed planner takes no objects; a failed mate stays at
// its last state. Trace fields [5] .. [7] of step are completed here.
template <bool NOISE>
__device__ __forceinline__ void sim_mates_body(const DevLat& lat, const SimDev& sd, double* trace, const SimNoise& nz)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    const int lo = sd.mate_lo[p], hi = sd.mate_hi[p];
    if (hi - lo < 2 || !sd.live[p]) return;
    const int base = sd.obj_base[p], c0 = sd.cnt[p];
    double* o = trace ? trace + (size_t)p * LTPL_FLEET_SIM_TRACE_DOUBLES : nullptr;
    int cnt = c0;
    for (int b0 = lo; b0 < hi; b0 += 64) {
        const int q = b0 + lane;
        const bool mate = q < hi && q != p;
        ObjIngest r{0, 0.0, 0.0, 0.0};
        double qx = 0.0, qy = 0.0, qv = 0.0, tx = 0.0, ty = 0.0;
        if (mate) {
            qx = sd.pos_x[q]; qy = sd.pos_y[q]; qv = sd.vel[q];
            double qth = sd.theta[q];
            if constexpr (NOISE) {          // the mate as planner p perceives it: p's seed, the mate's place in the race
                const uint64_t seed = nz.seed[p]; const int N = (int)gridDim.x;
                const uint32_t obj = fleet::kNoiseMate | (uint32_t)(q - lo);
                const double sp = nz.sigma[(size_t)NZ_OBJ_POS * N + p];
                tx = qx; ty = qy;
                qx = fleet::noise_add(qx, sp, seed, nz.tick, obj, 0);
                qy = fleet::noise_add(qy, sp, seed, nz.tick, obj, 1);
                qth = fleet::noise_add(qth, nz.sigma[(size_t)NZ_OBJ_THETA * N + p], seed, nz.tick, obj, 2);
                qv = fleet::noise_add_speed(qv, nz.sigma[(size_t)NZ_OBJ_VEL * N + p], seed, nz.tick, obj, 3);
            }
            r = process_object_dev(lat, 0.2, qx, qy, qth, qv, sd.mate_len[q]);     // ObjectListInterface.py:121
        }
        const bool keep = mate && r.on_track;
        const unsigned long long m = __ballot(keep);
        const int idx = cnt + __popcll(m & ((1ull << lane) - 1ull));
        if (keep) {
            sd.g_x[base + idx] = qx; sd.g_y[base + idx] = qy; sd.g_px[base + idx] = r.pred_x; sd.g_py[base + idx] = r.pred_y;
            sd.g_r[base + idx] = r.radius; sd.g_v[base + idx] = qv;
            if constexpr (NOISE) { nz.g_tx[base + idx] = tx; nz.g_ty[base + idx] = ty; }
            if (idx == 0 && o) { o[6] = qx; o[7] = qy; }
        }
        cnt += __popcll(m);
    }
    if (lane == 0 && cnt != c0) {
        sd.cnt[p] = cnt;
        if (o) o[5] = (double)cnt;
    }
}
__global__ __launch_bounds__(64) void k_fleet_sim_mates(DevLat lat, SimDev sd, double* trace /* this tick's records or null */)
{
    sim_mates_body<false>(lat, sd, trace, SimNoise{});
}
__global__ __launch_bounds__(64) void k_fleet_sim_mates_noise(DevLat lat, SimDev sd, double* trace, SimNoise nz)
{
    sim_mates_body<true>(lat, sd, trace, nz);
}

// ---------------------------------------------------------------------------------------------------------------------
// race telemetry (ltpl_fleet_sim_telemetry, include/ltpl_hip.h): a record of LTPL_FLEET_SIM_TELE_DOUBLES doubles per planner, updated in
// every tick in which the planner is live, behind its tracker and its mates. fp64, + - * / sqrt only, in the operation order of the
// header's table (host mirror: sim.Telemetry). The pointers live in a struct of their own: k_fleet_sim_step carries none of them.
// ---------------------------------------------------------------------------------------------------------------------
enum { TELE_TICKS = 0, TELE_S, TELE_DIST, TELE_LAPS, TELE_T_CROSS, TELE_LAP_LAST, TELE_LAP_BEST, TELE_VEL_SUM, TELE_VEL_MAX, TELE_ACT,
       TELE_CLEAR_MIN = 14, TELE_CLEAR_TICK, TELE_CLEAR_SLOT, TELE_CONTACT, TELE_RANK, TELE_PASSES, TELE_PASSED, TELE_GAP };
static_assert(TELE_GAP + 1 == LTPL_FLEET_SIM_TELE_DOUBLES, "telemetry record layout");

struct SimTele {
    int n_rl; const double* rl_x; const double* rl_y; const double* rl_s;   // the lattice's race line, one point per layer, contiguous
    double length;                         // closed length of the race line
    const double* radius;                  // [N] contact radius
    double* grid_s;                        // [N] progress offset of planner p (NaN: s of its first live tick, written there)
    double* rec;                           // [N][LTPL_FLEET_SIM_TELE_DOUBLES]
    double* prog;                          // [N] grid_s + dist of the last live tick (-inf before the first: behind everybody)
};

// `g_tx`, `g_ty` (null while the noise is off): the true positions of the tick's objects. Clearance and contacts are measured against
// them; the planner was handed the perceived g_x / g_y.
__global__ __launch_bounds__(64) void k_fleet_sim_tele(SimDev sd, SimTele te, int tick, const double* g_tx, const double* g_ty)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    if (!sd.live[p]) return;
    const double px = sd.pos_x[p], py = sd.pos_y[p];
    // (a pose that is not finite, or so far out that its squared distances overflow, has no closest point: the search would leave its index unset)
    const double s = fabs(px) <= 1e100 && fabs(py) <= 1e100 ? get_s_coord_dev(te.n_rl, te.rl_x, te.rl_y, 1, te.rl_s, 1, px, py, true, lane, nullptr) : NAN;
    // smallest clearance over the objects the planner is handed this tick (first smallest: the lower slot)
    const int base = sd.obj_base[p], cnt = sd.cnt[p];
    const double* gx = g_tx ? g_tx : sd.g_x; const double* gy = g_tx ? g_ty : sd.g_y;
    double cd = INFINITY; int ci = 0x7fffffff;
    for (int b0 = 0; b0 < cnt; b0 += 64) {
        const int k = b0 + lane;
        if (k < cnt) {
            const double dx = gx[base + k] - px, dy = gy[base + k] - py;
            const double c = sqrt(dx * dx + dy * dy) - sd.g_r[base + k];
            if (c < cd) { cd = c; ci = k; }
        }
    }
    wave_min2(cd, ci);
    if (lane != 0) return;
    double* r = te.rec + (size_t)p * LTPL_FLEET_SIM_TELE_DOUBLES;
    const double L = te.length, t_now = sd.now[p], vel = sd.vel[p];
    double delta = 0.0;
    bool fwd = false, bwd = false;
    if (r[TELE_TICKS] == 0.0) {
        if (isnan(te.grid_s[p])) te.grid_s[p] = s;
    } else {
        delta = s - r[TELE_S];
        if (delta < -(L / 2)) { delta += L; fwd = true; }
        else if (delta > L / 2) { delta -= L; bwd = true; }
    }
    r[TELE_TICKS] += 1.0;
    r[TELE_S] = s;
    r[TELE_DIST] += delta;
    if (fwd) {
        r[TELE_LAPS] += 1.0;
        const double tc = delta > 0.0 ? t_now - sd.dt * (s / delta) : t_now;
        const double prev = r[TELE_T_CROSS];
        r[TELE_T_CROSS] = tc;
        if (!isnan(prev)) {
            const double lap = tc - prev;
            r[TELE_LAP_LAST] = lap;
            if (isnan(r[TELE_LAP_BEST]) || lap < r[TELE_LAP_BEST]) r[TELE_LAP_BEST] = lap;
        }
    }
    if (bwd) r[TELE_LAPS] -= 1.0;
    r[TELE_VEL_SUM] += vel;
    if (vel > r[TELE_VEL_MAX]) r[TELE_VEL_MAX] = vel;
    const int sel = sd.sel[p];
    if (sel >= LTPL_ACT_STRAIGHT && sel <= LTPL_ACT_EMERGENCY) r[TELE_ACT + sel] += 1.0;
    if (cnt > 0) {
        if (cd < r[TELE_CLEAR_MIN]) { r[TELE_CLEAR_MIN] = cd; r[TELE_CLEAR_TICK] = (double)tick; r[TELE_CLEAR_SLOT] = (double)ci; }
        if (cd < te.radius[p]) r[TELE_CONTACT] += 1.0;
    }
    te.prog[p] = te.grid_s[p] + r[TELE_DIST];
    if (!sd.mate_lo || sd.mate_hi[p] - sd.mate_lo[p] < 2) r[TELE_RANK] = 1.0;          // alone in its race: no passes, no gap
}

// rank of planner p among the planners of its race by progress (ahead: larger, or equal and a lower planner index) and the gap to the
// nearest one ahead. A mate that has not lived a tick stands at -inf; a failed mate stays where it stopped.
__global__ __launch_bounds__(64) void k_fleet_sim_rank(SimDev sd, SimTele te)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    const int lo = sd.mate_lo[p], hi = sd.mate_hi[p];
    if (hi - lo < 2 || !sd.live[p]) return;
    const double mine = te.prog[p];
    int ahead = 0;
    double gap = INFINITY;
    for (int b0 = lo; b0 < hi; b0 += 64) {
        const int q = b0 + lane;
        bool a = false;
        if (q < hi && q != p) {
            const double pq = te.prog[q];
            a = pq > mine || (pq == mine && q < p);
            if (a) { const double g = pq - mine; if (g < gap) gap = g; }
        }
        ahead += __popcll(__ballot(a));
    }
    gap = wave_min_f64(gap);
    if (lane != 0) return;
    double* r = te.rec + (size_t)p * LTPL_FLEET_SIM_TELE_DOUBLES;
    const double rank = (double)(1 + ahead), prev = r[TELE_RANK];
    if (r[TELE_TICKS] > 1.0) {
        if (rank < prev) r[TELE_PASSES] += prev - rank;
        else if (rank > prev) r[TELE_PASSED] += rank - prev;
    }
    r[TELE_RANK] = rank;
    r[TELE_GAP] = ahead ? gap : NAN;
}

// ---------------------------------------------------------------------------------------------------------------------
// sensor model (ltpl_fleet_sim_sensor, include/ltpl_hip.h; the rule: fleet_sensor.hpp; host mirror: sim.SensorModel). A pure function of
// the tick's true state: configuration and a statistics record, no state. The pointers live in a struct of their own: no other kernel
// carries them.
// ---------------------------------------------------------------------------------------------------------------------
#define SENS_PARAMS 5                      // fleet::SensorParams
enum { SENS_TICKS = 0, SENS_N_OBJ, SENS_N_SEEN, SENS_N_RANGE, SENS_N_FOV, SENS_N_OCCL, SENS_N_DROP, SENS_BLIND_TICKS, SENS_CLEAR_MIN, SENS_CLEAR_TICK };
static_assert(SENS_CLEAR_TICK + 1 == LTPL_FLEET_SIM_SENSOR_DOUBLES && sizeof(fleet::SensorParams) == SENS_PARAMS * sizeof(double) &&
              SENS_N_RANGE + fleet::kSenseDrop - fleet::kSenseRange == SENS_N_DROP, "sensor record layout");
struct SimSense {
    const double* par;                     // [N][SENS_PARAMS] in the order of fleet::SensorParams
    const uint64_t* seed;                  // [N]
    double* rec;                           // [N][LTPL_FLEET_SIM_SENSOR_DOUBLES]
    uint32_t tick;                         // tick0 + fleet ticks since the sensor was set
};
struct SenseLds { double dx[SIM_OBJ_CAP], dy[SIM_OBJ_CAP], L2[SIM_OBJ_CAP], r[SIM_OBJ_CAP]; };

// the geometry of n objects (x, y, r `stride` doubles apart) seen from (px, py), one lane per object
__device__ __forceinline__ void sim_sense_stage(int lane, int n, double px, double py, const double* x, const double* y, const double* r, int stride,
                                                SenseLds& L)
{
    for (int k = lane; k < n; k += 64) {
        const fleet::SensorObj o = fleet::sensor_obj(px, py, x[(size_t)k * stride], y[(size_t)k * stride]);
        L.dx[k] = o.dx; L.dy[k] = o.dy; L.L2[k] = o.L2; L.r[k] = r[(size_t)k * stride];
    }
}
__device__ __forceinline__ fleet::SensorParams sim_sensor_params(const double* q) { return fleet::SensorParams{q[0], q[1], q[2], q[3], q[4]}; }

// `g_tx`, `g_ty` (null while the noise is off): the true positions of the tick's objects -- what decides whether an object is detected; what
// is handed on is what the noise made of it. Each lane loads the sources of its object before any lane stores (a barrier in between);
// destination <= source, and the second pass writes behind what the first one wrote and reads from slot 64 on.
__global__ __launch_bounds__(64) void k_fleet_sim_sense(SimDev sd, SimSense sn, double* g_tx, double* g_ty, double* trace /* this tick's records or null */)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    if (!sd.live[p]) return;
    __shared__ SenseLds L;
    const int base = sd.obj_base[p];
    int cnt = sd.cnt[p];
    if (cnt > SIM_OBJ_CAP) cnt = SIM_OBJ_CAP;
    const double px = sd.pos_x[p], py = sd.pos_y[p], th = sd.theta[p];
    const double fx = -sin(th), fy = cos(th);
    sim_sense_stage(lane, cnt, px, py, (g_tx ? g_tx : sd.g_x) + base, (g_tx ? g_ty : sd.g_y) + base, sd.g_r + base, 1, L);
    __syncthreads();
    const fleet::SensorParams P = sim_sensor_params(sn.par + (size_t)p * SENS_PARAMS);
    const uint64_t seed = sn.seed[p];
    double* o = trace ? trace + (size_t)p * LTPL_FLEET_SIM_TRACE_DOUBLES : nullptr;
    int kept = 0, lost[4] = {0, 0, 0, 0};
    double cd = INFINITY; int ci = 0x7fffffff;
    for (int b0 = 0; b0 < cnt; b0 += 64) {
        const int k = b0 + lane, g = base + k;
        int cause = -1;
        double vx = 0.0, vy = 0.0, vpx = 0.0, vpy = 0.0, vr = 0.0, vv = 0.0, vtx = 0.0, vty = 0.0;
        if (k < cnt) {
            vx = sd.g_x[g]; vy = sd.g_y[g]; vpx = sd.g_px[g]; vpy = sd.g_py[g]; vr = sd.g_r[g]; vv = sd.g_v[g];
            if (g_tx) { vtx = g_tx[g]; vty = g_ty[g]; }
            double u;
            cause = fleet::sensor_cause(P, seed, sn.tick, fx, fy, L.dx, L.dy, L.L2, L.r, cnt, k, &u);
            if (cause != fleet::kSenseSeen) {
                const double c = fleet::sensor_clearance(L.L2[k], L.r[k]);
                if (c < cd) { cd = c; ci = k; }
            }
        }
        const bool keep = cause == fleet::kSenseSeen;
        const unsigned long long m = __ballot(keep);
        const int d = base + kept + __popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
        for (int c = 0; c < 4; ++c) lost[c] += __popcll(__ballot(cause == fleet::kSenseRange + c));
        __syncthreads();
        if (keep) {
            sd.g_x[d] = vx; sd.g_y[d] = vy; sd.g_px[d] = vpx; sd.g_py[d] = vpy; sd.g_r[d] = vr; sd.g_v[d] = vv;
            if (g_tx) { g_tx[d] = vtx; g_ty[d] = vty; }
            if (d == base && o) { o[6] = vx; o[7] = vy; }
        }
        kept += __popcll(m);
    }
    wave_min2(cd, ci);
    if (lane != 0) return;
    sd.cnt[p] = kept;
    if (o) {
        o[5] = (double)kept;
        if (kept == 0) { o[6] = NAN; o[7] = NAN; }
    }
    double* r = sn.rec + (size_t)p * LTPL_FLEET_SIM_SENSOR_DOUBLES;
    r[SENS_TICKS] += 1.0; r[SENS_N_OBJ] += (double)cnt; r[SENS_N_SEEN] += (double)kept;
#pragma unroll
    for (int c = 0; c < 4; ++c) r[SENS_N_RANGE + c] += (double)lost[c];
    if (kept != cnt) {
        r[SENS_BLIND_TICKS] += 1.0;
        if (cd < r[SENS_CLEAR_MIN]) { r[SENS_CLEAR_MIN] = cd; r[SENS_CLEAR_TICK] = (double)sn.tick; }
    }
}

// the test hook of the rule: one wave per case, the staging and the decision of k_fleet_sim_sense on the case's own objects. The forward
// vector is handed in: no trigonometry here
__global__ __launch_bounds__(64) void k_fleet_sim_sensor_eval(const double* pose_f, const double* par, const uint64_t* seed, const uint32_t* tick,
                                                              const int* obj_off, const double* objs, int* cause, double* u)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    __shared__ SenseLds L;
    const int o0 = obj_off[q];
    int n = obj_off[q + 1] - o0;
    if (n > SIM_OBJ_CAP) n = SIM_OBJ_CAP;      // (refused by the host)
    const double* pf = pose_f + (size_t)q * 4;
    const double* ob = objs + (size_t)o0 * 3;
    sim_sense_stage(lane, n, pf[0], pf[1], ob, ob + 1, ob + 2, 3, L);
    __syncthreads();
    const fleet::SensorParams P = sim_sensor_params(par + (size_t)q * SENS_PARAMS);
    for (int k = lane; k < n; k += 64) {
        double uu = NAN;
        cause[o0 + k] = fleet::sensor_cause(P, seed[q], tick[q], pf[2], pf[3], L.dx, L.dy, L.L2, L.r, n, k, &uu);
        u[o0 + k] = uu;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// object tracker (ltpl_fleet_sim_tracker, include/ltpl_hip.h; the rule: fleet_track.hpp; host mirror: sim.TrackerModel). Configuration, a
// statistics record and STATE: the planner's track table, its count and next_id (copied by snapshot / branch, fleet_branch.hpp). The
// pointers live in a struct of their own: no other kernel carries them.
// ---------------------------------------------------------------------------------------------------------------------
#define TRK_PARAMS 5                       // fleet::TrackParams
static_assert(fleet::TRK_DOUBLES == LTPL_FLEET_SIM_TRACK_DOUBLES && fleet::TRS_DOUBLES == LTPL_FLEET_SIM_TRACKER_DOUBLES &&
              sizeof(fleet::TrackParams) == TRK_PARAMS * sizeof(double) && fleet::kTrackCap == SIM_OBJ_CAP && SIM_OBJ_CAP <= 128,
              "tracker record layout");
struct SimTrack {
    const double* par;                     // [N][TRK_PARAMS] in the order of fleet::TrackParams
    const int* base;                       // [N] first table row of planner p
    const int* cap;                        // [N] C_p = min(96, 2 S_p)
    const int* slots;                      // [N] S_p: the planner's staging slots
    double* rows;                          // [sum C_p][LTPL_FLEET_SIM_TRACK_DOUBLES]
    int* n;                                // [N] tracks in the table
    double* next_id;                       // [N]
    double* rec;                           // [N][LTPL_FLEET_SIM_TRACKER_DOUBLES]
    double adv;                            // dt / 0.2: ticks per prediction horizon of the ingestion
    uint32_t tick;                         // tick0 + fleet ticks since the tracker was set
};
struct TrackLds { double xp[SIM_OBJ_CAP], yp[SIM_OBJ_CAP], d[6][SIM_OBJ_CAP]; int tm[SIM_OBJ_CAP]; };
// detections in, handed-on list out: six arrays (x, y, px, py, r, v), elements `stride` doubles apart. Both may be the same memory: every
// detection is staged in LDS before the first store
struct TrackIo { const double* in[6]; double* out[6]; int stride; };

// the nearest free gated track of detection (xk, yk): lowest (d2, t). tf0 / tf1: the free tracks, uniform; every lane walks t in step
__device__ __forceinline__ void sim_track_scan(const TrackLds& L, int T, unsigned long long tf0, unsigned long long tf1, double xk, double yk, double g2,
                                               double& bd, int& bt)
{
    bd = INFINITY; bt = -1;
    for (int t = 0; t < T; ++t) {
        if (!((t < 64 ? tf0 >> t : tf1 >> (t - 64)) & 1ull)) continue;
        const double d2 = fleet::track_d2(xk, yk, L.xp[t], L.yp[t]);
        if (fleet::track_gated(d2, g2) && d2 < bd) { bd = d2; bt = t; }
    }
}
__device__ __forceinline__ fleet::TrackDet sim_track_lds_det(const TrackLds& L, int k)
{
    return fleet::TrackDet{L.d[0][k], L.d[1][k], L.d[2][k], L.d[3][k], L.d[4][k], L.d[5][k]};
}

// One tick of one planner's tracker by one wave64 (every lane enters). Lane l holds tracks l and l + 64 and detections l and l + 64 in
// registers from the staging to the stores at the end: sources are read before any destination is written. Returns the number of
// objects handed on (uniform). `assign` (or null): per detection the matched id, kTrackUnmatched or kTrackOverflow; `first` (or null):
// x, y of the first object handed on.
__device__ __forceinline__ int sim_track_tick(int lane, const fleet::TrackParams& P, double adv, double tick, int cap, int slots, double* rows, int* n_trk,
                                              double* next_id, int K, const TrackIo& io, int* assign, double* rec, double* first, TrackLds& L)
{
    constexpr int RD = LTPL_FLEET_SIM_TRACK_DOUBLES;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int T = *n_trk;
    if (T > cap) T = cap;                  // (never: the host refuses a copy above the capacity)
    const double id0 = *next_id;
    fleet::TrackRow row[2];
    double xp[2] = {0.0, 0.0}, yp[2] = {0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int t = lane + 64 * h;
#pragma unroll
        for (int c = 0; c < RD; ++c) row[h].f[c] = t < T ? rows[(size_t)t * RD + c] : 0.0;
        if (t < T) {
            xp[h] = fleet::track_predict(row[h].f[fleet::TRK_X], adv, row[h].f[fleet::TRK_EX]);
            yp[h] = fleet::track_predict(row[h].f[fleet::TRK_Y], adv, row[h].f[fleet::TRK_EY]);
            L.xp[t] = xp[h]; L.yp[t] = yp[h]; L.tm[t] = -1;
        }
    }
    for (int k = lane; k < K; k += 64) {
        const size_t i = (size_t)k * io.stride;
        const fleet::TrackDet d = fleet::track_det(io.in[0][i], io.in[1][i], io.in[2][i], io.in[3][i], io.in[4][i], io.in[5][i]);
        L.d[0][k] = d.x; L.d[1][k] = d.y; L.d[2][k] = d.ex; L.d[3][k] = d.ey; L.d[4][k] = d.r; L.d[5][k] = d.v;
    }
    __syncthreads();
    // step 2: one accepted pair per round, the wave's minimum over (d2, t 128 + k); a lane rescans only when its best track was taken
    const double g2 = fleet::track_gate2(P.gate);
    unsigned long long tf0 = T >= 64 ? ~0ull : (1ull << T) - 1ull, tf1 = T > 64 ? (1ull << (T - 64)) - 1ull : 0ull;
    double bd[2], xk[2], yk[2]; int bt[2]; bool unm[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        unm[h] = k < K; bd[h] = INFINITY; bt[h] = -1; xk[h] = yk[h] = 0.0;
        if (unm[h]) { xk[h] = L.d[0][k]; yk[h] = L.d[1][k]; sim_track_scan(L, T, tf0, tf1, xk[h], yk[h], g2, bd[h], bt[h]); }
    }
    for (;;) {
        double key = INFINITY; int idx = 0x7fffffff;
        if (bt[0] >= 0) { key = bd[0]; idx = bt[0] * 128 + lane; }
        if (bt[1] >= 0) {
            const int i1 = bt[1] * 128 + lane + 64;
            if (bd[1] < key || (bd[1] == key && i1 < idx)) { key = bd[1]; idx = i1; }
        }
        wave_min2(key, idx);
        if (idx == 0x7fffffff) break;
        const int ts = idx >> 7, ks = idx & 127;
        if (ts < 64) tf0 &= ~(1ull << ts); else tf1 &= ~(1ull << (ts - 64));
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (ks == lane + 64 * h) { L.tm[ts] = ks; unm[h] = false; bt[h] = -1; }
            else if (bt[h] == ts) sim_track_scan(L, T, tf0, tf1, xk[h], yk[h], g2, bd[h], bt[h]);
        }
    }
    __syncthreads();
    // steps 3 and 4: 1 matched, 2 coasting, 3 deleted as tentative, 4 deleted after n_coast misses (0: no track)
    int st[2] = {0, 0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int t = lane + 64 * h;
        if (t < T) {
            const int k = L.tm[t];
            if (k >= 0) {
                fleet::track_update(P, row[h], xp[h], yp[h], sim_track_lds_det(L, k));
                if (assign) assign[k] = (int)row[h].f[fleet::TRK_ID];
                st[h] = 1;
            } else {
                st[h] = 2 + fleet::track_miss(P, row[h], xp[h], yp[h]);
            }
        }
    }
    // step 6: the survivors' rows, then the births
    int pos[2], n = 0, n_matched = 0, del_tent = 0, del_coast = 0, confirmed = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const unsigned long long m = __ballot(st[h] == 1 || st[h] == 2);
        pos[h] = n + __popcll(m & lt); n += __popcll(m);
        n_matched += __popcll(__ballot(st[h] == 1)); del_tent += __popcll(__ballot(st[h] == 3)); del_coast += __popcll(__ballot(st[h] == 4));
        confirmed += __popcll(__ballot(st[h] == 1 && fleet::track_confirmed_now(P, row[h])));
    }
    const int n_surv = n;
    fleet::TrackRow brow[2]; int bpos[2], nb = 0; bool born[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        const unsigned long long m = __ballot(unm[h]);
        const int rank = nb + __popcll(m & lt);
        nb += __popcll(m);
        bpos[h] = n_surv + rank;
        born[h] = unm[h] && bpos[h] < cap;
        brow[h] = fleet::track_born(sim_track_lds_det(L, unm[h] ? k : 0), id0 + (double)rank, tick);
        if (unm[h] && assign) assign[k] = born[h] ? fleet::kTrackUnmatched : fleet::kTrackOverflow;
        confirmed += __popcll(__ballot(born[h] && fleet::track_confirmed_now(P, brow[h])));
    }
    const int n_born = nb < cap - n_surv ? nb : cap - n_surv, overflow = nb - n_born;
    // step 7: positions in the list handed on
    int opos[2], obpos[2], cpos[2], m_out = 0;
    bool lc[2], lb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        lc[h] = st[h] == 1 && fleet::track_confirmed(P, row[h]);
        const unsigned long long m = __ballot(lc[h]);
        opos[h] = m_out + __popcll(m & lt); m_out += __popcll(m);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        lb[h] = born[h] && fleet::track_confirmed(P, brow[h]);
        const unsigned long long m = __ballot(lb[h]);
        obpos[h] = m_out + __popcll(m & lt); m_out += __popcll(m);
    }
    const int n_live_out = m_out;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const unsigned long long m = __ballot(st[h] == 2);
        cpos[h] = m_out + __popcll(m & lt); m_out += __popcll(m);
    }
    const int n_out = m_out < slots ? m_out : slots, out_coast = n_out > n_live_out ? n_out - n_live_out : 0, withheld = m_out - n_out;
    __syncthreads();
    auto hand_on = [&](const fleet::TrackRow& r, int at) {
        double o[6];
        fleet::track_out(r, o);
        const size_t i = (size_t)at * io.stride;
#pragma unroll
        for (int c = 0; c < 6; ++c) io.out[c][i] = o[c];
        if (at == 0 && first) { first[0] = o[0]; first[1] = o[1]; }
    };
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (st[h] == 1 || st[h] == 2) {
#pragma unroll
            for (int c = 0; c < RD; ++c) rows[(size_t)pos[h] * RD + c] = row[h].f[c];
        }
        if (born[h]) {
#pragma unroll
            for (int c = 0; c < RD; ++c) rows[(size_t)bpos[h] * RD + c] = brow[h].f[c];
        }
        if (lc[h] && opos[h] < slots) hand_on(row[h], opos[h]);
        if (lb[h] && obpos[h] < slots) hand_on(brow[h], obpos[h]);
        if (st[h] == 2 && cpos[h] < slots) hand_on(row[h], cpos[h]);
    }
    if (lane == 0) {
        const int n_new = n_surv + n_born;
        *n_trk = n_new; *next_id = id0 + (double)n_born;
        rec[fleet::TRS_TICKS] += 1.0; rec[fleet::TRS_N_DET] += (double)K; rec[fleet::TRS_N_MATCHED] += (double)n_matched;
        rec[fleet::TRS_N_BORN] += (double)n_born; rec[fleet::TRS_N_CONFIRMED] += (double)confirmed; rec[fleet::TRS_N_DEL_TENT] += (double)del_tent;
        rec[fleet::TRS_N_DEL_COAST] += (double)del_coast; rec[fleet::TRS_N_OUT] += (double)n_out; rec[fleet::TRS_N_OUT_COAST] += (double)out_coast;
        rec[fleet::TRS_N_WITHHELD] += (double)withheld; rec[fleet::TRS_N_OVERFLOW] += (double)overflow;
        if ((double)n_new > rec[fleet::TRS_TRACKS_MAX]) rec[fleet::TRS_TRACKS_MAX] = (double)n_new;
    }
    return n_out;
}
__device__ __forceinline__ fleet::TrackParams sim_track_params(const double* q) { return fleet::TrackParams{q[0], q[1], q[2], q[3], q[4]}; }

// behind k_fleet_sim_sense (or telemetry / mates), in front of k_fleet_sim_offsets: the staged list of the planner is replaced by what its
// tracker hands on; sd.cnt and trace [5] .. [7] rewritten as k_fleet_sim_sense rewrites them. g_tx / g_ty are left alone
__global__ __launch_bounds__(64) void k_fleet_sim_track(SimDev sd, SimTrack tk, double* trace /* this tick's records or null */)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    if (!sd.live[p]) return;
    __shared__ TrackLds L;
    const int base = sd.obj_base[p];
    int cnt = sd.cnt[p];
    if (cnt > SIM_OBJ_CAP) cnt = SIM_OBJ_CAP;
    const fleet::TrackParams P = sim_track_params(tk.par + (size_t)p * TRK_PARAMS);
    double* o = trace ? trace + (size_t)p * LTPL_FLEET_SIM_TRACE_DOUBLES : nullptr;
    TrackIo io;
    io.in[0] = io.out[0] = sd.g_x + base; io.in[1] = io.out[1] = sd.g_y + base; io.in[2] = io.out[2] = sd.g_px + base;
    io.in[3] = io.out[3] = sd.g_py + base; io.in[4] = io.out[4] = sd.g_r + base; io.in[5] = io.out[5] = sd.g_v + base;
    io.stride = 1;
    const int n_out = sim_track_tick(lane, P, tk.adv, (double)tk.tick, tk.cap[p], tk.slots[p], tk.rows + (size_t)tk.base[p] * LTPL_FLEET_SIM_TRACK_DOUBLES,
                                     tk.n + p, tk.next_id + p, cnt, io, nullptr, tk.rec + (size_t)p * LTPL_FLEET_SIM_TRACKER_DOUBLES, o ? o + 6 : nullptr, L);
    if (lane != 0) return;
    sd.cnt[p] = n_out;
    if (o) {
        o[5] = (double)n_out;
        if (n_out == 0) { o[6] = NAN; o[7] = NAN; }
    }
}

// the test hook of the rule: one wave per case, the tick of k_fleet_sim_track on the case's own table (in place: tables [q][96][10], n_trk,
// next_id) and detections; cs[q] = capacity, slots
__global__ __launch_bounds__(64) void k_fleet_sim_tracker_eval(const double* par, const double* adv, const uint32_t* tick, const int* cs, double* tables,
                                                               int* n_trk, double* next_id, const int* det_off, const double* dets, double* out,
                                                               int* n_out, int* assign, double* rec)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    __shared__ TrackLds L;
    const int o0 = det_off[q];
    int K = det_off[q + 1] - o0;
    if (K > SIM_OBJ_CAP) K = SIM_OBJ_CAP;      // (refused by the host)
    const fleet::TrackParams P = sim_track_params(par + (size_t)q * TRK_PARAMS);
    TrackIo io;
#pragma unroll
    for (int c = 0; c < 6; ++c) { io.in[c] = dets + (size_t)o0 * 6 + c; io.out[c] = out + (size_t)q * SIM_OBJ_CAP * 6 + c; }
    io.stride = 6;
    const int m = sim_track_tick(lane, P, adv[q], (double)tick[q], cs[2 * q], cs[2 * q + 1], tables + (size_t)q * SIM_OBJ_CAP * LTPL_FLEET_SIM_TRACK_DOUBLES,
                                 n_trk + q, next_id + q, K, io, assign + o0, rec + (size_t)q * LTPL_FLEET_SIM_TRACKER_DOUBLES, nullptr, L);
    if (lane == 0) n_out[q] = m;
}

// ---------------------------------------------------------------------------------------------------------------------
// flight recorder (ltpl_fleet_sim_record, include/ltpl_hip.h): for M chosen planners a full record of every tick, kept in a ring of
// `depth` ticks. Record of (tick, recorded planner m): `stride` doubles at ring + ((tick % depth) M + m) stride --
//   head, REC_HEAD doubles (integers as exact doubles):
//     [0] fleet tick since the recorder was set  [1] planner  [2] error word (PlannerS::err)  [3] selected action  [4] t_now
//     [5] [6] tracked pose x, y  [7] vel_est  [8] heading  [9] objects handed to the planner
//     [10] cut_index_pos  [11] cut_layer  [12] vel_plan  [13] acc_plan  [14] trajectory keys  [15] id pairs
//     [16 + 3 k ..] trajectory key k: key id, trajectory id, rows (untrimmed)        [28 + 2 k ..] id pair k: key id, id value
//     [36] [37] start node (layer, node; -1: none)  [38] const_rows (-1: None)  [39] closest_obj_index (-1: None)  [40] path keys
//     [41 + 4 k ..] path key k: key id, n_rows, n_nodes, red_len                      [57 .. 63] zero
//   objects  [6][96]  column-major: radius, velocity, x, y, predicted x, predicted y of object i at [c][i], list order
//   const    [2][R]   x, y of rows [0, min(const_rows, n_rows of key 0)) of the first path key's path_param (R = cap_rows)
//   traj     [K][7][E] column-major per key: columns s, x, y, psi, kappa, vx, ax of rows [0, min(rows, E)) (E = n_export)
//   nodes    [K][CN][2] int32: the (layer, node) pairs of every path key (CN = cap_nodes, -1 = None)
// K = LTPL_PLANNER_MAX_KEYS. Every section is written column by column with the lanes walking rows: the state's row tables are column-major,
// so loads and stores are contiguous runs. Counts of a planner whose error word is set are zero. What lies behind a count is stale.
// ---------------------------------------------------------------------------------------------------------------------
#define REC_HEAD 64
enum { REC_TICK = 0, REC_PLANNER, REC_ERR, REC_SEL, REC_T_NOW, REC_X, REC_Y, REC_VEL, REC_THETA, REC_N_OBJ, REC_CUT_POS, REC_CUT_LAYER,
       REC_VEL_PLAN, REC_ACC_PLAN, REC_N_TRAJ, REC_N_IDS, REC_TRAJ = 16, REC_IDS = 28, REC_START = 36, REC_CONST_ROWS = 38, REC_CLOSEST,
       REC_N_PATHS, REC_PATHS };
static_assert(LTPL_PLANNER_MAX_KEYS == 4 && REC_TRAJ + 3 * LTPL_PLANNER_MAX_KEYS == REC_IDS && REC_IDS + 2 * LTPL_PLANNER_MAX_KEYS == REC_START &&
              REC_PATHS + 4 * LTPL_PLANNER_MAX_KEYS <= REC_HEAD, "flight recorder: head layout");

struct SimRec {
    const int* planners;                   // [M] recorded planner indices, in the caller's order
    double* ring;                          // [depth][M][stride]
    int M, E;                              // recorded planners; exported rows per trajectory
    size_t stride;                         // doubles per record
    size_t o_obj, o_const, o_traj, o_nodes;     // first double of every section
};
static SimRec sim_rec_layout(const fleet::Dims& D, int n_export)
{
    SimRec r{};
    r.E = n_export;
    r.o_obj = REC_HEAD;
    r.o_const = r.o_obj + (size_t)6 * SIM_OBJ_CAP;
    r.o_traj = r.o_const + (size_t)2 * D.R;
    r.o_nodes = r.o_traj + (size_t)LTPL_PLANNER_MAX_KEYS * 7 * n_export;
    r.stride = (r.o_nodes + (size_t)LTPL_PLANNER_MAX_KEYS * D.CN + 31) / 32 * 32;        // (a pair of int32 per double; records start on 256 bytes)
    return r;
}

// capture P, behind paths_post: what ltpl_fleet_get_paths would return now (Graph_LTPL.py:336-340; the velocity stage trims it afterwards)
__global__ __launch_bounds__(64) void k_fleet_sim_rec_paths(FleetArgs F, SimRec rc, int slot)
{
    const int m = blockIdx.x, lane = threadIdx.x; const WaveX x{lane};
    const int p = rc.planners[m];
    const fleet::Block B{F.state + F.D.stride * (size_t)p, F.D, nullptr};
    __shared__ fleet::PlannerS S;
    fleet_load(x, B, &S);
    constexpr int K = LTPL_PLANNER_MAX_KEYS;
    double* o = rc.ring + ((size_t)slot * rc.M + m) * rc.stride;
    const bool ok = !S.err;
    const int nk = !ok ? 0 : (S.n_last < K ? S.n_last : K);
    if (lane == 0) {
        o[REC_START] = ok && S.has_start ? (double)S.start_node[0] : -1.0; o[REC_START + 1] = ok && S.has_start ? (double)S.start_node[1] : -1.0;
        o[REC_CONST_ROWS] = ok ? (double)S.const_rows : -1.0; o[REC_CLOSEST] = ok ? (double)S.closest_obj_index : -1.0;
        o[REC_N_PATHS] = (double)nk;
    }
    if (lane < 4 * K) {
        const int k = lane >> 2, c = lane & 3;
        double v = 0.0;
        if (k < nk) { const fleet::TrajM& T = S.tm[S.cur_set][S.last_slot[k]]; v = (double)(c == 0 ? T.id : c == 1 ? T.rows : c == 2 ? T.nn : T.red_len); }
        o[REC_PATHS + lane] = v;
    }
    int* nodes = reinterpret_cast<int*>(o + rc.o_nodes);
    for (int k = 0; k < nk; ++k) {
        const int sl = S.last_slot[k]; const fleet::TrajM& T = S.tm[S.cur_set][sl];
        const int room = F.D.CN - T.n0, nn = T.nn < room ? T.nn : room;
        const int* nd = B.nodes(S.cur_set, sl) + (size_t)T.n0 * 2;
        for (int i = lane; i < nn * 2; i += 64) nodes[(size_t)k * F.D.CN * 2 + i] = nd[i];
    }
    if (nk > 0 && S.const_rows > 0) {                                      // TickLogWriter.snapshot_paths: path_param[keys[0]][:const_rows, 0:2]
        const int sl = S.last_slot[0]; const fleet::TrajM& T = S.tm[S.cur_set][sl];
        int n = S.const_rows < T.rows ? S.const_rows : T.rows;
        if (n > F.D.R - T.r0) n = F.D.R - T.r0;
        const fleet::Rows r = B.pp(S.cur_set, sl).from(T.r0);
        double* cx = o + rc.o_const; double* cy = cx + F.D.R;
        for (int i = lane; i < n; i += 64) cx[i] = r.at(i, 0);
        for (int i = lane; i < n; i += 64) cy[i] = r.at(i, 1);
    }
}

// capture V, behind the last kernel of the velocity stage: the simulation's head of the tick, the objects the planner was handed (its slice
// of the tick's object arrays) and what ltpl_fleet_get_trajectories would return now, rows trimmed to n_export, without vel_course
__global__ __launch_bounds__(64) void k_fleet_sim_rec_vel(FleetArgs F, SimDev sd, SimRec rc, int slot, int tick, int pos_stride /* positions per object */)
{
    const int m = blockIdx.x, lane = threadIdx.x; const WaveX x{lane};
    const int p = rc.planners[m];
    const fleet::Block B{F.state + F.D.stride * (size_t)p, F.D, nullptr};
    __shared__ fleet::PlannerS S;
    fleet_load(x, B, &S);
    constexpr int K = LTPL_PLANNER_MAX_KEYS;
    double* o = rc.ring + ((size_t)slot * rc.M + m) * rc.stride;
    const bool ok = !S.err;
    int cnt = ok ? sd.cnt[p] : 0;
    if (cnt > SIM_OBJ_CAP) cnt = SIM_OBJ_CAP;
    const int nb = !ok ? 0 : (S.n_bp < K ? S.n_bp : K), ni = !ok ? 0 : (S.n_ids < K ? S.n_ids : K);
    if (lane == 0) {
        o[REC_TICK] = (double)tick; o[REC_PLANNER] = (double)p; o[REC_ERR] = (double)S.err; o[REC_SEL] = (double)sd.sel[p]; o[REC_T_NOW] = sd.now[p];
        o[REC_X] = sd.pos_x[p]; o[REC_Y] = sd.pos_y[p]; o[REC_VEL] = sd.vel[p]; o[REC_THETA] = sd.theta[p]; o[REC_N_OBJ] = (double)cnt;
        o[REC_CUT_POS] = (double)S.cut_index_pos; o[REC_CUT_LAYER] = (double)S.cut_layer; o[REC_VEL_PLAN] = S.vel_plan; o[REC_ACC_PLAN] = S.acc_plan;
        o[REC_N_TRAJ] = (double)nb; o[REC_N_IDS] = (double)ni;
    }
    if (lane < 3 * K) {
        const int k = lane / 3, c = lane % 3;
        o[REC_TRAJ + lane] = k < nb ? (double)(c == 0 ? S.bp_id[k] : c == 1 ? S.bp_traj_id[k] : S.bp_rows[k]) : 0.0;
    }
    if (lane < 2 * K) {
        const int k = lane >> 1;
        o[REC_IDS + lane] = k < ni ? (double)((lane & 1) ? S.id_val[k] : S.id_key[k]) : 0.0;
    }
    if (lane >= REC_PATHS + 4 * K && lane < REC_HEAD) o[lane] = 0.0;
    {
        const int v0 = sd.veh_off[p];
        double* ob = o + rc.o_obj;
        for (int i = lane; i < cnt; i += 64) {
            const int v = v0 + i;
            ob[i] = sd.o_r[v]; ob[SIM_OBJ_CAP + i] = sd.o_v[v];
            const size_t q = (size_t)pos_stride * v;          // own position and point 1 (the prediction model's further points are not recorded)
            ob[2 * SIM_OBJ_CAP + i] = sd.o_px[q]; ob[3 * SIM_OBJ_CAP + i] = sd.o_py[q];
            ob[4 * SIM_OBJ_CAP + i] = sd.o_px[q + 1]; ob[5 * SIM_OBJ_CAP + i] = sd.o_py[q + 1];
        }
    }
    for (int k = 0; k < nb; ++k) {
        const fleet::Rows r = B.bp(S.bp_slot[k]);
        int n = S.bp_rows[k] < rc.E ? S.bp_rows[k] : rc.E;
        if (n > F.D.R) n = F.D.R;
        double* t = o + rc.o_traj + (size_t)k * 7 * rc.E;
        for (int c = 0; c < 7; ++c) for (int i = lane; i < n; i += 64) t[(size_t)c * rc.E + i] = r.at(i, c);
    }
}

// exclusive scan of the on-track counts (one workgroup; a few hundred thousand planners at most)
__global__ __launch_bounds__(1024) void k_fleet_sim_offsets(const int* cnt, int n, int* veh_off)
{
    __shared__ int part[1024];
    const int t = threadIdx.x, per = (n + 1023) / 1024;
    const int a = t * per, b = a + per < n ? a + per : n;
    int sum = 0;
    for (int i = a; i < b; ++i) sum += cnt[i];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - sum;
    for (int i = a; i < b; ++i) { veh_off[i] = run; run += cnt[i]; }
    if (t == 1023) veh_off[n] = part[1023];
}

// survivors into the fleet's object layout: own position, then the prediction (pos_off[v] = 2 v, written at setup)
__global__ __launch_bounds__(64) void k_fleet_sim_compact(SimDev sd, int n)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    const int base = sd.obj_base[p], o = sd.veh_off[p], c = sd.cnt[p];
    for (int i = 0; i < c; ++i) {
        const int v = o + i, g = base + i;
        sd.o_r[v] = sd.g_r[g]; sd.o_v[v] = sd.g_v[g];
        sd.o_px[2 * v] = sd.g_x[g]; sd.o_py[2 * v] = sd.g_y[g]; sd.o_px[2 * v + 1] = sd.g_px[g]; sd.o_py[2 * v + 1] = sd.g_py[g];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// prediction model (ltpl_fleet_sim_predictor, include/ltpl_hip.h; the rule: fleet_predict.hpp; host mirror: sim.PredictorModel).
// Configuration and a statistics record, no state. While it is set the staging and the tick's object arrays hold 1 + K positions per
// object (pos_off[v] = (1 + K) v) and k_fleet_sim_predict runs in k_fleet_sim_compact's place. The pointers live in a struct of their
// own: no other kernel carries them.
// ---------------------------------------------------------------------------------------------------------------------
#define PRD_PARAMS 4                       // fleet::PredParams
static_assert(fleet::PRS_DOUBLES == LTPL_FLEET_SIM_PREDICTOR_DOUBLES && sizeof(fleet::PredParams) == PRD_PARAMS * sizeof(double) &&
              fleet::kPredMaxPoints == LTPL_FLEET_SIM_PREDICTOR_MAX_POINTS && SIM_OBJ_CAP * 2 <= MAX_POS, "predictor record layout");
struct SimPred {
    const double* par;                     // [N][PRD_PARAMS] in the order of fleet::PredParams
    double* rec;                           // [N][LTPL_FLEET_SIM_PREDICTOR_DOUBLES]
    int K;                                 // points per object
};
struct PredLds { double x[SIM_OBJ_CAP], y[SIM_OBJ_CAP], px[SIM_OBJ_CAP], py[SIM_OBJ_CAP], v[SIM_OBJ_CAP], s0[SIM_OBJ_CAP], d[SIM_OBJ_CAP]; int oc[SIM_OBJ_CAP]; };
// objects in: five arrays (x, y, px, py, v), elements `stride` doubles apart
struct PredIn { const double* c[5]; int stride; };

__device__ __forceinline__ fleet::PredParams sim_pred_params(const double* q) { return fleet::PredParams{q[0], q[1], q[2], q[3]}; }

// The prediction of one planner's `cnt` objects by one wave64 (every lane enters): own position and K points of object i into
// ox / oy[(1 + K) i ..]; `outcome` (or null): per object its outcome; `rec` (or null): the planner's record, updated by lane 0.
// Projection: the wave strides the table's rows per object (coalesced loads, one wave minimum over (d2, row): the exact first minimum),
// then one lane per object decides; points: one lane per (object, point) pair in passes of 64.
__device__ __forceinline__ void sim_predict_wave(int lane, const fleet::PredParams& P, const fleet::PredTable& R, int K, int cnt, const PredIn& in,
                                                 double* ox, double* oy, int* outcome, double* rec, PredLds& L)
{
    for (int i = lane; i < cnt; i += 64) {
        const size_t a = (size_t)i * in.stride;
        L.x[i] = in.c[0][a]; L.y[i] = in.c[1][a]; L.px[i] = in.c[2][a]; L.py[i] = in.c[3][a]; L.v[i] = in.c[4][a];
        L.oc[i] = 0;
    }
    __syncthreads();
    if (P.mode == 2.0) {
        for (int k = 0; k < cnt; ++k) {
            if (!(L.v[k] > 0.0)) continue;             // (still: the row is not read; uniform)
            const double xk = L.x[k], yk = L.y[k];
            double bd = INFINITY; int bi = 0x7fffffff;
            for (int i = lane; i < R.n; i += 64) {
                const double d2 = fleet::pred_d2(xk, yk, R.x[i], R.y[i]);
                if (d2 < bd) { bd = d2; bi = i; }
            }
            wave_min2(bd, bi);
            if (lane == 0) L.oc[k] = bi == 0x7fffffff ? 0 : bi;
        }
        __syncthreads();
    }
    int n_oc[fleet::kPredOutcomes];
#pragma unroll
    for (int c = 0; c < fleet::kPredOutcomes; ++c) n_oc[c] = 0;
    double d_big = 0.0;
    const int stride = 1 + K;
    for (int b0 = 0; b0 < cnt; b0 += 64) {
        const int i = b0 + lane;
        int oc = -1;
        if (i < cnt) {
            const fleet::PredProj o = fleet::pred_project(P, R, L.oc[i], L.x[i], L.y[i], L.px[i], L.py[i], L.v[i]);
            oc = o.outcome;
            L.oc[i] = oc; L.s0[i] = o.s0; L.d[i] = o.d;
            if (oc == fleet::kPredTrack && fleet::pred_abs(o.d) > d_big) d_big = fleet::pred_abs(o.d);
            ox[(size_t)stride * i] = L.x[i]; oy[(size_t)stride * i] = L.y[i];
            if (outcome) outcome[i] = oc;
        }
#pragma unroll
        for (int c = 0; c < fleet::kPredOutcomes; ++c) n_oc[c] += __popcll(__ballot(oc == c));
    }
    __syncthreads();
    int wraps = 0;
    const int pairs = cnt * K;
    for (int b0 = 0; b0 < pairs; b0 += 64) {
        const int q = b0 + lane;
        bool w = false;
        if (q < pairs) {
            const int i = q / K, j = q - i * K + 1;
            const fleet::PredProj o{L.oc[i], L.s0[i], L.d[i]};
            const fleet::PredPoint pt = fleet::pred_point(P, R, K, j, o, L.x[i], L.y[i], L.px[i], L.py[i], L.v[i]);
            ox[(size_t)stride * i + j] = pt.x; oy[(size_t)stride * i + j] = pt.y;
            w = pt.wrapped;
        }
        wraps += __popcll(__ballot(w));
    }
    if (!rec) return;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const double o = __shfl_xor(d_big, m); if (o > d_big) d_big = o; }
    if (lane == 0) {
        rec[fleet::PRS_TICKS] += 1.0; rec[fleet::PRS_N_OBJ] += (double)cnt;
#pragma unroll
        for (int c = 0; c < fleet::kPredOutcomes; ++c) rec[fleet::PRS_OUTCOME0 + c] += (double)n_oc[c];
        if (d_big > rec[fleet::PRS_D_MAX]) rec[fleet::PRS_D_MAX] = d_big;
        rec[fleet::PRS_N_WRAP] += (double)wraps;
    }
}

// behind k_fleet_sim_offsets, in k_fleet_sim_compact's place: the planner's staged survivors into the fleet's object layout at 1 + K
// positions per object. A planner that is not live hands on what it staged (nothing) and leaves its record alone
__global__ __launch_bounds__(64) void k_fleet_sim_predict(SimDev sd, SimPred pd)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    __shared__ PredLds L;
    const int base = sd.obj_base[p], v0 = sd.veh_off[p];
    int cnt = sd.cnt[p];
    if (cnt > SIM_OBJ_CAP) cnt = SIM_OBJ_CAP;
    const fleet::PredTable R{sd.race, sd.race + sd.n_rl, sd.race + (size_t)2 * sd.n_rl, sd.n_rl};
    const PredIn in{{sd.g_x + base, sd.g_y + base, sd.g_px + base, sd.g_py + base, sd.g_v + base}, 1};
    for (int i = lane; i < cnt; i += 64) { sd.o_r[v0 + i] = sd.g_r[base + i]; sd.o_v[v0 + i] = sd.g_v[base + i]; }
    sim_predict_wave(lane, sim_pred_params(pd.par + (size_t)p * PRD_PARAMS), R, pd.K, cnt, in, sd.o_px + (size_t)(1 + pd.K) * v0,
                     sd.o_py + (size_t)(1 + pd.K) * v0, nullptr, sd.live[p] ? pd.rec + (size_t)p * LTPL_FLEET_SIM_PREDICTOR_DOUBLES : nullptr, L);
}

// the test hook of the rule: one wave per case on the fleet's race table; objs[obj_off[q] ..][5] = x, y, px, py, v; out_x / out_y
// [q][96][1 + kPredMaxPoints] (object i of the case from (1 + K) i on), outcome per object, rec[q][LTPL_FLEET_SIM_PREDICTOR_DOUBLES]
__global__ __launch_bounds__(64) void k_fleet_sim_predictor_eval(SimDev sd, const double* par, int K, const int* obj_off, const double* objs, double* out_x,
                                                                 double* out_y, int* outcome, double* rec)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    __shared__ PredLds L;
    const int o0 = obj_off[q];
    int cnt = obj_off[q + 1] - o0;
    if (cnt > SIM_OBJ_CAP) cnt = SIM_OBJ_CAP;      // (refused by the host)
    const fleet::PredTable R{sd.race, sd.race + sd.n_rl, sd.race + (size_t)2 * sd.n_rl, sd.n_rl};
    PredIn in;
#pragma unroll
    for (int c = 0; c < 5; ++c) in.c[c] = objs + (size_t)o0 * 5 + c;
    in.stride = 5;
    constexpr size_t PER = (size_t)SIM_OBJ_CAP * (1 + fleet::kPredMaxPoints);
    sim_predict_wave(lane, sim_pred_params(par + (size_t)q * PRD_PARAMS), R, K, cnt, in, out_x + (size_t)q * PER, out_y + (size_t)q * PER, outcome + o0,
                     rec + (size_t)q * LTPL_FLEET_SIM_PREDICTOR_DOUBLES, L);
}

// ---------------------------------------------------------------------------------------------------------------------
// behaviour selector (ltpl_fleet_sim_selector, include/ltpl_hip.h; the rule: fleet_select.hpp; host mirror: sim.SelectorModel).
// Configuration and a statistics record, no state. While it is set k_fleet_sim_select runs in front of the step kernel and writes an
// ordered copy of every planner's preference list into a buffer of its own (same pref_off); the step kernels get a SimDev whose `pref`
// points there. The user's list is only read. The pointers live in a struct of their own: no other kernel carries them.
// ---------------------------------------------------------------------------------------------------------------------
#define SLC_PARAMS 6                       // fleet::SelParams
static_assert(fleet::SLS_DOUBLES == LTPL_FLEET_SIM_SELECTOR_DOUBLES && sizeof(fleet::SelParams) == SLC_PARAMS * sizeof(double) &&
              fleet::kSelMaxRows == LTPL_FLEET_SIM_MAX_EXPORT && fleet::kSelMaxPref == LTPL_FLEET_SIM_MAX_PREF && fleet::kSelMaxObj == SIM_OBJ_CAP &&
              fleet::kSelEmergency == LTPL_ACT_EMERGENCY && LTPL_ACT_RIGHT == fleet::kSelActions - 1, "selector record layout");
struct SimSel {
    const double* par;                     // [N][SLC_PARAMS] in the order of fleet::SelParams
    const int* on;                         // [N] 0: the planner's list is copied unchanged
    int* ord;                              // the ordered lists, planner p's from pref_off[p] on
    double* rec;                           // [N][LTPL_FLEET_SIM_SELECTOR_DOUBLES]
};
// an action's rows: columns s, x, y, vx of n rows (n < 0: not exported)
struct SelRowsIn { const double* s; const double* x; const double* y; const double* v; int n; };
// objects in: five arrays (x, y, px, py, r), elements `stride` doubles apart
struct SelObjIn { const double* c[5]; int stride; };
struct SelLds {
    double x[fleet::kSelActions][LTPL_FLEET_SIM_MAX_EXPORT], y[fleet::kSelActions][LTPL_FLEET_SIM_MAX_EXPORT], t[fleet::kSelActions][LTPL_FLEET_SIM_MAX_EXPORT];
    double ox[SIM_OBJ_CAP], oy[SIM_OBJ_CAP], opx[SIM_OBJ_CAP], opy[SIM_OBJ_CAP], orad[SIM_OBJ_CAP];
    SelRowsIn rin[fleet::kSelActions];     // filled by the caller
    fleet::SelAct act[fleet::kSelActions];
    int user[8], ord[8], n_r[fleet::kSelActions], last[fleet::kSelActions];
};

__device__ __forceinline__ fleet::SelParams sim_sel_params(const double* q) { return fleet::SelParams{q[0], q[1], q[2], q[3], q[4], q[5]}; }

// One evaluation of the rule by one wave64 (every lane enters; L.rin filled by the caller, no barrier needed behind it): the ordered list
// into ord_out[0 .. n_pref), the four actions into act_out (or null), `rec` (or null) updated by lane 0.
// Times: the time steps of a chunk of 64 rows by one lane each (the first standing row by ballot), then lane a adds up action a's column
// serially -- the written order. Clearance: objects in turn, the window's rows over the lanes, one wave minimum per action on the key
// (d, 256 o + i). Score, order and record: fleet_select.hpp's own functions on the LDS copy.
__device__ __forceinline__ void sim_select_wave(int lane, const fleet::SelParams& P, const int* user, int n_pref, int sel_prev, bool emerg_exported,
                                                int cnt, const SelObjIn& in, int* ord_out, fleet::SelAct* act_out, double* rec, SelLds& L)
{
    if (lane < n_pref) L.user[lane] = user[lane];
    for (int i = lane; i < cnt; i += 64) {
        const size_t a = (size_t)i * in.stride;
        L.ox[i] = in.c[0][a]; L.oy[i] = in.c[1][a]; L.opx[i] = in.c[2][a]; L.opy[i] = in.c[3][a]; L.orad[i] = in.c[4][a];
    }
    __syncthreads();
    unsigned exported = emerg_exported ? 1u << fleet::kSelEmergency : 0u;
    for (int a = 0; a < fleet::kSelActions; ++a) {
        const SelRowsIn r = L.rin[a];
        if (r.n >= 0) exported |= 1u << a;
        bool listed = false;
        for (int e = 0; e < n_pref; ++e) listed = listed || L.user[e] == a;
        const bool scored = listed && r.n >= 2;
        int n_r = r.n;
        if (scored) {
            for (int b0 = 0; b0 < r.n; b0 += 64) {
                const int i = b0 + lane;
                bool stand = false;
                if (i < r.n) {
                    L.x[a][i] = r.x[i]; L.y[a][i] = r.y[i];
                    if (i >= 1) L.t[a][i] = fleet::sel_dt(r.s[i - 1], r.s[i], r.v[i - 1], r.v[i], &stand);
                }
                const unsigned long long m = __ballot(stand);
                if (m) { n_r = b0 + __ffsll((long long)m) - 1; break; }
            }
        }
        if (lane == 0) {
            L.act[a] = fleet::SelAct{(r.n >= 0 ? (int)fleet::kSelExported : 0) | (scored ? (int)fleet::kSelScored : 0), -1, 0.0, INFINITY, 0.0};
            L.n_r[a] = n_r;
        }
    }
    __syncthreads();
    if (lane < fleet::kSelActions && (L.act[lane].flags & fleet::kSelScored)) {
        const SelRowsIn r = L.rin[lane];
        const int n_r = L.n_r[lane];
        const int last = fleet::sel_prefix(L.t[lane], n_r, P.horizon);
        L.last[lane] = last;
        L.act[lane].vbar = fleet::sel_vbar(r.s, r.v[0], L.t[lane], r.n, n_r, last, P.horizon);
    }
    __syncthreads();
    for (int a = 0; a < fleet::kSelActions; ++a) {
        if (!(L.act[a].flags & fleet::kSelScored)) continue;       // (uniform)
        const int last = L.last[a];
        SimBest b{INFINITY, fleet::kSelNone};
        for (int o = 0; o < cnt; ++o) {
            const double ox = L.ox[o], oy = L.oy[o], opx = L.opx[o], opy = L.opy[o], orad = L.orad[o];
            for (int i = lane; i <= last; i += 64) {
                const double t = L.t[a][i];
                if (t <= P.horizon) b = sim_better(b, SimBest{fleet::sel_gap(L.x[a][i], L.y[a][i], t, ox, oy, opx, opy, orad, P.r_ego), o * fleet::kSelMaxRows + i});
            }
        }
        b = sim_wave_min(b);
        if (lane == 0) {
            L.act[a].clear = b.d; L.act[a].clear_obj = b.i == fleet::kSelNone ? -1 : b.i / fleet::kSelMaxRows;
            fleet::sel_score(P, a, sel_prev, &L.act[a]);
        }
    }
    __syncthreads();
    if (lane < n_pref) {
        const int r = fleet::sel_rank(lane, L.user, n_pref, L.act);
        L.ord[r] = L.user[lane]; ord_out[r] = L.user[lane];
    }
    __syncthreads();
    if (lane == 0 && rec) fleet::sel_record(rec, L.user, L.ord, n_pref, L.act, exported, sel_prev);
    if (act_out && lane < fleet::kSelActions) act_out[lane] = L.act[lane];
}

// head of a tick, behind the events kernel and in front of the step kernel: planner p's ordered list from its user list `user`, the
// exported set of the previous tick and the objects staged in it. Copied unchanged, the record left alone: a planner switched off in the
// mask, one that has not started or has its error word set, a one-entry list
__global__ __launch_bounds__(64) void k_fleet_sim_select(FleetArgs F, SimDev sd, SimSel sl)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    __shared__ SelLds L;
    const int off = sd.pref_off[p];
    int n_pref = sd.pref_off[p + 1] - off;
    if (n_pref > LTPL_FLEET_SIM_MAX_PREF) n_pref = LTPL_FLEET_SIM_MAX_PREF;      // (refused by the host)
    const fleet::Block B{F.state + F.D.stride * (size_t)p, F.D, nullptr};
    const fleet::PlannerS* S = B.S();
    if (!sl.on[p] || n_pref < 2 || !sd.started[p] || S->err) {
        if (lane < n_pref) sl.ord[off + lane] = sd.pref[off + lane];
        return;
    }
    int n_bp = S->n_bp;
    if (n_bp > fleet::BPS) n_bp = fleet::BPS;
    bool emerg = false;
    if (lane < fleet::kSelActions) {
        SelRowsIn r{nullptr, nullptr, nullptr, nullptr, -1};
        for (int k = n_bp - 1; k >= 0; --k)             // (the first slot of an id, as the step kernel finds it)
            if (S->bp_id[k] == lane) {
                const fleet::Rows tr = B.bp(S->bp_slot[k]);
                int n = S->bp_rows[k] < sd.n_export ? S->bp_rows[k] : sd.n_export;
                if (n < 0) n = 0;
                r = SelRowsIn{tr.col(0), tr.col(1), tr.col(2), tr.col(5), n};
            }
        L.rin[lane] = r;
    }
    for (int k = 0; k < n_bp; ++k) emerg = emerg || S->bp_id[k] == LTPL_ACT_EMERGENCY;
    int cnt = sd.cnt[p];
    if (cnt > SIM_OBJ_CAP) cnt = SIM_OBJ_CAP;
    if (cnt < 0) cnt = 0;
    const int base = sd.obj_base[p];
    const SelObjIn in{{sd.g_x + base, sd.g_y + base, sd.g_px + base, sd.g_py + base, sd.g_r + base}, 1};
    sim_select_wave(lane, sim_sel_params(sl.par + (size_t)p * SLC_PARAMS), sd.pref + off, n_pref, sd.sel[p], emerg, cnt, in, sl.ord + off, nullptr,
                    sl.rec + (size_t)p * LTPL_FLEET_SIM_SELECTOR_DOUBLES, L);
}

// the test hook of the rule: one wave per case. lists[q][8] = n_pref, sel_prev, emergency exported (0 / 1), the user's entries;
// n_rows[q][4] (-1: not exported); rows[q][4][4][256] = per action the columns s, x, y, vx; objs[obj_off[q] ..][5] = x, y, px, py, r.
// Out: ord[q][5], act[q][4], rec[q][LTPL_FLEET_SIM_SELECTOR_DOUBLES] (in: the record before)
__global__ __launch_bounds__(64) void k_fleet_sim_selector_eval(const double* par, const int* lists, const int* n_rows, const double* rows, const int* obj_off,
                                                                 const double* objs, int* ord, fleet::SelAct* act, double* rec)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    __shared__ SelLds L;
    const int* li = lists + (size_t)q * 8;
    int n_pref = li[0];
    if (n_pref > LTPL_FLEET_SIM_MAX_PREF) n_pref = LTPL_FLEET_SIM_MAX_PREF;      // (refused by the host)
    if (lane < fleet::kSelActions) {
        const double* c = rows + ((size_t)q * fleet::kSelActions + lane) * 4 * LTPL_FLEET_SIM_MAX_EXPORT;
        int n = n_rows[(size_t)q * fleet::kSelActions + lane];
        if (n > LTPL_FLEET_SIM_MAX_EXPORT) n = LTPL_FLEET_SIM_MAX_EXPORT;         // (refused by the host)
        L.rin[lane] = SelRowsIn{c, c + LTPL_FLEET_SIM_MAX_EXPORT, c + 2 * LTPL_FLEET_SIM_MAX_EXPORT, c + 3 * LTPL_FLEET_SIM_MAX_EXPORT, n};
    }
    const int o0 = obj_off[q];
    int cnt = obj_off[q + 1] - o0;
    if (cnt > SIM_OBJ_CAP) cnt = SIM_OBJ_CAP;          // (refused by the host)
    SelObjIn in;
#pragma unroll
    for (int c = 0; c < 5; ++c) in.c[c] = objs + (size_t)o0 * 5 + c;
    in.stride = 5;
    sim_select_wave(lane, sim_sel_params(par + (size_t)q * SLC_PARAMS), li + 3, n_pref, li[1], li[2] != 0, cnt, in, ord + (size_t)q * LTPL_FLEET_SIM_MAX_PREF,
                    act + (size_t)q * fleet::kSelActions, rec + (size_t)q * LTPL_FLEET_SIM_SELECTOR_DOUBLES, L);
}

// ---------------------------------------------------------------------------------------------------------------------
// safety monitor (ltpl_fleet_sim_safety, include/ltpl_hip.h; the rule: fleet_safety.hpp; host mirror: sim.SafetyModel). Measurement only:
// parameters, a record and an incident ring per planner, which the tick writes (they travel with snapshot / branch, fleet_branch.hpp).
// Nothing the planner reads is touched. The pointers live in a struct of their own: no other kernel carries them.
// ---------------------------------------------------------------------------------------------------------------------
#define SAF_PARAMS 5                       // fleet::SafetyParams
#define SAF_RING (LTPL_FLEET_SIM_SAFETY_INCIDENTS * LTPL_FLEET_SIM_SAFETY_INCIDENT_DOUBLES)
static_assert(fleet::SAF_DOUBLES == LTPL_FLEET_SIM_SAFETY_DOUBLES && sizeof(fleet::SafetyParams) == SAF_PARAMS * sizeof(double) &&
              fleet::kSafIncidents == LTPL_FLEET_SIM_SAFETY_INCIDENTS && fleet::SAF_INC_DOUBLES == LTPL_FLEET_SIM_SAFETY_INCIDENT_DOUBLES,
              "safety record layout");
struct SimSafety {
    const double* par;                     // [N][SAF_PARAMS] in the order of fleet::SafetyParams
    const int* on;                         // [N] 0: the planner is not monitored
    double* rec;                           // [N][LTPL_FLEET_SIM_SAFETY_DOUBLES]
    double* inc;                           // [N][SAF_RING]
    uint32_t tick;                         // tick0 + fleet ticks since the monitor was set
};
// objects in: five arrays (x, y, px, py, r), elements `stride` doubles apart. seen_x / seen_y (or null): the PERCEIVED positions next to
// true x, y -- the staged 0.2 s point was built from them, so the rule is handed Q = X + (Q_staged - X_perceived): the true position and
// the perceived displacement. (Q_staged - X_true would put the position error / 0.2 into the object's velocity.)
struct SafObjIn { const double* c[5]; int stride; const double* seen_x; const double* seen_y; };

__device__ __forceinline__ fleet::SafetyParams sim_safety_params(const double* q) { return fleet::SafetyParams{q[0], q[1], q[2], q[3], q[4]}; }

// One live tick of one planner by one wave64 (every lane enters): one lane per object in blocks of 64, each lane folds its objects in slot
// order (fleet::safety_fold), then the wave's reductions -- (value, slot) minima for gap and TTC, plain minima for the headway and, negated,
// for the maxima, ballot / popcount for the counts -- and lane 0 applies the record and incident rules. Registers only: no LDS.
// per_obj [cnt][6] and per_tick [8] (the hook's outputs) or null
__device__ __forceinline__ void sim_safety_wave(int lane, const fleet::SafetyParams& P, double px, double py, double dt, double tick, int cnt,
                                                const SafObjIn& in, double* rec, double* inc, double* per_obj, double* per_tick)
{
    double wx, wy;
    const bool evaluated = fleet::safety_velocity(rec, px, py, dt, &wx, &wy);
    fleet::SafetyTick T = fleet::safety_tick_start();
    int overlaps = 0, skipped = 0;
    for (int b0 = 0; b0 < cnt; b0 += 64) {
        const int k = b0 + lane;
        int fl = 0;
        if (k < cnt) {
            const size_t a = (size_t)k * in.stride;
            const double ox = in.c[0][a], oy = in.c[1][a];
            double qx = in.c[2][a], qy = in.c[3][a];
            if (in.seen_x) { qx = ox + (qx - in.seen_x[a]); qy = oy + (qy - in.seen_y[a]); }      // (uniform)
            const fleet::SafetyObj o = fleet::safety_obj(P, px, py, wx, wy, ox, oy, qx, qy, in.c[4][a]);
            fleet::safety_fold(T, o, k);
            fl = o.flags;
            if (per_obj) {
                double* q = per_obj + (size_t)6 * k;
                q[0] = o.ttc; q[1] = o.drac; q[2] = o.thw; q[3] = o.gap; q[4] = o.closing; q[5] = (double)o.flags;
            }
        }
        overlaps += __popcll(__ballot((fl & fleet::kSafOverlap) != 0));
        skipped += __popcll(__ballot((fl & fleet::kSafSkipped) != 0));
    }
    wave_min2(T.gap, T.gap_slot);
    wave_min2(T.ttc, T.ttc_slot);
    T.thw = wave_min_f64(T.thw);
    T.drac = -wave_min_f64(-T.drac); T.impact = -wave_min_f64(-T.impact); T.closing = -wave_min_f64(-T.closing);
    T.overlaps = overlaps; T.skipped = skipped;
    if (lane != 0) return;
    if (per_tick) fleet::safety_tick_out(T, per_tick);
    fleet::safety_apply(rec, inc, P, px, py, dt, tick, evaluated, T);
}

// behind k_fleet_sim_tele / k_fleet_sim_rank, in front of k_fleet_sim_sense: the staged list as the step and mates kernels left it, in
// front of sensor and tracker. `g_tx`, `g_ty` (null while the noise is off): the true positions of the tick's objects; the displacement to
// the 0.2 s point stays the perceived one (SafObjIn). A planner that is not live or not monitored returns at once
__global__ __launch_bounds__(64) void k_fleet_sim_safety(SimDev sd, SimSafety sf, const double* g_tx, const double* g_ty)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    if (!sd.live[p] || !sf.on[p]) return;
    const int base = sd.obj_base[p], slots = sd.obj_base[p + 1] - base;
    int cnt = sd.cnt[p];
    if (cnt > SIM_OBJ_CAP) cnt = SIM_OBJ_CAP;
    if (cnt > slots) cnt = slots;
    if (cnt < 0) cnt = 0;
    const SafObjIn in{{(g_tx ? g_tx : sd.g_x) + base, (g_tx ? g_ty : sd.g_y) + base, sd.g_px + base, sd.g_py + base, sd.g_r + base}, 1,
                      g_tx ? sd.g_x + base : nullptr, g_tx ? sd.g_y + base : nullptr};
    sim_safety_wave(lane, sim_safety_params(sf.par + (size_t)p * SAF_PARAMS), sd.pos_x[p], sd.pos_y[p], sd.dt, (double)sf.tick, cnt, in,
                    sf.rec + (size_t)p * LTPL_FLEET_SIM_SAFETY_DOUBLES, sf.inc + (size_t)p * SAF_RING, nullptr, nullptr);
}

// the test hook of the rule: one wave per case, the tick's own device function. pose[q][2], dt[q], tick[q], par[q][5],
// objs[obj_off[q] ..][5] = x, y, px, py, r; rec[q][31] and inc[q][8][6] in and out; per_obj[..][6], per_tick[q][8] out
__global__ __launch_bounds__(64) void k_fleet_sim_safety_eval(const double* pose, const double* dt, const int* tick, const double* par, const int* obj_off,
                                                              const double* objs, double* rec, double* inc, double* per_obj, double* per_tick)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    const int o0 = obj_off[q];
    int cnt = obj_off[q + 1] - o0;
    if (cnt > SIM_OBJ_CAP) cnt = SIM_OBJ_CAP;          // (refused by the host)
    if (cnt < 0) cnt = 0;
    SafObjIn in;
#pragma unroll
    for (int c = 0; c < 5; ++c) in.c[c] = objs + (size_t)o0 * 5 + c;
    in.stride = 5; in.seen_x = in.seen_y = nullptr;
    sim_safety_wave(lane, sim_safety_params(par + (size_t)q * SAF_PARAMS), pose[2 * q], pose[2 * q + 1], dt[q], (double)tick[q], cnt, in,
                    rec + (size_t)q * LTPL_FLEET_SIM_SAFETY_DOUBLES, inc + (size_t)q * SAF_RING, per_obj + (size_t)o0 * 6, per_tick + (size_t)q * 8);
}

// ---------------------------------------------------------------------------------------------------------------------
// reactive opponents (ltpl_fleet_sim_react, include/ltpl_hip.h; the rule: fleet_react.hpp; host mirror: sim.ReactModel): parameters, an
// EFFECTIVE vel_scale per opponent and a record per planner, which the tick writes (they travel with snapshot / branch, fleet_branch.hpp).
// While a model is set the step kernels get a SimDev whose opp_scale is `eff`; SimDev::opp_scale stays the configured scale, which the
// events write. The pointers live in a struct of their own: no other kernel carries them.
// ---------------------------------------------------------------------------------------------------------------------
#define RCT_PARAMS LTPL_FLEET_SIM_REACT_PARAMS
#define RCT_BLOCKS ((SIM_OBJ_CAP + 63) / 64)
static_assert(fleet::RCT_DOUBLES == LTPL_FLEET_SIM_REACT_DOUBLES && sizeof(fleet::ReactParams) == RCT_PARAMS * sizeof(double) &&
              fleet::kReactMaxOpp == SIM_OBJ_CAP, "reactive opponents: record layout");
struct SimReact {
    const double* par;                     // [N][RCT_PARAMS] in the order of fleet::ReactParams
    double* eff;                           // the effective scales, in the order of SimDev::opp_s
    double* rec;                           // [N][LTPL_FLEET_SIM_REACT_DOUBLES]
    uint32_t tick;                         // tick0 + fleet ticks since the model was set
};
struct ReactLds { double s[SIM_OBJ_CAP], u[SIM_OBJ_CAP], len[SIM_OBJ_CAP]; };      // what a leader search reads of every opponent

__device__ __forceinline__ fleet::ReactParams sim_react_params(const double* q)
{
    return fleet::ReactParams{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]};
}

// One tick of one planner's `no` opponents by one wave64 (every lane enters). Step 0: the wave strides the table's rows (coalesced loads)
// and ends in the minimum over (d2, row) -- pred_nearest's first minimum; every lane then projects the ego. One lane per opponent in
// blocks of 64: s, c, e, length (elements `stride` doubles apart) are read and s, leader speed and length staged in LDS BEFORE anything
// is written, so e_out may be the array e_in points into; the leader scan of fleet::react_opp is serial in list order. The wave's
// reductions fold the tick's values and lane 0 applies them to the record. per_opp [no][4] and ego_out [3] (the hook's outputs) or null
__device__ __forceinline__ void sim_react_wave(int lane, const fleet::ReactParams& P, const fleet::ReactTable& R, double x, double y, double v, double dt,
                                               double tick, int no, const double* in_s, const double* in_c, const double* in_e, const double* in_len,
                                               int stride, double* e_out, double* rec, double* per_opp, double* ego_out, ReactLds& L)
{
    SimBest b{INFINITY, 0x7fffffff};
    for (int i = lane; i < R.n; i += 64) {
        const double d2 = fleet::pred_d2(x, y, R.x[i], R.y[i]);
        if (d2 < b.d) { b.d = d2; b.i = i; }
    }
    b = sim_wave_min(b);
    const fleet::ReactEgo E = fleet::react_ego(P, R, b.i == 0x7fffffff ? 0 : b.i, x, y, v);
    double cq[RCT_BLOCKS], eq[RCT_BLOCKS], Vq[RCT_BLOCKS];
#pragma unroll
    for (int k = 0; k < RCT_BLOCKS; ++k) {
        const int q = k * 64 + lane;
        cq[k] = 0.0; eq[k] = 0.0; Vq[k] = 0.0;
        if (q < no) {
            const size_t a = (size_t)q * stride;
            const double s = in_s[a];
            cq[k] = in_c[a]; eq[k] = in_e[a]; Vq[k] = fleet::react_vrl(R, s);
            L.s[q] = s; L.u[q] = fleet::react_speed(cq[k], eq[k], Vq[k]); L.len[q] = in_len[a];
        }
    }
    __syncthreads();
    fleet::ReactTick T = fleet::react_tick_start();
#pragma unroll
    for (int k = 0; k < RCT_BLOCKS; ++k) {
        const int q = k * 64 + lane;
        int fl = 0;
        if (q < no) {
            const fleet::ReactOpp o = fleet::react_opp(P, R, E, dt, q, no, L.s, L.u, L.len, cq[k], eq[k], Vq[k]);
            fleet::react_fold(T, o, q);
            fl = o.flags;
            e_out[q] = o.e;
            if (per_opp) { double* w = per_opp + (size_t)4 * q; w[0] = (double)o.leader; w[1] = o.delta; w[2] = o.gap; w[3] = o.acc; }
        }
        T.follow += __popcll(__ballot((fl & fleet::kReactFollow) != 0)); T.ego_lead += __popcll(__ballot((fl & fleet::kReactEgoLead) != 0));
        T.clamped += __popcll(__ballot((fl & fleet::kReactClamped) != 0)); T.overlaps += __popcll(__ballot((fl & fleet::kReactOverlap) != 0));
        T.passive += __popcll(__ballot((fl & fleet::kReactPassive) != 0));
    }
    wave_min2(T.gap, T.gap_slot);
    wave_min2(T.acc, T.acc_slot);
    T.ego_gap = wave_min_f64(T.ego_gap);
    if (lane != 0) return;
    if (ego_out) { ego_out[0] = E.s; ego_out[1] = E.d; ego_out[2] = E.has ? 1.0 : 0.0; }
    fleet::react_apply(rec, E, no, tick, T);
}

// head of a tick, behind the events kernels and k_fleet_sim_select, in front of the step kernel: the effective scales the tick's opponents
// drive with, from the TRUE pose and speed the previous tick left. A planner whose error word is set returns at once; one with on == 0
// hands on its configured scales (an event's write still reaches the step) and leaves its record alone
__global__ __launch_bounds__(64) void k_fleet_sim_react(FleetArgs F, SimDev sd, SimReact rc)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    __shared__ ReactLds L;
    const fleet::Block B{F.state + F.D.stride * (size_t)p, F.D, nullptr};
    if (B.S()->err) return;
    const int o0 = sd.opp_off[p];
    int no = sd.opp_off[p + 1] - o0;
    if (no > SIM_OBJ_CAP) no = SIM_OBJ_CAP;            // (refused by the host)
    const double* par = rc.par + (size_t)p * RCT_PARAMS;
    if (par[0] == 0.0) {
        for (int q = lane; q < no; q += 64) rc.eff[o0 + q] = sd.opp_scale[o0 + q];
        return;
    }
    const size_t n = (size_t)sd.n_rl;
    const fleet::ReactTable R{sd.race, sd.race + n, sd.race + 2 * n, sd.race + 4 * n, sd.n_rl};
    sim_react_wave(lane, sim_react_params(par), R, sd.pos_x[p], sd.pos_y[p], sd.vel[p], sd.dt, (double)rc.tick, no, sd.opp_s + o0, sd.opp_scale + o0,
                   rc.eff + o0, sd.opp_len + o0, 1, rc.eff + o0, rc.rec + (size_t)p * LTPL_FLEET_SIM_REACT_DOUBLES, nullptr, nullptr, L);
}

// the test hook of the rule: one wave per case on the fleet's race table, the tick's own device function. par[q][9], ego[q][3] = x, y, v,
// dt[q], tick[q], opp[opp_off[q] ..][4] = s, c, e, length; rec[q][16] in and out; e_out[..], per_opp[..][4], ego_out[q][3] out
__global__ __launch_bounds__(64) void k_fleet_sim_react_eval(SimDev sd, const double* par, const double* ego, const double* dt, const int* tick,
                                                             const int* opp_off, const double* opp, double* rec, double* e_out, double* per_opp,
                                                             double* ego_out)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    __shared__ ReactLds L;
    const int o0 = opp_off[q];
    int no = opp_off[q + 1] - o0;
    if (no > SIM_OBJ_CAP) no = SIM_OBJ_CAP;            // (refused by the host)
    if (no < 0) no = 0;
    const size_t n = (size_t)sd.n_rl;
    const fleet::ReactTable R{sd.race, sd.race + n, sd.race + 2 * n, sd.race + 4 * n, sd.n_rl};
    const double* o = opp + (size_t)o0 * 4;
    sim_react_wave(lane, sim_react_params(par + (size_t)q * RCT_PARAMS), R, ego[3 * q], ego[3 * q + 1], ego[3 * q + 2], dt[q], (double)tick[q], no, o,
                   o + 1, o + 2, o + 3, 4, e_out + o0, rec + (size_t)q * LTPL_FLEET_SIM_REACT_DOUBLES, per_opp + (size_t)o0 * 4, ego_out + (size_t)3 * q, L);
}

// ---------------------------------------------------------------------------------------------------------------------
// campaign statistics (ltpl_fleet_sim_stats, include/ltpl_hip.h; the rule: fleet_stats.hpp; host mirror: sim.stats_reduce / sim.StatsModel).
// Measurement only: the kernels read the planners' records and write the plan's own buffers, which no kernel of the tick reads
// ---------------------------------------------------------------------------------------------------------------------
static_assert(fleet::STA_DOUBLES == LTPL_FLEET_SIM_STATS_DOUBLES && fleet::kStatsTop == LTPL_FLEET_SIM_STATS_MAX_TOP &&
              fleet::kStatsBins == LTPL_FLEET_SIM_STATS_MAX_BINS && fleet::STA_FAM_STATE == LTPL_SIM_STATS_STATE, "statistics row layout");
#define STA_TOP (2 * LTPL_FLEET_SIM_STATS_MAX_TOP)      // doubles of a top-K list: (value, planner) pairs
struct SimStats {
    int G, M;                              // groups, measures per group
    int spec_stride;                       // the spec of (group g, measure m) is g * spec_stride + m: 0 for a plan (every group the same
                                           // measures), 1 for the hook (M = 1, a spec per case)
    const int* ch_group; const int* ch_first; const int* ch_cnt;    // [chunks] group, first member (an index into `members`) and members
    const int* g_choff;                    // [G + 1] the chunks of group g: g_choff[g] .. g_choff[g + 1] - 1, in ascending member order
    const int* members;                    // the groups' planners, group after group
    const int* ms_fam; const int* ms_col; const int* ms_bins; const int* ms_dir; const int* ms_topk;      // [specs]
    const double* ms_edges;                // [specs][17] fleet::stats_edges
    double* part_row; double* part_top;    // [chunks][M][27], [chunks][M][8][2]
    const double* rec[fleet::STA_FAM_RECORDS];      // the records of the eight families AT THE LAUNCH (null: not referenced)
    const unsigned char* state; size_t state_stride;      // the planners' blocks (fleet::PlannerS in front): STATE / failed
};
struct StatsLds { double v[fleet::kStatsChunk]; int p[fleet::kStatsChunk]; double e[fleet::kStatsBins + 1]; };   // (e: the measure's edges)
struct StatsSpec { const double* e; int bins, top_dir, top_k; };

// the fixed tree of the sum order over the 64 lanes: t[l] + t[l + s] for s = 32 .. 1, as a butterfly -- the add commutes bit for bit, so
// every lane ends with the value the tree leaves in t[0]
__device__ __forceinline__ double sim_stats_tree(double t)
{
    double a, b;
    swap_pair_f64<32>(t, a, b); t = a + b;
    swap_pair_f64<16>(t, a, b); t = a + b;
    t = t + xor_f64<8>(t); t = t + xor_f64<4>(t); t = t + xor_f64<2>(t); t = t + xor_f64<1>(t);
    return t;
}

// One measure of one chunk by one wave64 (every lane enters): the cnt <= 1024 members staged in L (member i by lane i & 63: a lane reads
// what it wrote itself) -> the partial row and top-K list. Counts by ballot / popcount (cell c, under and over are kept by lane c, 16 and
// 17), extrema by wave_min2 on (value, planner) and (-value, planner), sums lane-serial and then the tree, top-K by rounds of wave_min2
// over the keys strictly above the last winner
__device__ __forceinline__ void sim_stats_chunk_wave(int lane, int cnt, const StatsLds& L, const StatsSpec& sp, double* row, double* top)
{
    double s = 0.0, q = 0.0, mn = INFINITY, xk = INFINITY;
    int mp = fleet::kStatsNoPlanner, xp = fleet::kStatsNoPlanner, n = 0, n_nan = 0, n_inf = 0, mine = 0;
    const int rounds = (cnt + 63) >> 6;
    for (int j = 0; j < rounds; ++j) {
        const int i = j * 64 + lane;
        const bool in = i < cnt;
        const double v = in ? L.v[i] : NAN;
        const int p = in ? L.p[i] : fleet::kStatsNoPlanner;
        const bool nan = fleet::stats_nan(v), fin = fleet::stats_finite(v);
        const int cls = in ? fleet::stats_class(v, sp.e, sp.bins) : (int)fleet::kStatsNoClass;
        n_nan += __popcll(__ballot(in && nan)); n_inf += __popcll(__ballot(!nan && !fin)); n += __popcll(__ballot(fin));
        if (fin) { s = s + v; q = q + v * v; }
        if (!nan) {
            if (fleet::stats_before(v, p, mn, mp)) { mn = v; mp = p; }
            if (fleet::stats_before(-v, p, xk, xp)) { xk = -v; xp = p; }
        }
        for (int c = 0; c < fleet::kStatsClasses; ++c) {
            if (c >= sp.bins && c < fleet::kStatsBins) continue;
            const int k = __popcll(__ballot(cls == c));
            if (lane == c) mine += k;
        }
    }
    s = sim_stats_tree(s); q = sim_stats_tree(q);
    wave_min2(mn, mp); wave_min2(xk, xp);
    if (lane == 0) {
        const bool any = mp != fleet::kStatsNoPlanner;
        row[fleet::STA_N] = (double)n; row[fleet::STA_N_NAN] = (double)n_nan; row[fleet::STA_N_INF] = (double)n_inf;
        row[fleet::STA_MIN] = mn; row[fleet::STA_ARGMIN] = any ? (double)mp : -1.0;
        row[fleet::STA_MAX] = -xk; row[fleet::STA_ARGMAX] = any ? (double)xp : -1.0;
        row[fleet::STA_SUM] = s; row[fleet::STA_SUMSQ] = q;
    }
    if (lane < fleet::kStatsBins) row[fleet::STA_HIST + lane] = lane < sp.bins ? (double)mine : 0.0;
    if (lane == fleet::kStatsUnder) row[fleet::STA_UNDER] = (double)mine;
    if (lane == fleet::kStatsOver) row[fleet::STA_OVER] = (double)mine;
    double lk = -INFINITY; int lp = -1;
    bool open = sp.top_dir != 0;
    for (int r = 0; r < fleet::kStatsTop; ++r) {
        double bk = INFINITY; int bp = fleet::kStatsNoPlanner;
        if (open && r < sp.top_k) {
            for (int j = 0; j < rounds; ++j) {
                const int i = j * 64 + lane;
                if (i < cnt) {
                    const double v = L.v[i]; const int p = L.p[i];
                    const double k = fleet::stats_top_key(v, sp.top_dir);
                    if (!fleet::stats_nan(v) && fleet::stats_before(lk, lp, k, p) && fleet::stats_before(k, p, bk, bp)) { bk = k; bp = p; }
                }
            }
            wave_min2(bk, bp);
        }
        open = open && bp != fleet::kStatsNoPlanner;
        if (lane == 0) { top[2 * r] = open ? fleet::stats_top_key(bk, sp.top_dir) : NAN; top[2 * r + 1] = open ? (double)bp : -1.0; }
        lk = bk; lp = bp;
    }
}

__device__ __forceinline__ StatsSpec sim_stats_spec(const SimStats& st, int spec)
{
    return StatsSpec{st.ms_edges + (size_t)spec * (fleet::kStatsBins + 1), st.ms_bins[spec], st.ms_dir[spec], st.ms_topk[spec]};
}

// the records' base and doubles per planner of a family (a chain of uniform selects: the kernel's argument block is never indexed)
__device__ __forceinline__ const double* sim_stats_family(const SimStats& st, int fam, int* stride)
{
    constexpr int D[fleet::STA_FAM_RECORDS] = {LTPL_FLEET_SIM_TELE_DOUBLES, LTPL_FLEET_SIM_VEH_DOUBLES, LTPL_FLEET_SIM_SENSOR_DOUBLES, LTPL_FLEET_SIM_TRACKER_DOUBLES,
                                               LTPL_FLEET_SIM_PREDICTOR_DOUBLES, LTPL_FLEET_SIM_SELECTOR_DOUBLES, LTPL_FLEET_SIM_SAFETY_DOUBLES,
                                               LTPL_FLEET_SIM_REACT_DOUBLES};
    const double* b = nullptr; int d = 0;
#pragma unroll
    for (int k = 0; k < fleet::STA_FAM_RECORDS; ++k) if (fam == k) { b = st.rec[k]; d = D[k]; }
    *stride = d;
    return b;
}

// One workgroup of one wave64 per (group, chunk): the chunk's planners into LDS once, then measure after measure -- the column of the
// family's [N][D] records (a strided read; the lines of a family fetched for one measure serve its later measures from the cache), the
// partial row and list of (chunk, measure). RAW (the hook): the values come from an array in member order
template <bool RAW>
__device__ __forceinline__ void sim_stats_chunk_body(const SimStats& st, const double* raw)
{
    __shared__ StatsLds L;
    const int ch = blockIdx.x, lane = threadIdx.x;
    const int g = st.ch_group[ch], first = st.ch_first[ch], cnt = st.ch_cnt[ch];
    for (int i = lane; i < cnt; i += 64) L.p[i] = st.members[first + i];
    for (int m = 0; m < st.M; ++m) {
        const int spec = g * st.spec_stride + m;
        if constexpr (RAW) {
            for (int i = lane; i < cnt; i += 64) L.v[i] = raw[first + i];
        } else {
            const int fam = st.ms_fam[spec], col = st.ms_col[spec];
            int stride = 0;
            const double* base = sim_stats_family(st, fam, &stride);
            for (int i = lane; i < cnt; i += 64) {
                const size_t p = (size_t)L.p[i];
                if (fam == fleet::STA_FAM_STATE)
                    L.v[i] = reinterpret_cast<const fleet::PlannerS*>(st.state + st.state_stride * p)->err != 0 ? 1.0 : 0.0;
                else L.v[i] = base[p * (size_t)stride + (size_t)col];
            }
        }
        StatsSpec sp = sim_stats_spec(st, spec);
        wave_sync_lds();                   // (the previous measure's compares are done with L.e)
        if (lane <= sp.bins) L.e[lane] = sp.e[lane];
        wave_sync_lds();
        sp.e = L.e;                        // every lane compares against the same 17 doubles: LDS broadcasts, not 34 scalar registers
        const size_t o = (size_t)ch * st.M + m;
        sim_stats_chunk_wave(lane, cnt, L, sp, st.part_row + o * LTPL_FLEET_SIM_STATS_DOUBLES, st.part_top + o * STA_TOP);
    }
}
__global__ __launch_bounds__(64) void k_fleet_sim_stats_chunk(SimStats st) { sim_stats_chunk_body<false>(st, nullptr); }
// the test hook (ltpl_fleet_sim_stats_eval): the same body on raw values; k_fleet_sim_stats_merge follows it as it follows the plan's
__global__ __launch_bounds__(64) void k_fleet_sim_stats_eval(SimStats st, const double* values) { sim_stats_chunk_body<true>(st, values); }

// One wave64 per (group, measure): the partials of the group's chunks folded in ascending chunk order -- lane j < 27 holds column j (counts
// and sums added serially from +0.0, the lanes of min and max fold (value, planner) and write their planner too), then the top-K list by
// rounds of wave_min2 over the chunks' lists
__global__ __launch_bounds__(64) void k_fleet_sim_stats_merge(SimStats st, double* rows, double* tops)
{
    const int g = blockIdx.x / st.M, m = blockIdx.x % st.M, lane = threadIdx.x;
    const int c0 = st.g_choff[g], c1 = st.g_choff[g + 1];
    const StatsSpec sp = sim_stats_spec(st, g * st.spec_stride + m);
    double* row = rows + (size_t)blockIdx.x * LTPL_FLEET_SIM_STATS_DOUBLES;
    double* top = tops + (size_t)blockIdx.x * STA_TOP;
    const double* part = st.part_row + ((size_t)c0 * st.M + m) * LTPL_FLEET_SIM_STATS_DOUBLES;
    const size_t step = (size_t)st.M * LTPL_FLEET_SIM_STATS_DOUBLES;
    if (lane == fleet::STA_MIN || lane == fleet::STA_MAX) {
        const double sign = lane == fleet::STA_MIN ? 1.0 : -1.0;      // the key of the maximum: (-value, planner)
        double bk = INFINITY, bv = sign * INFINITY; int bp = -1;
        for (int c = c0; c < c1; ++c) {
            const double* pr = part + (size_t)(c - c0) * step;
            const double v = pr[lane]; const int p = (int)pr[lane + 1];
            if (p >= 0 && (bp < 0 || fleet::stats_before(sign * v, p, bk, bp))) { bk = sign * v; bv = v; bp = p; }
        }
        row[lane] = bv; row[lane + 1] = (double)bp;
    } else if (lane < LTPL_FLEET_SIM_STATS_DOUBLES && lane != fleet::STA_ARGMIN && lane != fleet::STA_ARGMAX) {
        double a = 0.0;
        for (int c = c0; c < c1; ++c) a = a + part[(size_t)(c - c0) * step + lane];
        row[lane] = a;
    }
    const double* ptop = st.part_top;
    const int entries = (c1 - c0) * fleet::kStatsTop;
    double lk = -INFINITY; int lp = -1;
    bool open = sp.top_dir != 0;
    for (int r = 0; r < fleet::kStatsTop; ++r) {
        double bk = INFINITY; int bp = fleet::kStatsNoPlanner;
        if (open && r < sp.top_k) {
            for (int t = lane; t < entries; t += 64) {
                const double* e = ptop + (((size_t)(c0 + t / fleet::kStatsTop) * st.M + m) * fleet::kStatsTop + (size_t)(t % fleet::kStatsTop)) * 2;
                const int p = (int)e[1];
                if (p >= 0) {
                    const double k = fleet::stats_top_key(e[0], sp.top_dir);
                    if (fleet::stats_before(lk, lp, k, p) && fleet::stats_before(k, p, bk, bp)) { bk = k; bp = p; }
                }
            }
            wave_min2(bk, bp);
        }
        open = open && bp != fleet::kStatsNoPlanner;
        if (lane == 0) { top[2 * r] = open ? fleet::stats_top_key(bk, sp.top_dir) : NAN; top[2 * r + 1] = open ? (double)bp : -1.0; }
        lk = bk; lp = bp;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
struct SimSnaps;                           // snapshot slots (fleet_branch.hpp, ltpl_fleet_sim_snapshot)
static void sim_snaps_free(SimSnaps* s);
struct SimEvents;                           // scripted events (fleet_events.hpp, ltpl_fleet_sim_events)
static void sim_events_free(SimEvents* e);
static int sim_events_check_run(ltpl_fleet* f);                 // before the first launch of a run
static int sim_events_tick(ltpl_fleet* f, FleetTickIn* t);      // head of a tick: the event kernels, t->any_emerg

static void sim_free_list(std::vector<void*>& l)
{
    for (void* p : l) (void)hipFree(p);
    l.clear();
}
// device buffers of a call that become the fleet's only when the whole call succeeded: freed on every early return
struct SimAllocs {
    std::vector<void*> p;
    ~SimAllocs() { sim_free_list(p); }
};

// What the fleet holds of one model: the device buffers of the model's entry point, the argument struct its kernels get, whether the tick
// launches them, and the model's tick count. An entry point allocates everything new into a SimAllocs and calls commit() last, so the
// previous state stays unless every step succeeded; clear() switches the model off. A model without a tick leaves stamp() alone
namespace {                                 // (host helpers of this file: nothing of them is exported)
template <class Dev>
struct SimModule {
    std::vector<void*> allocs;
    Dev dev{};
    bool on = false;
    int tick0 = 0, tick = 0;                // the caller's tick0; ticks of ltpl_fleet_sim_run since the model was set
    void clear(const Dev& off = Dev{}) { sim_free_list(allocs); dev = off; on = false; tick0 = tick = 0; }
    void commit(SimAllocs& a, const Dev& d, int t0 = 0) { sim_free_list(allocs); allocs.swap(a.p); dev = d; on = true; tick0 = t0; tick = 0; }
    // the tick a launch of ltpl_fleet_sim_run stamps into dev.tick: counts on whether or not a planner is live, wraps like a uint32_t
    uint32_t stamp() { return (uint32_t)tick0 + (uint32_t)tick++; }
};
}  // namespace

struct FleetSim {
    std::vector<void*> allocs;
    std::vector<void*> stage_allocs;        // staging slots, the tick's object arrays and obj_base: sized again by ltpl_fleet_sim_race
    std::vector<void*> race_allocs;         // mate_lo / mate_hi / mate_len of ltpl_fleet_sim_race
    SimDev sd{};
    fleet::FObj ob{}; const int* zone_off = nullptr; const int* zone_gid = nullptr;
    FleetTickIn velt;                       // velocity arguments of ltpl_fleet_sim_vel (its own arena)
    bool has_vel = false;
    bool has_mates = false;                 // some race holds more than one planner: k_fleet_sim_mates runs every tick
    bool ran = false;                       // ltpl_fleet_sim_run was called (ltpl_fleet_sim_race comes before it)
    int n_opp = 0, n_obj = 0;
    std::vector<int> own;                   // [N] opponents + statics of planner p
    SimModule<SimTele> tele;                // race-line copies, radius, grid_s, records and progress of ltpl_fleet_sim_telemetry:
                                            // k_fleet_sim_tele (and k_fleet_sim_rank with has_mates) run every tick
    SimModule<SimRec> rec;                  // planner indices and ring of ltpl_fleet_sim_record: k_fleet_sim_rec_paths / k_fleet_sim_rec_vel
                                            // run every tick, on the unfused launch sequence; rec.tick picks the ring's row
    int rec_depth = 0;                      // ring depth
    std::vector<int> rec_planners;          // host copy of the indices
    std::vector<double> rec_host;           // host copy of the ring (ltpl_fleet_sim_record_get), valid until the next run or recorder
    bool rec_host_valid = false;
    std::vector<int> opp_off;               // [N + 1] host copy of sd.opp_off (ltpl_fleet_sim_branch compares opponent counts)
    int tele_gen = 0;                       // counts the calls of ltpl_fleet_sim_telemetry that took effect: a snapshot's telemetry part belongs to one
    SimSnaps* snaps = nullptr;              // allocated by the first ltpl_fleet_sim_snapshot
    std::vector<int> st_off, pref_off;      // [N + 1] host copies of sd.st_off / sd.pref_off (ltpl_fleet_sim_events checks local indices)
    std::vector<int> emerg; int n_emerg = 0;     // [N] host shadow of incl_emerg_traj (stored by ltpl_fleet_sim_vel, followed by the timed events) and its sum
    SimEvents* events = nullptr;            // the event list of ltpl_fleet_sim_events (null: events are off)
    SimModule<SimNoise> noise;              // seeds and sigmas of ltpl_fleet_sim_noise; est_x / est_y / est_v live in `allocs`
                                            // (ltpl_fleet_sim_setup), g_tx / g_ty in the staging. On: the tick launches k_fleet_sim_step_noise /
                                            // k_fleet_sim_mates_noise and reads pos_est / vel_est from noise.dev.est_*
    SimModule<SimVeh> veh;                  // model, parameters and records of ltpl_fleet_sim_vehicle: the tick launches k_fleet_sim_step_veh /
                                            // k_fleet_sim_step_noise_veh
    std::vector<int> veh_model;             // [N] host copy of veh.dev.model (KEEP_STATE; ltpl_fleet_sim_branch compares models)
    SimModule<SimSense> sens;               // parameters, seeds and records of ltpl_fleet_sim_sensor: k_fleet_sim_sense in front of k_fleet_sim_offsets
    std::vector<int> slots;                 // [N] staging slots of planner p (own + mates): the tracker's S_p
    SimModule<SimTrack> trk;                // parameters, tables, counts and records of ltpl_fleet_sim_tracker: k_fleet_sim_track in front of
                                            // k_fleet_sim_offsets
    std::vector<double> trk_par;            // [N][TRK_PARAMS] host copy (ltpl_fleet_sim_race allocates the tables again)
    std::vector<int> trk_cap;               // [N] host copy of trk.dev.cap (ltpl_fleet_sim_branch compares track counts with it)
    SimModule<SimPred> pred;                // parameters and records of ltpl_fleet_sim_predictor: k_fleet_sim_predict in k_fleet_sim_compact's place
    int pos_stride = 2;                     // positions per object of the staging in use: 2, or 1 + K while a predictor is set
    SimModule<SimSel> sel;                  // parameters, mask, ordered lists and records of ltpl_fleet_sim_selector: k_fleet_sim_select in front
                                            // of the step kernel, which walks sel.dev.ord
    bool staged_valid = false;              // cnt and the staging slots hold the list of the last tick (false behind a re-allocation of the
                                            // staging: a run with a selector then starts from empty lists)
    SimModule<SimSafety> saf;               // parameters, mask, records and incident rings of ltpl_fleet_sim_safety: k_fleet_sim_safety behind
                                            // telemetry, in front of the sensor
    SimModule<SimReact> react;              // parameters, effective scales and records of ltpl_fleet_sim_react: k_fleet_sim_react in front of the
                                            // step kernel, which reads react.dev.eff as opp_scale
    SimModule<SimStats> stats;              // the plan of ltpl_fleet_sim_stats (groups, chunks, specs, partials, rows and lists); stats.tick
                                            // counts the fleet's ticks since the plan was set. The records' pointers are filled in at
                                            // every launch (sim_stats_sources): a module that is set again re-allocates its records
    struct StatsPlan {                      // its host part
        int n_chunks = 0, top_k = 0, period = 0, depth = 0;
        std::vector<int> fam;               // [M] the family of every measure
        double* rows = nullptr; double* tops = nullptr;      // [G][M][27], [G][M][8][2] of ltpl_fleet_sim_stats_reduce (in stats.allocs)
        std::vector<void*> ring_allocs;     // the series: [depth][G][M][27], a list of its own (LTPL_SIM_STATS_KEEP_SERIES hands it on)
        double* ring = nullptr;
        std::vector<int32_t> ring_tick;     // [depth] the tick of the row in ring slot i (the host knows it at the launch)
        long long n_rows = 0;               // rows ever written
    } sp;
};
static void fleet_sim_free(FleetSim* s)
{
    if (!s) return;
    sim_snaps_free(s->snaps);
    sim_events_free(s->events);
    sim_free_list(s->stage_allocs); sim_free_list(s->race_allocs);
    s->tele.clear(); s->rec.clear(); s->noise.clear(); s->veh.clear(); s->sens.clear(); s->trk.clear(); s->pred.clear(); s->sel.clear();
    s->saf.clear(); s->react.clear(); s->stats.clear(); sim_free_list(s->sp.ring_allocs);
    for (void* p : s->allocs) (void)hipFree(p);
    if (s->velt.d_buf) (void)hipFree(s->velt.d_buf);
    delete s;
}

template <class T>
static int sim_upload(ltpl_fleet* f, std::vector<void*>& allocs, const T* src, size_t n, T** out)
{
    void* p = nullptr;
    FLEET_TRY(f, hipMalloc(&p, (n ? n : 1) * sizeof(T)));
    allocs.push_back(p);
    if (src && n) FLEET_TRY(f, hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    else FLEET_TRY(f, hipMemset(p, 0, (n ? n : 1) * sizeof(T)));
    *out = static_cast<T*>(p);
    return LTPL_OK;
}
template <class T>
static int sim_upload(ltpl_fleet* f, FleetSim* s, const T* src, size_t n, T** out) { return sim_upload(f, s->allocs, src, n, out); }

// one per-planner column of a model's ltpl_fleet_sim_*_in: its name in the messages and its values, doubles or integers
struct SimCol {
    const char* name; const double* d = nullptr; const int32_t* i = nullptr;
    SimCol(const char* n, const double* p) : name(n), d(p) {}
    SimCol(const char* n, const int32_t* p) : name(n), i(p) {}
    double at(int p) const { return d ? d[p] : (double)i[p]; }
};
// Gathers the columns into the model's [N][P] parameter table *par, the one the entry point uploads, and checks it on the way:
// "fleet sim <what>: <name> missing" for a column that is not there, then head() (the entry point's checks that come between the two:
// null, or what is wrong), then row_ok(p, row, &why) for every planner, reported as "... planner <p>: <why>". The rules stay the model's
template <size_t P, class Head, class RowOk>
static int sim_param_table(ltpl_fleet* f, const char* what, const SimCol (&col)[P], Head head, RowOk row_ok, std::vector<double>* par)
{
    auto bad = [&](const std::string& why) { f->err = std::string("fleet sim ") + what + ": " + why; return LTPL_ERR_INVALID_ARG; };
    for (const SimCol& c : col) if (!c.d && !c.i) return bad(std::string(c.name) + " missing");
    if (const char* why = head()) return bad(why);
    const int N = f->D.N;
    par->resize((size_t)N * P);
    for (int p = 0; p < N; ++p) {
        double* q = par->data() + (size_t)p * P;
        for (size_t c = 0; c < P; ++c) q[c] = col[c].at(p);
        std::string why;
        if (!row_ok(p, q, &why)) return bad("planner " + std::to_string(p) + ": " + why);
    }
    return LTPL_OK;
}
static const char* sim_no_head() { return nullptr; }

// The shape the _read entry points share. Before the first HIP call, in this order: simulation present, model on (`off`: what the refusal
// says), `out` present, record size, then extra(), the entry point's checks of its further outputs (0: fine). Then the device, the
// stream and the N records of the model
template <class Dev, class Extra>
static int sim_read_records(ltpl_fleet* f, const char* what, SimModule<Dev> FleetSim::* mod, const char* off, double* out, const char* out_name,
                            int32_t doubles_per_planner, int32_t record_doubles, Extra extra)
{
    auto bad = [&](const std::string& why) { f->err = std::string("fleet sim ") + what + ": " + why; return LTPL_ERR_INVALID_ARG; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    const SimModule<Dev>& m = f->sim->*mod;
    if (!m.on) return bad(off);
    if (!out) return bad(std::string(out_name) + " missing");
    if (doubles_per_planner != record_doubles) return bad("record size mismatch");
    if (int rc = extra()) return rc;
    FLEET_TRY(f, hipSetDevice(f->h->device));
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FLEET_TRY(f, hipMemcpy(out, m.dev.rec, sizeof(double) * (size_t)f->D.N * (size_t)record_doubles, hipMemcpyDeviceToHost));
    return LTPL_OK;
}
template <class Dev>
static int sim_read_records(ltpl_fleet* f, const char* what, SimModule<Dev> FleetSim::* mod, const char* off, double* out, int32_t doubles_per_planner,
                            int32_t record_doubles)
{
    return sim_read_records(f, what, mod, off, out, "out", doubles_per_planner, record_doubles, [] { return 0; });
}

// The device block of a test hook (ltpl_fleet_sim_*_eval and their kin): one hipMalloc, freed on every return. in / out / inout declare
// the arrays by element count and return references that turn into device pointers once upload() has run; an array of 0 elements still
// gets an address of its own, and is neither copied in nor fetched.
// Order, the same for every hook: upload() zeroes the whole block, copies the inputs in and synchronises the stream; the hook launches;
// fetch() queues the copies back behind the kernel and finish() waits for them. All of it runs on the fleet's stream, so the stream's
// order is the only one needed; the synchronisation in front of the launch keeps the kernel from starting while the runtime may still
// read a caller's pageable array. (Blocking hipMemset / hipMemcpy on the null stream, as the hooks once did, are correct as well: the
// fleet's stream does not wait for the null stream, but a blocking copy returns with its bytes, and what was queued before it, in place.)
namespace {
class SimHookBlock {
public:
    template <class T> struct Ref {
        const SimHookBlock* b; size_t off;
        T* get() const { return reinterpret_cast<T*>(b->d_ + off); }
        operator T*() const { return get(); }
    };
    explicit SimHookBlock(ltpl_fleet* f) : f_(f) {}
    SimHookBlock(const SimHookBlock&) = delete;
    SimHookBlock& operator=(const SimHookBlock&) = delete;
    ~SimHookBlock() { if (d_) (void)hipFree(d_); }
    template <class T> Ref<const T> in(const T* host, size_t count) { return {this, add(host, count * sizeof(T))}; }
    template <class T> Ref<T> out(size_t count) { return {this, add(nullptr, count * sizeof(T))}; }
    template <class T> Ref<T> inout(const T* host, size_t count) { return {this, add(host, count * sizeof(T))}; }
    int upload()
    {
        hipStream_t st = f_->h->stream;
        FLEET_TRY(f_, hipMalloc(reinterpret_cast<void**>(&d_), ar_.size));
        FLEET_TRY(f_, hipMemsetAsync(d_, 0, ar_.size, st));
        for (const Copy& c : copies_) FLEET_TRY(f_, hipMemcpyAsync(d_ + c.off, c.host, c.bytes, hipMemcpyHostToDevice, st));
        FLEET_TRY(f_, hipStreamSynchronize(st));
        return LTPL_OK;
    }
    template <class T, class U>
    int fetch(T* host, Ref<U> dev, size_t count)
    {
        static_assert(std::is_same<T, typename std::remove_const<U>::type>::value, "the host array has the device array's element type");
        if (count) FLEET_TRY(f_, hipMemcpyAsync(host, dev.get(), count * sizeof(T), hipMemcpyDeviceToHost, f_->h->stream));
        return LTPL_OK;
    }
    int finish()
    {
        FLEET_TRY(f_, hipStreamSynchronize(f_->h->stream));
        return LTPL_OK;
    }
private:
    struct Copy { size_t off; const void* host; size_t bytes; };
    size_t add(const void* host, size_t bytes)
    {
        const size_t off = ar_.add(bytes ? bytes : 1);
        if (host && bytes) copies_.push_back(Copy{off, host, bytes});
        return off;
    }
    ltpl_fleet* f_;
    Arena ar_;                              // (arrays start on cache-line multiples)
    std::vector<Copy> copies_;
    unsigned char* d_ = nullptr;
};
}  // namespace

// staging slots of every planner from obj_base[p] on (slots[p] of them) and the tick's object arrays of the fleet (pos_off[v] = stride v;
// stride 2: own position and the ingestion's point; 1 + K with a prediction model):
// allocated by sim_stage_alloc into a list of their own, which sim_stage_commit hands to the fleet (freeing the previous staging)
struct SimStage {
    SimAllocs a;
    int* obj_base = nullptr; int* pos_off = nullptr; int stride = 2;
    double* g[8] = {};                      // g_x, g_y, g_px, g_py, g_r, g_v; g_tx, g_ty (written and read only while sensor noise is set)
    double* o[4] = {};                      // o_r, o_v, o_px, o_py
};
static int sim_stage_alloc(ltpl_fleet* f, const std::vector<int>& slots, int stride, SimStage* st)
{
    st->stride = stride;
    const int N = f->D.N;
    std::vector<int> base((size_t)N + 1);  // (entry N: the total; ltpl_fleet_sim_branch takes a planner's slot count from it)
    int total = 0;
    for (int p = 0; p < N; ++p) { base[(size_t)p] = total; total += slots[(size_t)p]; }
    base[(size_t)N] = total;
    std::vector<int> pos_off((size_t)total + 1);
    for (int v = 0; v <= total; ++v) pos_off[(size_t)v] = stride * v;
    int rc;
    const double* z = nullptr;
#define SIM_UP(dst, src, n) do { if ((rc = sim_upload(f, st->a.p, src, (size_t)(n), &dst))) return rc; } while (0)
    SIM_UP(st->obj_base, base.data(), N + 1);
    for (double*& g : st->g) SIM_UP(g, z, total);
    SIM_UP(st->pos_off, pos_off.data(), total + 1);
    SIM_UP(st->o[0], z, total); SIM_UP(st->o[1], z, total); SIM_UP(st->o[2], z, (size_t)stride * total); SIM_UP(st->o[3], z, (size_t)stride * total);
#undef SIM_UP
    return LTPL_OK;
}
static void sim_stage_commit(FleetSim* s, SimStage* st)
{
    sim_free_list(s->stage_allocs);
    s->stage_allocs.swap(st->a.p);
    SimDev& d = s->sd;
    d.obj_base = st->obj_base;
    d.g_x = st->g[0]; d.g_y = st->g[1]; d.g_px = st->g[2]; d.g_py = st->g[3]; d.g_r = st->g[4]; d.g_v = st->g[5];
    d.o_r = st->o[0]; d.o_v = st->o[1]; d.o_px = st->o[2]; d.o_py = st->o[3];
    s->noise.dev.g_tx = st->g[6]; s->noise.dev.g_ty = st->g[7];
    s->pos_stride = st->stride;
    s->staged_valid = false;                // (the new staging holds no list: see FleetSim::staged_valid)
    s->ob = fleet::FObj{d.prev_action, d.t_now, d.veh_off, st->pos_off, d.o_r, d.o_v, d.o_px, d.o_py};
}

// the tracker's device arrays for the staging slots `slots`: empty tables, next_id 0, fresh statistics. Allocated into `al`; the caller
// commits with sim_tracker_commit (which starts the tick count at tick0) once everything else of its call succeeded
struct SimTrackNew { SimAllocs al; SimTrack tk{}; std::vector<int> cap; };
static int sim_tracker_alloc(ltpl_fleet* f, const std::vector<int>& slots, const std::vector<double>& par, SimTrackNew* t)
{
    const size_t N = (size_t)f->D.N;
    std::vector<int> base(N);
    t->cap.resize(N);
    size_t total = 0;
    for (size_t p = 0; p < N; ++p) {
        base[p] = (int)total;
        t->cap[p] = 2 * slots[p] < SIM_OBJ_CAP ? 2 * slots[p] : SIM_OBJ_CAP;
        total += (size_t)t->cap[p];
    }
    int rc;
    double* d_par = nullptr; int* d_base = nullptr; int* d_cap = nullptr; int* d_slots = nullptr;
    if ((rc = sim_upload(f, t->al.p, par.data(), par.size(), &d_par))) return rc;
    if ((rc = sim_upload(f, t->al.p, base.data(), N, &d_base))) return rc;
    if ((rc = sim_upload(f, t->al.p, t->cap.data(), N, &d_cap))) return rc;
    if ((rc = sim_upload(f, t->al.p, slots.data(), N, &d_slots))) return rc;
    t->tk.par = d_par; t->tk.base = d_base; t->tk.cap = d_cap; t->tk.slots = d_slots;
    if ((rc = sim_upload(f, t->al.p, (const double*)nullptr, total * LTPL_FLEET_SIM_TRACK_DOUBLES, &t->tk.rows))) return rc;
    if ((rc = sim_upload(f, t->al.p, (const int*)nullptr, N, &t->tk.n))) return rc;
    if ((rc = sim_upload(f, t->al.p, (const double*)nullptr, N, &t->tk.next_id))) return rc;
    if ((rc = sim_upload(f, t->al.p, (const double*)nullptr, N * LTPL_FLEET_SIM_TRACKER_DOUBLES, &t->tk.rec))) return rc;
    t->tk.adv = f->sim->sd.dt / 0.2;       // the one division of the rule (fleet_track.hpp)
    return LTPL_OK;
}
static void sim_tracker_commit(FleetSim* s, SimTrackNew* t, int tick0)
{
    s->trk.commit(t->al, t->tk, tick0);
    s->trk_cap.swap(t->cap);
}

static int sim_check_csr(ltpl_fleet* f, const int32_t* off, int N, const char* what, int* total)
{
    if (!off) { f->err = std::string("fleet sim: ") + what + " offsets missing"; return LTPL_ERR_INVALID_ARG; }
    if (off[0] != 0) { f->err = std::string("fleet sim: ") + what + " offsets must start at 0"; return LTPL_ERR_INVALID_ARG; }
    for (int p = 0; p < N; ++p) if (off[p + 1] < off[p]) { f->err = std::string("fleet sim: ") + what + " offsets must not decrease"; return LTPL_ERR_INVALID_ARG; }
    *total = off[N];
    return LTPL_OK;
}

// every argument is checked before the first HIP call
static int sim_check_in(ltpl_fleet* f, const ltpl_fleet_sim_in* in, int* n_opp, int* n_st, int* n_pref, int* n_zone)
{
    const int N = f->D.N;
    auto bad = [&](const char* why, int code = LTPL_ERR_INVALID_ARG) { f->err = std::string("fleet sim: ") + why; return code; };
    if (in->n_rl < 2 || !in->race) return bad("race-line table with fewer than 2 rows");
    for (int i = 0; i + 1 < in->n_rl; ++i) if (!(in->race[(size_t)5 * (i + 1)] >= in->race[(size_t)5 * i])) return bad("s_rl must not decrease");
    int rc;
    if ((rc = sim_check_csr(f, in->opp_off, N, "opponent", n_opp))) return rc;
    if ((rc = sim_check_csr(f, in->static_off, N, "static object", n_st))) return rc;
    if ((rc = sim_check_csr(f, in->pref_off, N, "preference", n_pref))) return rc;
    if ((rc = sim_check_csr(f, in->zone_off, N, "zone", n_zone))) return rc;
    if (*n_opp > 0 && (!in->opp_s0 || !in->opp_vel_scale || !in->opp_length)) return bad("opponent arrays missing");
    if (*n_st > 0 && (!in->static_x || !in->static_y || !in->static_theta || !in->static_v || !in->static_length)) return bad("static object arrays missing");
    for (int p = 0; p < N; ++p) {
        if ((in->opp_off[p + 1] - in->opp_off[p]) + (in->static_off[p + 1] - in->static_off[p]) > SIM_OBJ_CAP)
            return bad("more than 96 objects for one planner", LTPL_ERR_CAPACITY);
        const int np_ = in->pref_off[p + 1] - in->pref_off[p];
        if (np_ < 1 || np_ > LTPL_FLEET_SIM_MAX_PREF) return bad("a preference list needs 1 .. 5 entries");
    }
    if (!in->pref_action) return bad("preference actions missing");
    for (int i = 0; i < *n_pref; ++i) if (in->pref_action[i] < LTPL_ACT_STRAIGHT || in->pref_action[i] > LTPL_ACT_EMERGENCY) return bad("unknown action in a preference list");
    if (*n_zone > 0 && !in->zone_gid) return bad("zone node ids missing");
    for (int i = 0; i < *n_zone; ++i) if (in->zone_gid[i] < 0 || in->zone_gid[i] >= f->h->lat.V) return bad("zone node id out of range");
    if (!(in->dt > 0.0) || !std::isfinite(in->dt) || !std::isfinite(in->t0) || !std::isfinite(in->tic0)) return bad("dt must be positive, t0 / tic0 finite");
    if (in->n_export < 1 || in->n_export > LTPL_FLEET_SIM_MAX_EXPORT) return bad("n_export must be 1 .. 256", LTPL_ERR_CAPACITY);
    if (!in->pos_est_x || !in->pos_est_y || !in->vel_est) return bad("initial pose estimate missing");
    return LTPL_OK;
}

extern "C" int ltpl_fleet_sim_setup(ltpl_fleet* f, const ltpl_fleet_sim_in* in)
try {
    if (!f || !in) return LTPL_ERR_INVALID_ARG;
    int n_opp = 0, n_st = 0, n_pref = 0, n_zone = 0;
    int rc = sim_check_in(f, in, &n_opp, &n_st, &n_pref, &n_zone);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    fleet_sim_free(f->sim); f->sim = nullptr;
    std::unique_ptr<FleetSim, void (*)(FleetSim*)> s(new FleetSim(), fleet_sim_free);
    const int N = f->D.N, n_obj = n_opp + n_st;
    s->n_opp = n_opp; s->n_obj = n_obj;
    s->opp_off.assign(in->opp_off, in->opp_off + N + 1);
    s->st_off.assign(in->static_off, in->static_off + N + 1); s->pref_off.assign(in->pref_off, in->pref_off + N + 1);
    SimDev& d = s->sd;
    d.n_rl = in->n_rl; d.dt = in->dt; d.n_export = in->n_export;
    {
        std::vector<double> race((size_t)5 * in->n_rl);             // column-major on the device
        for (int i = 0; i < in->n_rl; ++i) for (int c = 0; c < 5; ++c) race[(size_t)c * in->n_rl + i] = in->race[(size_t)5 * i + c];
        double* p = nullptr;
        if ((rc = sim_upload(f, s.get(), race.data(), race.size(), &p))) return rc;
        d.race = p;
    }
    const std::vector<double> tic(n_opp, in->tic0), now(N, in->t0);
    const std::vector<int> sel(N, LTPL_ACT_NONE);
    s->own.resize((size_t)N);
    for (int p = 0; p < N; ++p) s->own[(size_t)p] = (in->opp_off[p + 1] - in->opp_off[p]) + (in->static_off[p + 1] - in->static_off[p]);
    int* pi = nullptr; double* pd = nullptr;
#define SIM_UP(dst, src, n) do { if ((rc = sim_upload(f, s.get(), src, (size_t)(n), &dst))) return rc; } while (0)
    SIM_UP(pi, in->opp_off, N + 1); d.opp_off = pi;
    SIM_UP(d.opp_s, in->opp_s0, n_opp); SIM_UP(d.opp_tic, tic.data(), n_opp);
    SIM_UP(pd, in->opp_vel_scale, n_opp); d.opp_scale = pd; SIM_UP(pd, in->opp_length, n_opp); d.opp_len = pd;
    SIM_UP(pi, in->static_off, N + 1); d.st_off = pi;
    SIM_UP(pd, in->static_x, n_st); d.st_x = pd; SIM_UP(pd, in->static_y, n_st); d.st_y = pd; SIM_UP(pd, in->static_theta, n_st); d.st_th = pd;
    SIM_UP(pd, in->static_v, n_st); d.st_v = pd; SIM_UP(pd, in->static_length, n_st); d.st_len = pd;
    SIM_UP(pi, in->pref_off, N + 1); d.pref_off = pi; SIM_UP(pi, in->pref_action, n_pref); d.pref = pi;
    SIM_UP(d.now, now.data(), N); SIM_UP(d.sel, sel.data(), N); SIM_UP(d.started, (const int*)nullptr, N);
    SIM_UP(d.pos_x, in->pos_est_x, N); SIM_UP(d.pos_y, in->pos_est_y, N); SIM_UP(d.vel, in->vel_est, N);
    SIM_UP(d.theta, (const double*)nullptr, N); SIM_UP(d.live, (const int*)nullptr, N);
    SIM_UP(d.cnt, (const int*)nullptr, N);
    SIM_UP(s->noise.dev.est_x, in->pos_est_x, N); SIM_UP(s->noise.dev.est_y, in->pos_est_y, N); SIM_UP(s->noise.dev.est_v, in->vel_est, N);
    SIM_UP(d.prev_action, sel.data(), N); SIM_UP(d.t_now, now.data(), N); SIM_UP(d.veh_off, (const int*)nullptr, N + 1);
    int* zo = nullptr; int* zg = nullptr;
    SIM_UP(zo, in->zone_off, N + 1); SIM_UP(zg, in->zone_gid, n_zone);
#undef SIM_UP
    {
        SimStage st;
        if ((rc = sim_stage_alloc(f, s->own, 2, &st))) return rc;
        sim_stage_commit(s.get(), &st);
        s->slots = s->own;
    }
    s->zone_off = zo; s->zone_gid = zg;
    f->sim = s.release();
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_vel(ltpl_fleet* f, const ltpl_planner_vel_in* in)
try {
    if (!f || !in) return LTPL_ERR_INVALID_ARG;
    if (!f->sim) { f->err = "fleet sim: ltpl_fleet_sim_setup first"; return LTPL_ERR_INVALID_ARG; }
    if (in->gg_row_off || in->gg_rows) { f->err = "fleet sim: local_gg as a dict depends on the tick's own paths (not supported by the simulation)"; return LTPL_ERR_UNSUPPORTED; }
    int rc = fleet_enter(f);
    if (rc) return rc;
    // pos_est / vel_est come from the simulation: stand-ins for the checks of the packer
    const std::vector<double> zero((size_t)f->D.N, 0.0);
    ltpl_planner_vel_in v = *in;
    v.pos_est_x = v.pos_est_y = v.vel_est = zero.data();
    f->sim->has_vel = false;
    if ((rc = fleet_pack_inputs(f, &f->sim->velt, nullptr, &v, false))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    f->sim->emerg.assign((size_t)f->D.N, 0); f->sim->n_emerg = 0;
    if (in->incl_emerg_traj) for (int p = 0; p < f->D.N; ++p) f->sim->n_emerg += (f->sim->emerg[(size_t)p] = in->incl_emerg_traj[p] ? 1 : 0);
    f->sim->has_vel = true;
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

static int sim_stats_sources(ltpl_fleet* f, SimStats* st);        // the records' pointers of this moment; refuses a family that is off
static int sim_stats_series_row(ltpl_fleet* f, uint32_t tick);    // the two statistics kernels into the next row of the ring

extern "C" int ltpl_fleet_sim_run(ltpl_fleet* f, int32_t n_ticks, double* trace, int32_t doubles_per_tick_planner, float* ms_total)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    if (n_ticks < 1) { f->err = "fleet sim: n_ticks must be positive"; return LTPL_ERR_INVALID_ARG; }
    if (trace && doubles_per_tick_planner != LTPL_FLEET_SIM_TRACE_DOUBLES) { f->err = "fleet sim: trace record size mismatch"; return LTPL_ERR_INVALID_ARG; }
    if (!f->sim || !f->sim->has_vel) { f->err = "fleet sim: ltpl_fleet_sim_setup and ltpl_fleet_sim_vel first"; return LTPL_ERR_INVALID_ARG; }
    int rc = sim_events_check_run(f);
    if (rc) return rc;
    if (f->sim->stats.on && f->sim->sp.period > 0) {             // a series over a family that is off: refused before the first tick
        SimStats probe = f->sim->stats.dev;
        if ((rc = sim_stats_sources(f, &probe))) return rc;
    }
    if ((rc = fleet_enter(f))) return rc;
    FleetSim& s = *f->sim;
    const int N = f->D.N;
    const size_t rec = (size_t)N * LTPL_FLEET_SIM_TRACE_DOUBLES;
    double* d_trace = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct Guard { double** t; hipEvent_t* a; hipEvent_t* b; ~Guard() { if (*t) (void)hipFree(*t); if (*a) (void)hipEventDestroy(*a); if (*b) (void)hipEventDestroy(*b); } } g{&d_trace, &e0, &e1};
    if (trace) FLEET_TRY(f, hipMalloc(reinterpret_cast<void**>(&d_trace), sizeof(double) * rec * (size_t)n_ticks));
    FLEET_TRY(f, hipEventCreate(&e0)); FLEET_TRY(f, hipEventCreate(&e1));
    FleetTickIn t = s.velt;
    // the emergency stage's launches follow the host's shadow of incl_emerg_traj: ltpl_fleet_sim_vel stores it (the same OR as
    // velt.any_emerg then), timed events change it, and what they wrote stays after the list is switched off
    t.any_emerg = s.n_emerg > 0 ? 1 : 0;
    t.ob = s.ob; t.zone_off = s.zone_off; t.zone_gid = s.zone_gid;
    t.vin.pos_x = s.sd.pos_x; t.vin.pos_y = s.sd.pos_y; t.vin.vel_est = s.sd.vel;
    SimNoise& nz = s.noise.dev;
    if (s.noise.on) { t.vin.pos_x = nz.est_x; t.vin.pos_y = nz.est_y; t.vin.vel_est = nz.est_v; }   // get_ref_idx and the velocity stage see the estimate
    // g_tx / g_ty of the staging for telemetry, the safety monitor and the sensor (written and read only while sensor noise is set)
    double* const g_tx = s.noise.on ? nz.g_tx : nullptr; double* const g_ty = s.noise.on ? nz.g_ty : nullptr;
    t.has_paths = true;
    hipStream_t st = f->h->stream;
    s.ran = true;
    s.rec_host_valid = false;
    FLEET_TRY(f, hipStreamSynchronize(st));
    FLEET_TRY(f, hipEventRecord(e0, st));
    // a selector reads the previous tick's staged list at the head of the tick: behind a re-allocation of the staging there is none
    if (s.sel.on && !s.staged_valid) FLEET_TRY(f, hipMemsetAsync(s.sd.cnt, 0, sizeof(int) * (size_t)N, st));
    s.staged_valid = true;
    SimDev sds = s.sd;                      // what the step and mates kernels get: the selector's ordered lists in the user's place
    if (s.sel.on) sds.pref = s.sel.dev.ord;
    if (s.react.on) sds.opp_scale = s.react.dev.eff; // ... and the reactive opponents' effective scales in the configured ones' place
    // (every model's tick advances whether or not a planner is live: a draw depends on the fleet's tick, not on the planner's history)
    for (int k = 0; k < n_ticks; ++k) {
        double* tr = d_trace ? d_trace + rec * (size_t)k : nullptr;
        if (s.events && (rc = sim_events_tick(f, &t))) return rc;
        if (s.sel.on) {
            hipLaunchKernelGGL(k_fleet_sim_select, dim3(N), dim3(64), 0, st, f->args, s.sd, s.sel.dev);
            FLEET_TRY(f, hipGetLastError());
        }
        if (s.react.on) {
            s.react.dev.tick = s.react.stamp();
            hipLaunchKernelGGL(k_fleet_sim_react, dim3(N), dim3(64), 0, st, f->args, s.sd, s.react.dev);
            FLEET_TRY(f, hipGetLastError());
        }
        if (s.noise.on) {
            nz.tick = s.noise.stamp();
            if (s.veh.on) hipLaunchKernelGGL(k_fleet_sim_step_noise_veh, dim3(N), dim3(64), 0, st, f->args, f->h->lat, sds, tr, nz, s.veh.dev);
            else hipLaunchKernelGGL(k_fleet_sim_step_noise, dim3(N), dim3(64), 0, st, f->args, f->h->lat, sds, tr, nz);
        } else if (s.veh.on) {
            hipLaunchKernelGGL(k_fleet_sim_step_veh, dim3(N), dim3(64), 0, st, f->args, f->h->lat, sds, tr, s.veh.dev);
        } else {
            hipLaunchKernelGGL(k_fleet_sim_step, dim3(N), dim3(64), 0, st, f->args, f->h->lat, sds, tr);
        }
        FLEET_TRY(f, hipGetLastError());
        if (s.has_mates) {
            if (s.noise.on) hipLaunchKernelGGL(k_fleet_sim_mates_noise, dim3(N), dim3(64), 0, st, f->h->lat, sds, tr, nz);
            else hipLaunchKernelGGL(k_fleet_sim_mates, dim3(N), dim3(64), 0, st, f->h->lat, sds, tr);
            FLEET_TRY(f, hipGetLastError());
        }
        if (s.tele.on) {
            hipLaunchKernelGGL(k_fleet_sim_tele, dim3(N), dim3(64), 0, st, s.sd, s.tele.dev, s.tele.tick++, (const double*)g_tx, (const double*)g_ty);
            FLEET_TRY(f, hipGetLastError());
            if (s.has_mates) {
                hipLaunchKernelGGL(k_fleet_sim_rank, dim3(N), dim3(64), 0, st, s.sd, s.tele.dev);
                FLEET_TRY(f, hipGetLastError());
            }
        }
        if (s.saf.on) {
            s.saf.dev.tick = s.saf.stamp();
            hipLaunchKernelGGL(k_fleet_sim_safety, dim3(N), dim3(64), 0, st, s.sd, s.saf.dev, (const double*)g_tx, (const double*)g_ty);
            FLEET_TRY(f, hipGetLastError());
        }
        if (s.sens.on) {
            s.sens.dev.tick = s.sens.stamp();
            hipLaunchKernelGGL(k_fleet_sim_sense, dim3(N), dim3(64), 0, st, s.sd, s.sens.dev, g_tx, g_ty, tr);
            FLEET_TRY(f, hipGetLastError());
        }
        if (s.trk.on) {
            s.trk.dev.tick = s.trk.stamp();
            hipLaunchKernelGGL(k_fleet_sim_track, dim3(N), dim3(64), 0, st, s.sd, s.trk.dev, tr);
            FLEET_TRY(f, hipGetLastError());
        }
        hipLaunchKernelGGL(k_fleet_sim_offsets, dim3(1), dim3(1024), 0, st, (const int*)s.sd.cnt, N, s.sd.veh_off);
        FLEET_TRY(f, hipGetLastError());
        if (s.pred.on) hipLaunchKernelGGL(k_fleet_sim_predict, dim3(N), dim3(64), 0, st, s.sd, s.pred.dev);
        else hipLaunchKernelGGL(k_fleet_sim_compact, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, s.sd, N);
        FLEET_TRY(f, hipGetLastError());
        const SimRec& rd = s.rec.dev;
        if (f->tape_fuse && !s.rec.on) {
            fleet::FPathsOut po{};
            if ((rc = fleet_launch_paths(f, t, true, true, false, &po))) return rc;
            if ((rc = fleet_launch_vel(f, t, &po))) return rc;
        } else {
            // (the recorder looks at the state between paths_post and stage A: the launch sequence of LTPL_FLEET_NO_FUSE)
            if ((rc = fleet_launch_paths(f, t, true, true))) return rc;
            if (s.rec.on) {
                hipLaunchKernelGGL(k_fleet_sim_rec_paths, dim3(rd.M), dim3(64), 0, st, f->args, rd, s.rec.tick % s.rec_depth);
                FLEET_TRY(f, hipGetLastError());
            }
            if ((rc = fleet_launch_vel(f, t))) return rc;
        }
        if (s.rec.on) {
            // (the object arrays and veh_off through the simulation's pointers of this launch: ltpl_fleet_sim_race re-allocates the staging)
            hipLaunchKernelGGL(k_fleet_sim_rec_vel, dim3(rd.M), dim3(64), 0, st, f->args, s.sd, rd, s.rec.tick % s.rec_depth, s.rec.tick, s.pos_stride);
            FLEET_TRY(f, hipGetLastError());
            ++s.rec.tick;
        }
        if (tr) {
            hipLaunchKernelGGL(k_fleet_digest, dim3(N), dim3(64), 0, st, f->args, tr + 8, (int)LTPL_FLEET_SIM_TRACE_DOUBLES);
            FLEET_TRY(f, hipGetLastError());
        }
        if (s.stats.on && s.sp.period > 0) {                     // the tail of the tick: every record of the tick is written
            const uint32_t index = s.stats.stamp();
            if ((index + 1u) % (uint32_t)s.sp.period == 0u && (rc = sim_stats_series_row(f, index))) return rc;
        }
    }
    FLEET_TRY(f, hipEventRecord(e1, st));
    FLEET_TRY(f, hipEventSynchronize(e1));
    if (ms_total) FLEET_TRY(f, hipEventElapsedTime(ms_total, e0, e1));
    if (trace) FLEET_TRY(f, hipMemcpy(trace, d_trace, sizeof(double) * rec * (size_t)n_ticks, hipMemcpyDeviceToHost));
    f->cur.has_paths = false;           // (the objects of the last tick live in the simulation: a per-call calc_vel_profile needs its own calc_paths first)
    return fleet_check(f);
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_state(ltpl_fleet* f, double* pos_est_x, double* pos_est_y, double* vel_est, int32_t* sel_action, double* now,
                                    double* opp_s, double* opp_tic)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    if (!f->sim) { f->err = "fleet sim: ltpl_fleet_sim_setup first"; return LTPL_ERR_INVALID_ARG; }
    FLEET_TRY(f, hipSetDevice(f->h->device));
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    const SimDev& d = f->sim->sd;
    const size_t n = (size_t)f->D.N, no = (size_t)f->sim->n_opp;
    if (pos_est_x) FLEET_TRY(f, hipMemcpy(pos_est_x, d.pos_x, 8 * n, hipMemcpyDeviceToHost));
    if (pos_est_y) FLEET_TRY(f, hipMemcpy(pos_est_y, d.pos_y, 8 * n, hipMemcpyDeviceToHost));
    if (vel_est) FLEET_TRY(f, hipMemcpy(vel_est, d.vel, 8 * n, hipMemcpyDeviceToHost));
    if (sel_action) FLEET_TRY(f, hipMemcpy(sel_action, d.sel, 4 * n, hipMemcpyDeviceToHost));
    if (now) FLEET_TRY(f, hipMemcpy(now, d.now, 8 * n, hipMemcpyDeviceToHost));
    if (opp_s && no) FLEET_TRY(f, hipMemcpy(opp_s, d.opp_s, 8 * no, hipMemcpyDeviceToHost));
    if (opp_tic && no) FLEET_TRY(f, hipMemcpy(opp_tic, d.opp_tic, 8 * no, hipMemcpyDeviceToHost));
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

// every argument is checked before the first HIP call
static int sim_check_race(ltpl_fleet* f, const ltpl_fleet_sim_race_in* in)
{
    const int N = f->D.N;
    auto bad = [&](const char* why, int code = LTPL_ERR_INVALID_ARG) { f->err = std::string("fleet sim race: ") + why; return code; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    if (f->sim->ran) return bad("races are set before the first ltpl_fleet_sim_run (ltpl_fleet_sim_setup starts over)");
    if (in->n_races < 1 || !in->race_off) return bad("race offsets missing");
    const int32_t* off = in->race_off;
    if (off[0] != 0 || off[in->n_races] != N) return bad("race offsets must cover the planners 0 .. n");
    for (int r = 0; r < in->n_races; ++r) if (off[r + 1] < off[r]) return bad("race offsets must not decrease");
    if (!in->length || !in->heading0) return bad("length / heading0 missing");
    for (int p = 0; p < N; ++p) {
        if (!std::isfinite(in->length[p]) || !(in->length[p] > 0.0)) return bad("a length must be finite and positive");
        if (!std::isfinite(in->heading0[p])) return bad("a heading0 must be finite");
    }
    for (int r = 0; r < in->n_races; ++r)
        for (int p = off[r]; p < off[r + 1]; ++p)
            if (f->sim->own[(size_t)p] + (off[r + 1] - off[r] - 1) > SIM_OBJ_CAP)
                return bad("opponents + statics + mates above 96 for one planner", LTPL_ERR_CAPACITY);
    if (f->sim->pred.on)                    // the path kernel's position arrays (ltpl_fleet_sim_predictor)
        for (int r = 0; r < in->n_races; ++r)
            for (int p = off[r]; p < off[r + 1]; ++p)
                if ((f->sim->own[(size_t)p] + (off[r + 1] - off[r] - 1)) * f->sim->pos_stride > MAX_POS)
                    return bad("(opponents + statics + mates) x (1 + n_points of the predictor) above 192 for one planner", LTPL_ERR_CAPACITY);
    return LTPL_OK;
}

extern "C" int ltpl_fleet_sim_race(ltpl_fleet* f, const ltpl_fleet_sim_race_in* in)
try {
    if (!f || !in) return LTPL_ERR_INVALID_ARG;
    int rc = sim_check_race(f, in);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FleetSim& s = *f->sim;
    const int N = f->D.N;
    std::vector<int> lo((size_t)N), hi((size_t)N), slots(s.own);
    bool mates = false;
    for (int r = 0; r < in->n_races; ++r)
        for (int p = in->race_off[r]; p < in->race_off[r + 1]; ++p) {
            lo[(size_t)p] = in->race_off[r]; hi[(size_t)p] = in->race_off[r + 1];
            slots[(size_t)p] += in->race_off[r + 1] - in->race_off[r] - 1;
            mates = mates || in->race_off[r + 1] - in->race_off[r] > 1;
        }
    // everything new is allocated first; the fleet keeps its previous races and staging (all of it valid) unless every step succeeds
    SimStage st;
    SimAllocs ra;
    int* d_lo = nullptr; int* d_hi = nullptr; double* d_len = nullptr;
    if ((rc = sim_stage_alloc(f, slots, s.pos_stride, &st))) return rc;
    if ((rc = sim_upload(f, ra.p, lo.data(), (size_t)N, &d_lo))) return rc;
    if ((rc = sim_upload(f, ra.p, hi.data(), (size_t)N, &d_hi))) return rc;
    if ((rc = sim_upload(f, ra.p, in->length, (size_t)N, &d_len))) return rc;
    SimTrackNew tn;                         // a tracker keeps its configuration; its tables follow the new slot counts and start empty
    if (s.trk.on && (rc = sim_tracker_alloc(f, slots, s.trk_par, &tn))) return rc;
    FLEET_TRY(f, hipMemcpy(s.sd.theta, in->heading0, sizeof(double) * (size_t)N, hipMemcpyHostToDevice));
    if (s.trk.on) sim_tracker_commit(&s, &tn, s.trk.tick0);    // (no run yet, see sim_check_race: its tick count is still 0)
    s.slots = slots;
    sim_stage_commit(&s, &st);
    sim_free_list(s.race_allocs);
    s.race_allocs.swap(ra.p);
    s.sd.mate_lo = d_lo; s.sd.mate_hi = d_hi; s.sd.mate_len = d_len;
    s.has_mates = mates;
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_heading(ltpl_fleet* f, double* theta)
try {
    if (!f || !theta) return LTPL_ERR_INVALID_ARG;
    if (!f->sim) { f->err = "fleet sim: ltpl_fleet_sim_setup first"; return LTPL_ERR_INVALID_ARG; }
    FLEET_TRY(f, hipSetDevice(f->h->device));
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FLEET_TRY(f, hipMemcpy(theta, f->sim->sd.theta, sizeof(double) * (size_t)f->D.N, hipMemcpyDeviceToHost));
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

// every argument is checked before the first HIP call
static int sim_check_tele(ltpl_fleet* f, const ltpl_fleet_sim_tele_in* in)
{
    const int N = f->D.N;
    auto bad = [&](const char* why, int code = LTPL_ERR_INVALID_ARG) { f->err = std::string("fleet sim telemetry: ") + why; return code; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    if (!in) return LTPL_OK;
    if (!in->radius) return bad("radius missing");
    for (int p = 0; p < N; ++p) if (!std::isfinite(in->radius[p]) || !(in->radius[p] >= 0.0)) return bad("a radius must be finite and not negative");
    if (in->grid_s) for (int p = 0; p < N; ++p) if (!std::isfinite(in->grid_s[p])) return bad("a grid_s must be finite");
    const ltplp::HostLat& hl = f->h->hostlat;
    if (!f->h->has_hostlat || hl.L < 2) return bad("the lattice carries no race line", LTPL_ERR_UNSUPPORTED);
    // get_s_coord.py:67-68 shifts an s array that does not start at 0 by one entry; the wave-wide projection reads the array as it is
    if (hl.s_rl[0] > 0.05) return bad("s_raceline[0] above 0.05 (the shifted s array of get_s_coord is not supported)", LTPL_ERR_UNSUPPORTED);
    return LTPL_OK;
}

extern "C" int ltpl_fleet_sim_telemetry(ltpl_fleet* f, const ltpl_fleet_sim_tele_in* in)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    int rc = sim_check_tele(f, in);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FleetSim& s = *f->sim;
    if (!in) {
        s.tele.clear(); ++s.tele_gen;
        return LTPL_OK;
    }
    const int N = f->D.N;
    const ltplp::HostLat& hl = f->h->hostlat;
    const int n = hl.L;
    SimTele te{};
    te.n_rl = n;
    {
        const double dx = hl.race_x[0] - hl.race_x[(size_t)n - 1], dy = hl.race_y[0] - hl.race_y[(size_t)n - 1];
        te.length = hl.s_rl[(size_t)n - 1] + std::sqrt(dx * dx + dy * dy);
    }
    std::vector<double> rec((size_t)N * LTPL_FLEET_SIM_TELE_DOUBLES, 0.0);
    for (int p = 0; p < N; ++p) {
        double* r = rec.data() + (size_t)p * LTPL_FLEET_SIM_TELE_DOUBLES;
        r[TELE_S] = r[TELE_T_CROSS] = r[TELE_LAP_LAST] = r[TELE_LAP_BEST] = r[TELE_GAP] = NAN;
        r[TELE_VEL_MAX] = -INFINITY; r[TELE_CLEAR_MIN] = INFINITY; r[TELE_CLEAR_TICK] = r[TELE_CLEAR_SLOT] = -1.0;
    }
    const std::vector<double> prog((size_t)N, -INFINITY), grid_nan((size_t)N, NAN);
    // everything new is allocated first; the fleet keeps its previous telemetry unless every step succeeds
    SimAllocs a;
    double* pd = nullptr;
#define SIM_UP(dst, src, cnt) do { if ((rc = sim_upload(f, a.p, src, (size_t)(cnt), &dst))) return rc; } while (0)
    SIM_UP(pd, hl.race_x.data(), n); te.rl_x = pd; SIM_UP(pd, hl.race_y.data(), n); te.rl_y = pd; SIM_UP(pd, hl.s_rl.data(), n); te.rl_s = pd;
    SIM_UP(pd, in->radius, N); te.radius = pd;
    SIM_UP(te.grid_s, in->grid_s ? in->grid_s : grid_nan.data(), N);
    SIM_UP(te.rec, rec.data(), rec.size()); SIM_UP(te.prog, prog.data(), N);
#undef SIM_UP
    s.tele.commit(a, te); ++s.tele_gen;
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_telemetry_read(ltpl_fleet* f, double* out, int32_t doubles_per_planner, double* track_length)
try {
    if (!f || !out) return LTPL_ERR_INVALID_ARG;
    const int rc = sim_read_records(f, "telemetry", &FleetSim::tele, "telemetry is off (ltpl_fleet_sim_telemetry first)", out, doubles_per_planner,
                                    LTPL_FLEET_SIM_TELE_DOUBLES);
    if (rc == LTPL_OK && track_length) *track_length = f->sim->tele.dev.length;
    return rc;
} LTPL_ABI_CATCH(abi_err_of(f))

// every argument is checked before the first HIP call
static int sim_check_record(ltpl_fleet* f, const int32_t* planners, int32_t n_planners, int32_t depth)
{
    const int N = f->D.N;
    auto bad = [&](const char* why) { f->err = std::string("fleet sim record: ") + why; return LTPL_ERR_INVALID_ARG; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    if (n_planners < 0) return bad("n_planners must not be negative");
    if (!planners || n_planners == 0) return LTPL_OK;
    if (n_planners > N) return bad("more recorded planners than planners");
    if (depth < 1) return bad("depth must be positive");
    std::vector<char> seen((size_t)N, 0);
    for (int i = 0; i < n_planners; ++i) {
        if (planners[i] < 0 || planners[i] >= N) return bad("planner index out of range");
        if (seen[(size_t)planners[i]]) return bad("a planner index is given twice");
        seen[(size_t)planners[i]] = 1;
    }
    return LTPL_OK;
}

extern "C" int ltpl_fleet_sim_record(ltpl_fleet* f, const int32_t* planners, int32_t n_planners, int32_t depth)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    int rc = sim_check_record(f, planners, n_planners, depth);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FleetSim& s = *f->sim;
    auto drop_host = [&]() { s.rec_host_valid = false; s.rec_host.clear(); s.rec_host.shrink_to_fit(); };
    if (!planners || n_planners == 0) {
        s.rec.clear(); s.rec_depth = 0; s.rec_planners.clear();
        drop_host();
        return LTPL_OK;
    }
    SimRec r = sim_rec_layout(f->D, s.sd.n_export);
    r.M = n_planners;
    // everything new is allocated first; the fleet keeps its previous recorder unless every step succeeds
    SimAllocs a;
    int* d_idx = nullptr;
    if ((rc = sim_upload(f, a.p, planners, (size_t)n_planners, &d_idx))) return rc;
    if ((rc = sim_upload(f, a.p, (const double*)nullptr, (size_t)depth * (size_t)n_planners * r.stride, &r.ring))) return rc;
    r.planners = d_idx;
    s.rec.commit(a, r); s.rec_depth = depth; s.rec_planners.assign(planners, planners + n_planners);
    drop_host();
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_record_info(ltpl_fleet* f, int32_t* n_planners, int32_t* depth, int32_t* first_tick, int32_t* n_ticks)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    if (!f->sim) { f->err = "fleet sim record: ltpl_fleet_sim_setup first"; return LTPL_ERR_INVALID_ARG; }
    const FleetSim& s = *f->sim;
    const int held = s.rec.on ? (s.rec.tick < s.rec_depth ? s.rec.tick : s.rec_depth) : 0;
    if (n_planners) *n_planners = s.rec.on ? s.rec.dev.M : 0;
    if (depth) *depth = s.rec_depth;
    if (first_tick) *first_tick = s.rec.tick - held;
    if (n_ticks) *n_ticks = held;
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_record_get(ltpl_fleet* f, int32_t tick, int32_t slot, ltpl_fleet_sim_record_head* head, double* objects,
                                         ltpl_planner_paths_view* pv, double* const_xy, ltpl_planner_traj_view* tv)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const char* why) { f->err = std::string("fleet sim record: ") + why; return LTPL_ERR_INVALID_ARG; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    FleetSim& s = *f->sim;
    if (!s.rec.on) return bad("the recorder is off (ltpl_fleet_sim_record first)");
    const int held = s.rec.tick < s.rec_depth ? s.rec.tick : s.rec_depth;
    if (tick < s.rec.tick - held || tick >= s.rec.tick) return bad("the ring does not hold this tick (ltpl_fleet_sim_record_info)");
    if (slot < 0 || slot >= s.rec.dev.M) return bad("slot outside the recorded planners");
    FLEET_TRY(f, hipSetDevice(f->h->device));
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    const SimRec& r = s.rec.dev;
    if (!s.rec_host_valid) {                                    // once per run: later calls are served from the host copy
        const size_t n = (size_t)s.rec_depth * (size_t)r.M * r.stride;
        s.rec_host.resize(n);
        FLEET_TRY(f, hipMemcpy(s.rec_host.data(), r.ring, sizeof(double) * n, hipMemcpyDeviceToHost));
        s.rec_host_valid = true;
    }
    const double* o = s.rec_host.data() + ((size_t)(tick % s.rec_depth) * (size_t)r.M + (size_t)slot) * r.stride;
    const int R = f->D.R, CN = f->D.CN, E = r.E;
    const int n_obj = (int)o[REC_N_OBJ];
    if (head) {
        head->tick = (int32_t)o[REC_TICK]; head->planner = (int32_t)o[REC_PLANNER]; head->error = (int32_t)o[REC_ERR];
        head->sel_action = (int32_t)o[REC_SEL]; head->t_now = o[REC_T_NOW]; head->pos_x = o[REC_X]; head->pos_y = o[REC_Y];
        head->vel_est = o[REC_VEL]; head->heading = o[REC_THETA]; head->n_objects = n_obj; head->reserved0 = 0;
    }
    if (objects) {
        const double* ob = o + r.o_obj;
        for (int i = 0; i < n_obj; ++i) for (int c = 0; c < 6; ++c) objects[(size_t)i * 6 + c] = ob[(size_t)c * SIM_OBJ_CAP + i];
    }
    const int nk = (int)o[REC_N_PATHS];
    const int const_rows = (int)o[REC_CONST_ROWS];
    if (pv) {
        pv->n_keys = nk;
        pv->start_node[0] = (int32_t)o[REC_START]; pv->start_node[1] = (int32_t)o[REC_START + 1];
        pv->const_rows = const_rows; pv->closest_obj_index = (int32_t)o[REC_CLOSEST];
        const int* nodes = reinterpret_cast<const int*>(o + r.o_nodes);
        for (int k = 0; k < nk; ++k) {
            const double* q = o + REC_PATHS + 4 * k;
            pv->key_id[k] = (int32_t)q[0]; pv->n_rows[k] = (int32_t)q[1]; pv->n_nodes[k] = (int32_t)q[2]; pv->red_len[k] = (int32_t)q[3];
            const int nn = pv->n_nodes[k] < CN ? pv->n_nodes[k] : CN;
            if (pv->nodes[k] && nn > 0) std::memcpy(pv->nodes[k], nodes + (size_t)k * CN * 2, sizeof(int) * 2 * (size_t)nn);
        }
    }
    if (const_xy && nk > 0 && const_rows > 0) {
        int n = const_rows < (int)o[REC_PATHS + 1] ? const_rows : (int)o[REC_PATHS + 1];
        if (n > R) n = R;
        const double* cx = o + r.o_const; const double* cy = cx + R;
        for (int i = 0; i < n; ++i) { const_xy[(size_t)i * 2] = cx[i]; const_xy[(size_t)i * 2 + 1] = cy[i]; }
    }
    if (tv) {
        const int nb = (int)o[REC_N_TRAJ], ni = (int)o[REC_N_IDS];
        tv->n_keys = nb; tv->n_ids = ni; tv->n_vel_course = 0;
        tv->cut_index_pos = (int32_t)o[REC_CUT_POS]; tv->cut_layer = (int32_t)o[REC_CUT_LAYER]; tv->vel_plan = o[REC_VEL_PLAN]; tv->acc_plan = o[REC_ACC_PLAN];
        for (int k = 0; k < ni; ++k) { tv->id_key[k] = (int32_t)o[REC_IDS + 2 * k]; tv->id_val[k] = (int32_t)o[REC_IDS + 2 * k + 1]; }
        for (int k = 0; k < nb; ++k) {
            const double* q = o + REC_TRAJ + 3 * k;
            tv->key_id[k] = (int32_t)q[0]; tv->traj_id[k] = (int32_t)q[1]; tv->n_rows[k] = (int32_t)q[2];
            if (tv->traj[k]) {
                const int n = tv->n_rows[k] < E ? tv->n_rows[k] : E;
                const double* t = o + r.o_traj + (size_t)k * 7 * E;
                for (int i = 0; i < n; ++i) for (int c = 0; c < 7; ++c) tv->traj[k][(size_t)i * 7 + c] = t[(size_t)c * E + i];
            }
        }
    }
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

// ---------------------------------------------------------------------------------------------------------------------
// sensor noise (ltpl_fleet_sim_noise, include/ltpl_hip.h; the generator: fleet_noise.hpp)
// ---------------------------------------------------------------------------------------------------------------------
// every argument is checked before the first HIP call
static int sim_check_noise(ltpl_fleet* f, const ltpl_fleet_sim_noise_in* in)
{
    const int N = f->D.N;
    auto bad = [&](const char* why) { f->err = std::string("fleet sim noise: ") + why; return LTPL_ERR_INVALID_ARG; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    if (!in) return LTPL_OK;
    if (!in->seed) return bad("seed missing");
    if (in->tick0 < 0) return bad("tick0 must not be negative");
    const double* sg[NZ_SIGMAS] = {in->sigma_pos, in->sigma_vel, in->sigma_obj_pos, in->sigma_obj_theta, in->sigma_obj_vel};
    for (const double* a : sg)
        if (a) for (int p = 0; p < N; ++p) if (!std::isfinite(a[p]) || !(a[p] >= 0.0)) return bad("a sigma must be finite and not negative");
    return LTPL_OK;
}

extern "C" int ltpl_fleet_sim_noise(ltpl_fleet* f, const ltpl_fleet_sim_noise_in* in)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    int rc = sim_check_noise(f, in);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FleetSim& s = *f->sim;
    if (!in) {
        SimNoise nz = s.noise.dev;         // (est_* and g_* belong to the setup and the staging: they stay)
        nz.seed = nullptr; nz.sigma = nullptr;
        s.noise.clear(nz);
        return LTPL_OK;
    }
    const size_t N = (size_t)f->D.N;
    std::vector<double> sigma(NZ_SIGMAS * N, 0.0);
    const double* sg[NZ_SIGMAS] = {in->sigma_pos, in->sigma_vel, in->sigma_obj_pos, in->sigma_obj_theta, in->sigma_obj_vel};
    for (int c = 0; c < NZ_SIGMAS; ++c) if (sg[c]) std::copy(sg[c], sg[c] + N, sigma.begin() + (size_t)c * N);
    // everything new is allocated first; the fleet keeps its previous noise and its tick count unless every step succeeds
    SimAllocs a;
    uint64_t* d_seed = nullptr; double* d_sigma = nullptr;
    if ((rc = sim_upload(f, a.p, in->seed, N, &d_seed))) return rc;
    if ((rc = sim_upload(f, a.p, sigma.data(), sigma.size(), &d_sigma))) return rc;
    SimNoise nz = s.noise.dev;             // (est_* and g_* belong to the setup and the staging: they stay)
    if (!s.noise.on) {                      // until the first noisy tick the estimate is the true state
        FLEET_TRY(f, hipMemcpy(nz.est_x, s.sd.pos_x, 8 * N, hipMemcpyDeviceToDevice));
        FLEET_TRY(f, hipMemcpy(nz.est_y, s.sd.pos_y, 8 * N, hipMemcpyDeviceToDevice));
        FLEET_TRY(f, hipMemcpy(nz.est_v, s.sd.vel, 8 * N, hipMemcpyDeviceToDevice));
    }
    nz.seed = d_seed; nz.sigma = d_sigma;
    s.noise.commit(a, nz, in->tick0);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_estimate(ltpl_fleet* f, double* x, double* y, double* v)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    if (!f->sim) { f->err = "fleet sim noise: ltpl_fleet_sim_setup first"; return LTPL_ERR_INVALID_ARG; }
    FLEET_TRY(f, hipSetDevice(f->h->device));
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    const FleetSim& s = *f->sim;
    const size_t n = (size_t)f->D.N;
    const SimNoise& nz = s.noise.dev;
    if (x) FLEET_TRY(f, hipMemcpy(x, s.noise.on ? nz.est_x : s.sd.pos_x, 8 * n, hipMemcpyDeviceToHost));
    if (y) FLEET_TRY(f, hipMemcpy(y, s.noise.on ? nz.est_y : s.sd.pos_y, 8 * n, hipMemcpyDeviceToHost));
    if (v) FLEET_TRY(f, hipMemcpy(v, s.noise.on ? nz.est_v : s.sd.vel, 8 * n, hipMemcpyDeviceToHost));
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

// the test hook of the generator: one lane per tuple
__global__ __launch_bounds__(256) void k_fleet_noise_draws(const uint64_t* seed, const uint32_t* tick, const uint32_t* obj, const uint32_t* comp, int n,
                                                           double* g, uint32_t* words /* [n][12] or null */)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t w[12];
    g[i] = fleet::noise_gauss(seed[i], tick[i], obj[i], comp[i], w);
    if (words) for (int k = 0; k < 12; ++k) words[(size_t)i * 12 + k] = w[k];
}

extern "C" int ltpl_fleet_sim_noise_draws(ltpl_fleet* f, const uint64_t* seed, const uint32_t* tick, const uint32_t* obj, const uint32_t* comp, int32_t n,
                                          double* g, uint32_t* words)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const char* why) { f->err = std::string("fleet sim noise: ") + why; return LTPL_ERR_INVALID_ARG; };
    if (n < 0) return bad("n must not be negative");
    if (n > 0 && (!seed || !tick || !obj || !comp || !g)) return bad("seed / tick / obj / comp / g missing");
    if (n == 0) return LTPL_OK;
    int rc = fleet_enter(f);
    if (rc) return rc;
    const size_t m = (size_t)n;
    SimHookBlock b(f);
    const auto d_seed = b.in(seed, m); const auto d_tick = b.in(tick, m); const auto d_obj = b.in(obj, m); const auto d_comp = b.in(comp, m);
    const auto d_g = b.out<double>(m); const auto d_words = b.out<uint32_t>(12 * m);
    if ((rc = b.upload())) return rc;
    hipLaunchKernelGGL(k_fleet_noise_draws, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, f->h->stream, d_seed, d_tick, d_obj, d_comp, (int)n, d_g,
                       words ? d_words.get() : nullptr);
    FLEET_TRY(f, hipGetLastError());
    if ((rc = b.fetch(g, d_g, m))) return rc;
    if (words && (rc = b.fetch(words, d_words, 12 * m))) return rc;
    return b.finish();
} LTPL_ABI_CATCH(abi_err_of(f))

// ---------------------------------------------------------------------------------------------------------------------
// vehicle model (ltpl_fleet_sim_vehicle, include/ltpl_hip.h; the model: fleet_vehicle.hpp)
// ---------------------------------------------------------------------------------------------------------------------
// every argument is checked before the first HIP call
static int sim_check_vehicle(ltpl_fleet* f, const ltpl_fleet_sim_vehicle_in* in, std::vector<double>* par)
{
    auto bad = [&](const std::string& why) { f->err = "fleet sim vehicle: " + why; return LTPL_ERR_INVALID_ARG; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    if (!in) return LTPL_OK;
    if (in->flags & ~(uint32_t)LTPL_SIM_VEH_KEEP_STATE) return bad("unknown flag");
    if (in->ctl_steps < 1) return bad("ctl_steps must be at least 1");
    if (!in->model) return bad("model missing");
    const SimCol col[VEH_PARAMS] = {{"ax_max", in->ax_max}, {"ay_max", in->ay_max}, {"grip", in->grip}, {"kappa_max", in->kappa_max}, {"tau_a", in->tau_a},
                                    {"tau_kappa", in->tau_kappa}, {"k_v", in->k_v}, {"t_look", in->t_look}, {"ld_min", in->ld_min}};
    return sim_param_table(f, "vehicle", col, sim_no_head, [&](int p, const double* q, std::string* why) {
        if (in->model[p] != 0 && in->model[p] != 1) { *why = "model must be 0 or 1"; return false; }
        if (in->model[p] == 0) return true;         // (the parameters of a planner on the ideal tracker are not read)
        for (int c = 0; c < VEH_PARAMS; ++c) {
            if (!std::isfinite(q[c]) || !(q[c] > 0.0)) { *why = std::string(col[c].name) + " must be finite and positive"; return false; }
            if ((c == 4 || c == 5) && q[c] < 0.001) { *why = std::string(col[c].name) + " must be at least 0.001 s"; return false; }
        }
        return true;
    }, par);
}

extern "C" int ltpl_fleet_sim_vehicle(ltpl_fleet* f, const ltpl_fleet_sim_vehicle_in* in)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    std::vector<double> par;
    int rc = sim_check_vehicle(f, in, &par);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FleetSim& s = *f->sim;
    if (!in) {
        s.veh.clear(); s.veh_model.clear();
        return LTPL_OK;
    }
    const size_t N = (size_t)f->D.N;
    constexpr size_t RD = LTPL_FLEET_SIM_VEH_DOUBLES;
    const bool keep = (in->flags & LTPL_SIM_VEH_KEEP_STATE) && s.veh.on;
    std::vector<double> rec(N * RD, NAN), old, px(N), py(N), pv(N), pt(N);
    FLEET_TRY(f, hipMemcpy(px.data(), s.sd.pos_x, 8 * N, hipMemcpyDeviceToHost));
    FLEET_TRY(f, hipMemcpy(py.data(), s.sd.pos_y, 8 * N, hipMemcpyDeviceToHost));
    FLEET_TRY(f, hipMemcpy(pv.data(), s.sd.vel, 8 * N, hipMemcpyDeviceToHost));
    FLEET_TRY(f, hipMemcpy(pt.data(), s.sd.theta, 8 * N, hipMemcpyDeviceToHost));
    if (keep) {
        old.resize(N * RD);
        FLEET_TRY(f, hipMemcpy(old.data(), s.veh.dev.rec, 8 * N * RD, hipMemcpyDeviceToHost));
    }
    for (size_t p = 0; p < N; ++p) {
        if (in->model[p] == 0) continue;            // NaN: no state, no statistics
        double* r = rec.data() + p * RD;
        if (keep && s.veh_model[p] == 1) { std::copy(old.begin() + p * RD, old.begin() + (p + 1) * RD, r); continue; }
        std::fill(r, r + RD, 0.0);
        r[VEH_X] = px[p]; r[VEH_Y] = py[p]; r[VEH_C] = -std::sin(pt[p]); r[VEH_S] = std::cos(pt[p]); r[VEH_V] = pv[p];
    }
    // everything new is allocated first; the fleet keeps its previous model, state and statistics unless every step succeeds
    SimAllocs al;
    int* d_model = nullptr; double* d_par = nullptr; double* d_rec = nullptr;
    if ((rc = sim_upload(f, al.p, in->model, N, &d_model))) return rc;
    if ((rc = sim_upload(f, al.p, par.data(), par.size(), &d_par))) return rc;
    if ((rc = sim_upload(f, al.p, rec.data(), rec.size(), &d_rec))) return rc;
    s.veh.commit(al, SimVeh{d_model, d_par, d_rec, in->ctl_steps});
    s.veh_model.assign(in->model, in->model + N);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_vehicle_read(ltpl_fleet* f, double* out, int32_t doubles_per_planner)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    return sim_read_records(f, "vehicle", &FleetSim::veh, "the model is off (ltpl_fleet_sim_vehicle first)", out, doubles_per_planner,
                            LTPL_FLEET_SIM_VEH_DOUBLES);
} LTPL_ABI_CATCH(abi_err_of(f))

// the test hook of the model: one wave per case, the device function of the tick (sim_vehicle_tick) on the case's own rows, staged in LDS
// as the tick stages a trajectory. out: the state after the tick, the tick's statistics (from zero), 1.0 in VEH_OFF_TRACK where the
// pose fails the ingestion's track test on the fleet's lattice; theta: the library's heading of (s, c)
__global__ __launch_bounds__(64) void k_fleet_sim_vehicle_step(DevLat lat, const double* state, const double* par, const int* row_off, const double* rows,
                                                               const double* dt, const int* ctl_steps, double* out, double* theta)
{
    const int q = blockIdx.x, lane = threadIdx.x;
    __shared__ double ts[LTPL_FLEET_SIM_MAX_EXPORT], tx[LTPL_FLEET_SIM_MAX_EXPORT], ty[LTPL_FLEET_SIM_MAX_EXPORT], tv[LTPL_FLEET_SIM_MAX_EXPORT],
        ta[LTPL_FLEET_SIM_MAX_EXPORT];
    const int r0 = row_off[q];
    int n = row_off[q + 1] - r0;
    if (n > LTPL_FLEET_SIM_MAX_EXPORT) n = LTPL_FLEET_SIM_MAX_EXPORT;      // (refused by the host)
    for (int i = lane; i < n; i += 64) {
        const double* r = rows + (size_t)(r0 + i) * 5;
        ts[i] = r[0]; tx[i] = r[1]; ty[i] = r[2]; tv[i] = r[3]; ta[i] = r[4];
    }
    __syncthreads();
    const double* s0 = state + (size_t)q * 7;
    fleet::VehState V{s0[0], s0[1], s0[2], s0[3], s0[4], s0[5], s0[6]};
    fleet::VehStats st{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    sim_vehicle_tick(lane, V, sim_vehicle_params(par + (size_t)q * VEH_PARAMS), fleet::VehRows{ts, tx, ty, tv, ta, n}, dt[q], ctl_steps[q], st);
    if (lane != 0) return;
    double* r = out + (size_t)q * LTPL_FLEET_SIM_VEH_DOUBLES;
    r[VEH_X] = V.x; r[VEH_Y] = V.y; r[VEH_C] = V.c; r[VEH_S] = V.s; r[VEH_V] = V.v; r[VEH_A] = V.a; r[VEH_KAPPA] = V.kappa;
    r[VEH_E] = st.e; r[VEH_E_MAX] = st.e_max; r[VEH_E2_SUM] = st.e2_sum; r[VEH_DV_MAX] = st.dv_max; r[VEH_CTL] = st.ctl;
    r[VEH_SAT_LAT] = st.sat_lat; r[VEH_SAT_LON] = st.sat_lon;
    r[VEH_OFF_TRACK] = process_object_dev(lat, 0.2, V.x, V.y, 0.0, 0.0, 0.0).on_track ? 0.0 : 1.0;
    theta[q] = heading_atan2(-V.c, V.s);
}

extern "C" int ltpl_fleet_sim_vehicle_step(ltpl_fleet* f, int32_t n_cases, const double* state, const double* params, const int32_t* row_off,
                                           const double* rows, const double* dt, const int32_t* ctl_steps, double* out, int32_t doubles_per_case,
                                           double* theta)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const std::string& why) { f->err = "fleet sim vehicle step: " + why; return LTPL_ERR_INVALID_ARG; };
    if (n_cases < 0) return bad("n_cases must not be negative");
    if (n_cases == 0) return LTPL_OK;
    if (!state || !params || !row_off || !dt || !ctl_steps || !out || !theta) return bad("state / params / row_off / dt / ctl_steps / out / theta missing");
    if (doubles_per_case != LTPL_FLEET_SIM_VEH_DOUBLES) return bad("record size mismatch");
    if (row_off[0] != 0) return bad("row offsets must start at 0");
    for (int q = 0; q < n_cases; ++q) {
        const int n = row_off[q + 1] - row_off[q];
        if (n < 0 || n > LTPL_FLEET_SIM_MAX_EXPORT) return bad("case " + std::to_string(q) + ": 0 .. 256 rows");
        if (!(dt[q] > 0.0) || !(dt[q] <= 1.0)) return bad("case " + std::to_string(q) + ": dt must lie in (0, 1] s");
        if (ctl_steps[q] < 1) return bad("case " + std::to_string(q) + ": ctl_steps must be at least 1");
    }
    const size_t m = (size_t)n_cases, nr = (size_t)row_off[n_cases];
    if (nr > 0 && !rows) return bad("rows missing");
    int rc = fleet_enter(f);
    if (rc) return rc;
    SimHookBlock b(f);
    const auto d_state = b.in(state, 7 * m); const auto d_par = b.in(params, VEH_PARAMS * m); const auto d_off = b.in(row_off, m + 1);
    const auto d_rows = b.in(rows, 5 * nr); const auto d_dt = b.in(dt, m); const auto d_ctl = b.in(ctl_steps, m);
    const auto d_out = b.out<double>(LTPL_FLEET_SIM_VEH_DOUBLES * m); const auto d_theta = b.out<double>(m);
    if ((rc = b.upload())) return rc;
    hipLaunchKernelGGL(k_fleet_sim_vehicle_step, dim3((unsigned)m), dim3(64), 0, f->h->stream, f->h->lat, d_state, d_par, d_off, d_rows, d_dt, d_ctl, d_out,
                       d_theta);
    FLEET_TRY(f, hipGetLastError());
    if ((rc = b.fetch(out, d_out, LTPL_FLEET_SIM_VEH_DOUBLES * m))) return rc;
    if ((rc = b.fetch(theta, d_theta, m))) return rc;
    return b.finish();
} LTPL_ABI_CATCH(abi_err_of(f))

// ---------------------------------------------------------------------------------------------------------------------
// sensor model (ltpl_fleet_sim_sensor, include/ltpl_hip.h; the rule: fleet_sensor.hpp)
// ---------------------------------------------------------------------------------------------------------------------
// every argument is checked before the first HIP call
static int sim_check_sensor(ltpl_fleet* f, const ltpl_fleet_sim_sensor_in* in, std::vector<double>* par)
{
    auto bad = [&](const std::string& why) { f->err = "fleet sim sensor: " + why; return LTPL_ERR_INVALID_ARG; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    if (!in) return LTPL_OK;
    const SimCol col[SENS_PARAMS] = {{"range", in->range}, {"r_near", in->r_near}, {"fov_cos", in->fov_cos}, {"occl", in->occl}, {"p_drop", in->p_drop}};
    auto head = [&]() -> const char* { return !in->seed ? "seed missing" : in->tick0 < 0 ? "tick0 must not be negative" : nullptr; };
    return sim_param_table(f, "sensor", col, head, [](int, const double* q, std::string* why) {
        const double range = q[0], r_near = q[1], fov_cos = q[2], occl = q[3], p_drop = q[4];
        if (!(range >= 0.0)) { *why = "range must not be negative or NaN (+inf: no limit)"; return false; }
        if (!(r_near >= 0.0) || !(r_near <= range)) { *why = "r_near must lie in [0, range]"; return false; }
        if (!(fov_cos >= -1.0) || !(fov_cos <= 1.0)) { *why = "fov_cos must lie in [-1, 1]"; return false; }
        if (!std::isfinite(occl) || !(occl >= 0.0)) { *why = "occl must be finite and not negative"; return false; }
        if (!(p_drop >= 0.0) || !(p_drop < 1.0)) { *why = "p_drop must lie in [0, 1)"; return false; }
        return true;
    }, par);
}

extern "C" int ltpl_fleet_sim_sensor(ltpl_fleet* f, const ltpl_fleet_sim_sensor_in* in)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    std::vector<double> par;
    int rc = sim_check_sensor(f, in, &par);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FleetSim& s = *f->sim;
    if (!in) {
        s.sens.clear();
        return LTPL_OK;
    }
    const size_t N = (size_t)f->D.N;
    constexpr size_t RD = LTPL_FLEET_SIM_SENSOR_DOUBLES;
    std::vector<double> rec(N * RD, 0.0);
    for (size_t p = 0; p < N; ++p) { rec[p * RD + SENS_CLEAR_MIN] = INFINITY; rec[p * RD + SENS_CLEAR_TICK] = -1.0; }
    // everything new is allocated first; the fleet keeps its previous sensor, its tick count and its statistics unless every step succeeds
    SimAllocs al;
    double* d_par = nullptr; uint64_t* d_seed = nullptr; double* d_rec = nullptr;
    if ((rc = sim_upload(f, al.p, par.data(), par.size(), &d_par))) return rc;
    if ((rc = sim_upload(f, al.p, in->seed, N, &d_seed))) return rc;
    if ((rc = sim_upload(f, al.p, rec.data(), rec.size(), &d_rec))) return rc;
    s.sens.commit(al, SimSense{d_par, d_seed, d_rec, 0u}, in->tick0);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_sensor_read(ltpl_fleet* f, double* out, int32_t doubles_per_planner)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    return sim_read_records(f, "sensor", &FleetSim::sens, "the sensor is off (ltpl_fleet_sim_sensor first)", out, doubles_per_planner,
                            LTPL_FLEET_SIM_SENSOR_DOUBLES);
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_sensor_eval(ltpl_fleet* f, int32_t n_cases, const double* pose_f, const double* params, const uint64_t* seed,
                                          const uint32_t* tick, const int32_t* obj_off, const double* objs, int32_t* cause, double* u)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const std::string& why) { f->err = "fleet sim sensor eval: " + why; return LTPL_ERR_INVALID_ARG; };
    if (n_cases < 0) return bad("n_cases must not be negative");
    if (n_cases == 0) return LTPL_OK;
    if (!pose_f || !params || !seed || !tick || !obj_off) return bad("pose_f / params / seed / tick / obj_off missing");
    if (obj_off[0] != 0) return bad("object offsets must start at 0");
    for (int q = 0; q < n_cases; ++q) {
        const int n = obj_off[q + 1] - obj_off[q];
        if (n < 0 || n > SIM_OBJ_CAP) return bad("case " + std::to_string(q) + ": 0 .. 96 objects");
    }
    const size_t m = (size_t)n_cases, no = (size_t)obj_off[n_cases];
    if (no > 0 && (!objs || !cause || !u)) return bad("objs / cause / u missing");
    int rc = fleet_enter(f);
    if (rc) return rc;
    SimHookBlock b(f);
    const auto d_pf = b.in(pose_f, 4 * m); const auto d_par = b.in(params, SENS_PARAMS * m); const auto d_seed = b.in(seed, m);
    const auto d_tick = b.in(tick, m); const auto d_off = b.in(obj_off, m + 1); const auto d_objs = b.in(objs, 3 * no);
    const auto d_cause = b.out<int32_t>(no); const auto d_u = b.out<double>(no);
    if ((rc = b.upload())) return rc;
    hipLaunchKernelGGL(k_fleet_sim_sensor_eval, dim3((unsigned)m), dim3(64), 0, f->h->stream, d_pf, d_par, d_seed, d_tick, d_off, d_objs, d_cause, d_u);
    FLEET_TRY(f, hipGetLastError());
    if ((rc = b.fetch(cause, d_cause, no))) return rc;
    if ((rc = b.fetch(u, d_u, no))) return rc;
    return b.finish();
} LTPL_ABI_CATCH(abi_err_of(f))

// ---------------------------------------------------------------------------------------------------------------------
// object tracker (ltpl_fleet_sim_tracker, include/ltpl_hip.h; the rule: fleet_track.hpp)
// ---------------------------------------------------------------------------------------------------------------------
// every argument is checked before the first HIP call
static int sim_check_tracker(ltpl_fleet* f, const ltpl_fleet_sim_tracker_in* in, std::vector<double>* par)
{
    auto bad = [&](const std::string& why) { f->err = "fleet sim tracker: " + why; return LTPL_ERR_INVALID_ARG; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    if (!in) return LTPL_OK;
    const SimCol col[TRK_PARAMS] = {{"gate", in->gate}, {"w_pos", in->w_pos}, {"w_vel", in->w_vel}, {"n_confirm", in->n_confirm}, {"n_coast", in->n_coast}};
    auto head = [&]() -> const char* { return in->tick0 < 0 ? "tick0 must not be negative" : nullptr; };
    return sim_param_table(f, "tracker", col, head, [](int, const double* q, std::string* why) {
        if (!std::isfinite(q[0]) || !(q[0] > 0.0)) { *why = "gate must be finite and positive"; return false; }
        if (!(q[1] >= 0.0) || !(q[1] < 1.0)) { *why = "w_pos must lie in [0, 1)"; return false; }
        if (!(q[2] >= 0.0) || !(q[2] < 1.0)) { *why = "w_vel must lie in [0, 1)"; return false; }
        if (q[3] < 1.0 || q[3] > 255.0) { *why = "n_confirm must lie in 1 .. 255"; return false; }
        if (q[4] < 0.0 || q[4] > 255.0) { *why = "n_coast must lie in 0 .. 255"; return false; }
        return true;
    }, par);
}

extern "C" int ltpl_fleet_sim_tracker(ltpl_fleet* f, const ltpl_fleet_sim_tracker_in* in)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    std::vector<double> par;
    int rc = sim_check_tracker(f, in, &par);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FleetSim& s = *f->sim;
    if (!in) {
        s.trk.clear();
        s.trk_par.clear(); s.trk_cap.clear();
        return LTPL_OK;
    }
    // everything new is allocated first; the fleet keeps its previous tracker, its tables, its tick count and its statistics unless every step succeeds
    SimTrackNew tn;
    if ((rc = sim_tracker_alloc(f, s.slots, par, &tn))) return rc;
    sim_tracker_commit(&s, &tn, in->tick0);
    s.trk_par.swap(par);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_tracker_read(ltpl_fleet* f, double* rec_out, int32_t doubles_per_planner, int32_t n_sel, const int32_t* sel_planners,
                                           double* tracks_out, int32_t* n_tracks_out)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const std::string& why) { f->err = "fleet sim tracker: " + why; return LTPL_ERR_INVALID_ARG; };
    const int N = f->D.N;
    int rc = sim_read_records(f, "tracker", &FleetSim::trk, "the tracker is off (ltpl_fleet_sim_tracker first)", rec_out, "rec_out", doubles_per_planner,
                              LTPL_FLEET_SIM_TRACKER_DOUBLES, [&] {
        if (n_sel < 0) return bad("n_sel must not be negative");
        if (n_sel > 0 && (!sel_planners || !tracks_out || !n_tracks_out)) return bad("sel_planners / tracks_out / n_tracks_out missing");
        for (int i = 0; i < n_sel; ++i) if (sel_planners[i] < 0 || sel_planners[i] >= N) return bad("planner index " + std::to_string(sel_planners[i]) + " out of range");
        return LTPL_OK;
    });
    if (rc) return rc;
    const FleetSim& s = *f->sim;
    const SimTrack& tk = s.trk.dev;
    if (n_sel == 0) return LTPL_OK;
    std::vector<int> n_trk((size_t)N);
    FLEET_TRY(f, hipMemcpy(n_trk.data(), tk.n, sizeof(int) * (size_t)N, hipMemcpyDeviceToHost));
    constexpr size_t RD = LTPL_FLEET_SIM_TRACK_DOUBLES, TAB = (size_t)SIM_OBJ_CAP * RD;
    size_t base = 0;
    std::vector<size_t> row0((size_t)N);
    for (int p = 0; p < N; ++p) { row0[(size_t)p] = base; base += (size_t)s.trk_cap[(size_t)p]; }
    for (int i = 0; i < n_sel; ++i) {
        const size_t p = (size_t)sel_planners[i];
        const int n = n_trk[p] < s.trk_cap[p] ? n_trk[p] : s.trk_cap[p];
        double* o = tracks_out + (size_t)i * TAB;
        for (size_t c = 0; c < TAB; ++c) o[c] = NAN;
        if (n > 0) FLEET_TRY(f, hipMemcpy(o, tk.rows + row0[p] * RD, sizeof(double) * (size_t)n * RD, hipMemcpyDeviceToHost));
        n_tracks_out[i] = n;
    }
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_tracker_eval(ltpl_fleet* f, int32_t n_cases, const double* params, const double* adv, const uint32_t* tick,
                                           const int32_t* cap_slots, const int32_t* trk_off, const double* tracks, const double* next_id,
                                           const int32_t* det_off, const double* dets, double* tracks_out, int32_t* n_tracks_out, double* next_id_out,
                                           double* out, int32_t* n_out, int32_t* assign, double* rec)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const std::string& why) { f->err = "fleet sim tracker eval: " + why; return LTPL_ERR_INVALID_ARG; };
    if (n_cases < 0) return bad("n_cases must not be negative");
    if (n_cases == 0) return LTPL_OK;
    if (!params || !adv || !tick || !cap_slots || !trk_off || !next_id || !det_off) return bad("params / adv / tick / cap_slots / trk_off / next_id / det_off missing");
    if (!tracks_out || !n_tracks_out || !next_id_out || !out || !n_out || !rec) return bad("tracks_out / n_tracks_out / next_id_out / out / n_out / rec missing");
    if (trk_off[0] != 0 || det_off[0] != 0) return bad("track and detection offsets must start at 0");
    for (int q = 0; q < n_cases; ++q) {
        const std::string who = "case " + std::to_string(q) + ": ";
        const int T = trk_off[q + 1] - trk_off[q], K = det_off[q + 1] - det_off[q], cap = cap_slots[2 * q], slots = cap_slots[2 * q + 1];
        if (cap < 0 || cap > SIM_OBJ_CAP || slots < 0 || slots > SIM_OBJ_CAP) return bad(who + "capacity and slots must lie in 0 .. 96");
        if (T < 0 || T > cap) return bad(who + "0 .. capacity tracks");
        if (K < 0 || K > slots) return bad(who + "0 .. slots detections");
        const double* P = params + (size_t)q * TRK_PARAMS;
        if (!std::isfinite(P[0]) || !(P[0] > 0.0) || !(P[1] >= 0.0) || !(P[1] < 1.0) || !(P[2] >= 0.0) || !(P[2] < 1.0) || !(P[3] >= 1.0) || !(P[3] <= 255.0) ||
            !(P[4] >= 0.0) || !(P[4] <= 255.0))
            return bad(who + "parameters out of range");
    }
    const size_t m = (size_t)n_cases, nt = (size_t)trk_off[n_cases], nd = (size_t)det_off[n_cases];
    if (nt > 0 && !tracks) return bad("tracks missing");
    if (nd > 0 && (!dets || !assign)) return bad("dets / assign missing");
    constexpr size_t RD = LTPL_FLEET_SIM_TRACK_DOUBLES, TAB = (size_t)SIM_OBJ_CAP * RD, OUT = (size_t)SIM_OBJ_CAP * 6, SD = LTPL_FLEET_SIM_TRACKER_DOUBLES;
    std::vector<double> tab(m * TAB, NAN);
    std::vector<int> n0(m);
    for (size_t q = 0; q < m; ++q) {
        n0[q] = trk_off[q + 1] - trk_off[q];
        if (n0[q]) std::memcpy(&tab[q * TAB], tracks + (size_t)trk_off[q] * RD, sizeof(double) * (size_t)n0[q] * RD);
    }
    int rc = fleet_enter(f);
    if (rc) return rc;
    SimHookBlock b(f);
    const auto d_par = b.in(params, TRK_PARAMS * m); const auto d_adv = b.in(adv, m); const auto d_tick = b.in(tick, m);
    const auto d_cs = b.in(cap_slots, 2 * m); const auto d_doff = b.in(det_off, m + 1); const auto d_dets = b.in(dets, 6 * nd);
    const auto d_tab = b.inout(tab.data(), TAB * m); const auto d_n = b.inout(n0.data(), m); const auto d_id = b.inout(next_id, m);
    const auto d_out = b.out<double>(OUT * m); const auto d_nout = b.out<int32_t>(m); const auto d_asg = b.out<int32_t>(nd);
    const auto d_rec = b.out<double>(SD * m);
    if ((rc = b.upload())) return rc;
    hipLaunchKernelGGL(k_fleet_sim_tracker_eval, dim3((unsigned)m), dim3(64), 0, f->h->stream, d_par, d_adv, d_tick, d_cs, d_tab, d_n, d_id, d_doff, d_dets,
                       d_out, d_nout, d_asg, d_rec);
    FLEET_TRY(f, hipGetLastError());
    if ((rc = b.fetch(tracks_out, d_tab, TAB * m))) return rc;
    if ((rc = b.fetch(n_tracks_out, d_n, m))) return rc;
    if ((rc = b.fetch(next_id_out, d_id, m))) return rc;
    if ((rc = b.fetch(out, d_out, OUT * m))) return rc;
    if ((rc = b.fetch(n_out, d_nout, m))) return rc;
    if ((rc = b.fetch(rec, d_rec, SD * m))) return rc;
    if ((rc = b.fetch(assign, d_asg, nd))) return rc;
    if ((rc = b.finish())) return rc;
    for (size_t q = 0; q < m; ++q)          // (rows behind the new count hold what the compaction left there)
        for (size_t c = (size_t)(n_tracks_out[q] > 0 ? n_tracks_out[q] : 0) * RD; c < TAB; ++c) tracks_out[q * TAB + c] = NAN;
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

// ---------------------------------------------------------------------------------------------------------------------
// prediction model (ltpl_fleet_sim_predictor, include/ltpl_hip.h; the rule: fleet_predict.hpp)
// ---------------------------------------------------------------------------------------------------------------------
// q[PRD_PARAMS] = mode, horizon, relax, d_max
static bool sim_pred_params_ok(const double* q, std::string* why)
{
    const double mode = q[0], horizon = q[1], relax = q[2], d_max = q[3];
    if (!(mode == 0.0 || mode == 1.0 || mode == 2.0)) { *why = "mode must be 0, 1 or 2"; return false; }
    if (!std::isfinite(horizon) || !(horizon > 0.0)) { *why = "horizon must be finite and positive"; return false; }
    if (!(relax >= 0.0) || !(relax <= 1.0)) { *why = "relax must lie in [0, 1]"; return false; }
    if (!(d_max >= 0.0)) { *why = "d_max must not be negative or NaN"; return false; }
    return true;
}

// every argument is checked before the first HIP call
static int sim_check_predictor(ltpl_fleet* f, const ltpl_fleet_sim_predictor_in* in, std::vector<double>* par)
{
    const int N = f->D.N;
    auto bad = [&](const std::string& why, int code = LTPL_ERR_INVALID_ARG) { f->err = "fleet sim predictor: " + why; return code; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    if (!in) return LTPL_OK;
    if (in->n_points < 1 || in->n_points > LTPL_FLEET_SIM_PREDICTOR_MAX_POINTS) return bad("n_points must lie in 1 .. 8");
    const SimCol col[PRD_PARAMS] = {{"mode", in->mode}, {"horizon", in->horizon}, {"relax", in->relax}, {"d_max", in->d_max}};
    if (int rc = sim_param_table(f, "predictor", col, sim_no_head, [](int, const double* q, std::string* why) { return sim_pred_params_ok(q, why); }, par))
        return rc;
    // the path kernel's per-position arrays hold MAX_POS entries and the simulation hands its objects on without the per-call check
    for (int p = 0; p < N; ++p)
        if (f->sim->slots[(size_t)p] * (1 + in->n_points) > MAX_POS)
            return bad("planner " + std::to_string(p) + ": (opponents + statics + mates) x (1 + n_points) = " +
                       std::to_string(f->sim->slots[(size_t)p] * (1 + in->n_points)) + " positions, above 192", LTPL_ERR_CAPACITY);
    return LTPL_OK;
}

extern "C" int ltpl_fleet_sim_predictor(ltpl_fleet* f, const ltpl_fleet_sim_predictor_in* in)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    std::vector<double> par;
    int rc = sim_check_predictor(f, in, &par);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FleetSim& s = *f->sim;
    if (!in && !s.pred.on) return LTPL_OK;
    // everything new is allocated first; the fleet keeps its previous predictor, its staging and its records unless every step succeeds
    const int stride = in ? 1 + in->n_points : 2;
    SimStage st;
    if ((rc = sim_stage_alloc(f, s.slots, stride, &st))) return rc;
    if (!in) {
        sim_stage_commit(&s, &st);
        s.pred.clear();
        return LTPL_OK;
    }
    const size_t N = (size_t)f->D.N;
    SimAllocs al;
    SimPred pd{};
    double* d_par = nullptr;
    if ((rc = sim_upload(f, al.p, par.data(), par.size(), &d_par))) return rc;
    if ((rc = sim_upload(f, al.p, (const double*)nullptr, N * LTPL_FLEET_SIM_PREDICTOR_DOUBLES, &pd.rec))) return rc;
    pd.par = d_par; pd.K = in->n_points;
    sim_stage_commit(&s, &st);
    s.pred.commit(al, pd);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_predictor_read(ltpl_fleet* f, double* out, int32_t doubles_per_planner)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    return sim_read_records(f, "predictor", &FleetSim::pred, "the predictor is off (ltpl_fleet_sim_predictor first)", out, doubles_per_planner,
                            LTPL_FLEET_SIM_PREDICTOR_DOUBLES);
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_predictor_eval(ltpl_fleet* f, int32_t n_cases, int32_t n_points, const double* params, const int32_t* obj_off,
                                             const double* objs, double* points, int32_t* outcome, double* rec)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const std::string& why) { f->err = "fleet sim predictor eval: " + why; return LTPL_ERR_INVALID_ARG; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first (the hook runs on the simulation's race-line table)");
    if (n_cases < 0) return bad("n_cases must not be negative");
    if (n_points < 1 || n_points > LTPL_FLEET_SIM_PREDICTOR_MAX_POINTS) return bad("n_points must lie in 1 .. 8");
    if (n_cases == 0) return LTPL_OK;
    if (!params || !obj_off || !rec) return bad("params / obj_off / rec missing");
    if (obj_off[0] != 0) return bad("object offsets must start at 0");
    for (int q = 0; q < n_cases; ++q) {
        const std::string who = "case " + std::to_string(q) + ": ";
        const int n = obj_off[q + 1] - obj_off[q];
        if (n < 0 || n > SIM_OBJ_CAP) return bad(who + "0 .. 96 objects");
        std::string why;
        if (!sim_pred_params_ok(params + (size_t)q * PRD_PARAMS, &why)) return bad(who + why);
    }
    const size_t m = (size_t)n_cases, no = (size_t)obj_off[n_cases], K = (size_t)n_points;
    if (no > 0 && (!objs || !points || !outcome)) return bad("objs / points / outcome missing");
    constexpr size_t PER = (size_t)SIM_OBJ_CAP * (1 + LTPL_FLEET_SIM_PREDICTOR_MAX_POINTS), SD = LTPL_FLEET_SIM_PREDICTOR_DOUBLES;
    int rc = fleet_enter(f);
    if (rc) return rc;
    SimHookBlock b(f);
    const auto d_par = b.in(params, PRD_PARAMS * m); const auto d_off = b.in(obj_off, m + 1); const auto d_objs = b.in(objs, 5 * no);
    const auto d_x = b.out<double>(PER * m); const auto d_y = b.out<double>(PER * m); const auto d_oc = b.out<int32_t>(no);
    const auto d_rec = b.out<double>(SD * m);
    if ((rc = b.upload())) return rc;
    hipLaunchKernelGGL(k_fleet_sim_predictor_eval, dim3((unsigned)m), dim3(64), 0, f->h->stream, f->sim->sd, d_par, n_points, d_off, d_objs, d_x, d_y, d_oc,
                       d_rec);
    FLEET_TRY(f, hipGetLastError());
    std::vector<double> hx(PER * m), hy(PER * m);
    if ((rc = b.fetch(hx.data(), d_x, PER * m))) return rc;
    if ((rc = b.fetch(hy.data(), d_y, PER * m))) return rc;
    if ((rc = b.fetch(rec, d_rec, SD * m))) return rc;
    if ((rc = b.fetch(outcome, d_oc, no))) return rc;
    if ((rc = b.finish())) return rc;
    // points[object][1 + n_points][2]: the device's layout of the tick (own position, then the K points), objects in case order
    for (size_t q = 0; q < m; ++q)
        for (size_t i = 0, n = (size_t)(obj_off[q + 1] - obj_off[q]); i < n; ++i)
            for (size_t j = 0; j <= K; ++j) {
                double* o = points + (((size_t)obj_off[q] + i) * (1 + K) + j) * 2;
                o[0] = hx[q * PER + (1 + K) * i + j]; o[1] = hy[q * PER + (1 + K) * i + j];
            }
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

// ---------------------------------------------------------------------------------------------------------------------
// behaviour selector (ltpl_fleet_sim_selector, include/ltpl_hip.h; the rule: fleet_select.hpp)
// ---------------------------------------------------------------------------------------------------------------------
static bool sim_sel_params_ok(const double* q, std::string* why)
{
    for (int c = 0; c < SLC_PARAMS; ++c) if (q[c] != q[c]) { *why = "a parameter is NaN"; return false; }
    if (!(q[0] > 0.0)) { *why = "horizon must be positive"; return false; }
    if (!(q[1] >= 0.0)) { *why = "r_ego must not be negative"; return false; }
    if (!(q[4] >= 0.0)) { *why = "w_clear must not be negative"; return false; }
    if (!(q[5] >= 0.0)) { *why = "w_switch must not be negative"; return false; }
    return true;
}

// every argument is checked before the first HIP call
static int sim_check_selector(ltpl_fleet* f, const ltpl_fleet_sim_selector_in* in, std::vector<double>* par)
{
    auto bad = [&](const std::string& why) { f->err = "fleet sim selector: " + why; return LTPL_ERR_INVALID_ARG; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    if (!in) return LTPL_OK;
    if (!in->on) return bad("on missing");
    const SimCol col[SLC_PARAMS] = {{"horizon", in->horizon}, {"r_ego", in->r_ego}, {"c_hard", in->c_hard}, {"c_soft", in->c_soft}, {"w_clear", in->w_clear},
                                    {"w_switch", in->w_switch}};
    return sim_param_table(f, "selector", col, sim_no_head, [](int, const double* q, std::string* why) { return sim_sel_params_ok(q, why); }, par);
}

extern "C" int ltpl_fleet_sim_selector(ltpl_fleet* f, const ltpl_fleet_sim_selector_in* in)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    std::vector<double> par;
    int rc = sim_check_selector(f, in, &par);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FleetSim& s = *f->sim;
    if (!in) {
        s.sel.clear();
        return LTPL_OK;
    }
    // everything new is allocated first; the fleet keeps its previous selector and its records unless every step succeeds
    const size_t N = (size_t)f->D.N, n_pref = (size_t)s.pref_off[N];
    std::vector<int> on(N);
    for (size_t p = 0; p < N; ++p) on[p] = in->on[p] ? 1 : 0;
    std::vector<double> rec(N * LTPL_FLEET_SIM_SELECTOR_DOUBLES, 0.0);
    for (size_t p = 0; p < N; ++p) rec[p * LTPL_FLEET_SIM_SELECTOR_DOUBLES + fleet::SLS_CLEAR_MIN] = INFINITY;
    SimAllocs al;
    SimSel sl{};
    double* d_par = nullptr; int* d_on = nullptr;
    if ((rc = sim_upload(f, al.p, par.data(), par.size(), &d_par))) return rc;
    if ((rc = sim_upload(f, al.p, on.data(), N, &d_on))) return rc;
    if ((rc = sim_upload(f, al.p, (const int*)nullptr, n_pref, &sl.ord))) return rc;
    if ((rc = sim_upload(f, al.p, rec.data(), rec.size(), &sl.rec))) return rc;
    FLEET_TRY(f, hipMemcpy(sl.ord, s.sd.pref, sizeof(int) * n_pref, hipMemcpyDeviceToDevice));     // until the first tick: the user's lists
    sl.par = d_par; sl.on = d_on;
    s.sel.commit(al, sl);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_selector_read(ltpl_fleet* f, double* out, int32_t doubles_per_planner, int32_t* ordered, int32_t n_ordered)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const std::string& why) { f->err = "fleet sim selector: " + why; return LTPL_ERR_INVALID_ARG; };
    int rc = sim_read_records(f, "selector", &FleetSim::sel, "the selector is off (ltpl_fleet_sim_selector first)", out, "out", doubles_per_planner,
                              LTPL_FLEET_SIM_SELECTOR_DOUBLES, [&] {
        const int n_pref = f->sim->pref_off[(size_t)f->D.N];
        if (ordered && n_ordered != n_pref)
            return bad("n_ordered is " + std::to_string(n_ordered) + ", the preference lists hold " + std::to_string(n_pref) + " entries");
        return LTPL_OK;
    });
    if (rc) return rc;
    if (ordered) FLEET_TRY(f, hipMemcpy(ordered, f->sim->sel.dev.ord, sizeof(int) * (size_t)n_ordered, hipMemcpyDeviceToHost));
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_selector_eval(ltpl_fleet* f, int32_t n_cases, const double* params, const int32_t* lists, const int32_t* n_rows,
                                            const double* rows, const int32_t* obj_off, const double* objs, int32_t* ordered, double* act_d,
                                            int32_t* act_i, double* rec)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const std::string& why) { f->err = "fleet sim selector eval: " + why; return LTPL_ERR_INVALID_ARG; };
    if (n_cases < 0) return bad("n_cases must not be negative");
    if (n_cases == 0) return LTPL_OK;
    if (!params || !lists || !n_rows || !rows || !obj_off || !ordered || !act_d || !act_i || !rec) return bad("an array is missing");
    if (obj_off[0] != 0) return bad("object offsets must start at 0");
    constexpr int A = fleet::kSelActions;
    for (int q = 0; q < n_cases; ++q) {
        const std::string who = "case " + std::to_string(q) + ": ";
        const int n = obj_off[q + 1] - obj_off[q];
        if (n < 0 || n > SIM_OBJ_CAP) return bad(who + "0 .. 96 objects");
        std::string why;
        if (!sim_sel_params_ok(params + (size_t)q * SLC_PARAMS, &why)) return bad(who + why);
        const int32_t* li = lists + (size_t)q * 8;
        if (li[0] < 1 || li[0] > LTPL_FLEET_SIM_MAX_PREF) return bad(who + "a preference list needs 1 .. 5 entries");
        for (int e = 0; e < li[0]; ++e) if (li[3 + e] < LTPL_ACT_STRAIGHT || li[3 + e] > LTPL_ACT_EMERGENCY) return bad(who + "unknown action in the preference list");
        for (int a = 0; a < A; ++a) if (n_rows[(size_t)q * A + a] < -1 || n_rows[(size_t)q * A + a] > LTPL_FLEET_SIM_MAX_EXPORT) return bad(who + "rows must lie in -1 .. 256");
    }
    const size_t m = (size_t)n_cases, no = (size_t)obj_off[n_cases];
    if (no > 0 && !objs) return bad("objs missing");
    constexpr size_t RW = (size_t)A * 4 * LTPL_FLEET_SIM_MAX_EXPORT, SD = LTPL_FLEET_SIM_SELECTOR_DOUBLES, MP = LTPL_FLEET_SIM_MAX_PREF;
    int rc = fleet_enter(f);
    if (rc) return rc;
    SimHookBlock b(f);
    const auto d_par = b.in(params, SLC_PARAMS * m); const auto d_li = b.in(lists, 8 * m); const auto d_nr = b.in(n_rows, A * m);
    const auto d_rows = b.in(rows, RW * m); const auto d_off = b.in(obj_off, m + 1); const auto d_objs = b.in(objs, 5 * no);
    const auto d_ord = b.out<int32_t>(MP * m); const auto d_act = b.out<fleet::SelAct>(A * m); const auto d_rec = b.inout(rec, SD * m);
    if ((rc = b.upload())) return rc;
    hipLaunchKernelGGL(k_fleet_sim_selector_eval, dim3((unsigned)m), dim3(64), 0, f->h->stream, d_par, d_li, d_nr, d_rows, d_off, d_objs, d_ord, d_act, d_rec);
    FLEET_TRY(f, hipGetLastError());
    std::vector<fleet::SelAct> act(A * m);
    if ((rc = b.fetch(act.data(), d_act, A * m))) return rc;
    if ((rc = b.fetch(rec, d_rec, SD * m))) return rc;
    if ((rc = b.fetch(ordered, d_ord, MP * m))) return rc;
    if ((rc = b.finish())) return rc;
    for (size_t i = 0; i < A * m; ++i) {
        act_d[3 * i] = act[i].vbar; act_d[3 * i + 1] = act[i].clear; act_d[3 * i + 2] = act[i].J;
        act_i[2 * i] = act[i].clear_obj; act_i[2 * i + 1] = act[i].flags;
    }
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

// ---------------------------------------------------------------------------------------------------------------------
// safety monitor (ltpl_fleet_sim_safety, include/ltpl_hip.h; the rule: fleet_safety.hpp)
// ---------------------------------------------------------------------------------------------------------------------
static bool sim_safety_params_ok(const double* q, std::string* why)
{
    static const char* const name[SAF_PARAMS] = {"r_ego", "ttc_thr", "drac_thr", "thw_thr", "margin"};
    for (int c = 0; c < SAF_PARAMS; ++c) {
        if (!std::isfinite(q[c])) { *why = std::string(name[c]) + " must be finite"; return false; }
        if (c == 1 ? !(q[c] > 0.0) : !(q[c] >= 0.0)) { *why = std::string(name[c]) + (c == 1 ? " must be positive" : " must not be negative"); return false; }
    }
    return true;
}

// every argument is checked before the first HIP call
static int sim_check_safety(ltpl_fleet* f, const ltpl_fleet_sim_safety_in* in, std::vector<double>* par)
{
    auto bad = [&](const std::string& why) { f->err = "fleet sim safety: " + why; return LTPL_ERR_INVALID_ARG; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    if (!in) return LTPL_OK;
    if (!in->on) return bad("on missing");
    const SimCol col[SAF_PARAMS] = {{"r_ego", in->r_ego}, {"ttc_thr", in->ttc_thr}, {"drac_thr", in->drac_thr}, {"thw_thr", in->thw_thr}, {"margin", in->margin}};
    auto head = [&]() -> const char* {
        return in->tick0 < 0 ? "tick0 must not be negative" : (in->flags & ~(uint32_t)LTPL_SIM_SAFETY_KEEP_STATE) ? "unknown flag" : nullptr;
    };
    return sim_param_table(f, "safety", col, head, [&](int p, const double* q, std::string* why) {
        if (in->on[p] != 0 && in->on[p] != 1) { *why = "on must be 0 or 1"; return false; }
        return sim_safety_params_ok(q, why);
    }, par);
}

extern "C" int ltpl_fleet_sim_safety(ltpl_fleet* f, const ltpl_fleet_sim_safety_in* in)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    std::vector<double> par;
    int rc = sim_check_safety(f, in, &par);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FleetSim& s = *f->sim;
    if (!in) {
        s.saf.clear();
        return LTPL_OK;
    }
    const size_t N = (size_t)f->D.N;
    constexpr size_t RD = LTPL_FLEET_SIM_SAFETY_DOUBLES, RI = SAF_RING;
    const bool keep = (in->flags & LTPL_SIM_SAFETY_KEEP_STATE) && s.saf.on;
    std::vector<double> rec(N * RD), inc(N * RI);
    if (keep) {
        FLEET_TRY(f, hipMemcpy(rec.data(), s.saf.dev.rec, 8 * N * RD, hipMemcpyDeviceToHost));
        FLEET_TRY(f, hipMemcpy(inc.data(), s.saf.dev.inc, 8 * N * RI, hipMemcpyDeviceToHost));
    } else {
        for (size_t p = 0; p < N; ++p) fleet::safety_start(rec.data() + p * RD, inc.data() + p * RI);
    }
    // everything new is allocated first; the fleet keeps its previous monitor, its tick count, records and rings unless every step succeeds
    SimAllocs al;
    SimSafety sf{};
    double* d_par = nullptr; int* d_on = nullptr;
    if ((rc = sim_upload(f, al.p, par.data(), par.size(), &d_par))) return rc;
    if ((rc = sim_upload(f, al.p, in->on, N, &d_on))) return rc;
    if ((rc = sim_upload(f, al.p, rec.data(), rec.size(), &sf.rec))) return rc;
    if ((rc = sim_upload(f, al.p, inc.data(), inc.size(), &sf.inc))) return rc;
    sf.par = d_par; sf.on = d_on;
    s.saf.commit(al, sf, in->tick0);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_safety_read(ltpl_fleet* f, double* out, int32_t doubles_per_planner, double* incidents, int32_t doubles_per_incident)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const std::string& why) { f->err = "fleet sim safety: " + why; return LTPL_ERR_INVALID_ARG; };
    int rc = sim_read_records(f, "safety", &FleetSim::saf, "the monitor is off (ltpl_fleet_sim_safety first)", out, "out", doubles_per_planner,
                              LTPL_FLEET_SIM_SAFETY_DOUBLES, [&] {
        if (incidents && doubles_per_incident != LTPL_FLEET_SIM_SAFETY_INCIDENT_DOUBLES) return bad("incident size mismatch");
        return LTPL_OK;
    });
    if (rc) return rc;
    if (incidents) FLEET_TRY(f, hipMemcpy(incidents, f->sim->saf.dev.inc, sizeof(double) * (size_t)f->D.N * SAF_RING, hipMemcpyDeviceToHost));
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_safety_eval(ltpl_fleet* f, int32_t n_cases, const double* pose, const double* dt, const int32_t* tick, const double* params,
                                          const int32_t* obj_off, const double* objs, double* rec, double* inc, double* per_obj, double* per_tick)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const std::string& why) { f->err = "fleet sim safety eval: " + why; return LTPL_ERR_INVALID_ARG; };
    if (n_cases < 0) return bad("n_cases must not be negative");
    if (n_cases == 0) return LTPL_OK;
    if (!pose || !dt || !tick || !params || !obj_off || !rec || !inc || !per_tick) return bad("an array is missing");
    if (obj_off[0] != 0) return bad("object offsets must start at 0");
    for (int q = 0; q < n_cases; ++q) {
        const std::string who = "case " + std::to_string(q) + ": ";
        const int n = obj_off[q + 1] - obj_off[q];
        if (n < 0 || n > SIM_OBJ_CAP) return bad(who + "0 .. 96 objects");
        std::string why;
        if (!sim_safety_params_ok(params + (size_t)q * SAF_PARAMS, &why)) return bad(who + why);
        if (!std::isfinite(dt[q]) || !(dt[q] > 0.0)) return bad(who + "dt must be finite and positive");
        if (tick[q] < 0) return bad(who + "tick must not be negative");
    }
    const size_t m = (size_t)n_cases, no = (size_t)obj_off[n_cases];
    if (no > 0 && (!objs || !per_obj)) return bad("objs / per_obj missing");
    constexpr size_t RD = LTPL_FLEET_SIM_SAFETY_DOUBLES, RI = SAF_RING;
    int rc = fleet_enter(f);
    if (rc) return rc;
    SimHookBlock b(f);
    const auto d_pose = b.in(pose, 2 * m); const auto d_dt = b.in(dt, m); const auto d_tick = b.in(tick, m); const auto d_par = b.in(params, SAF_PARAMS * m);
    const auto d_off = b.in(obj_off, m + 1); const auto d_objs = b.in(objs, 5 * no);
    const auto d_rec = b.inout(rec, RD * m); const auto d_inc = b.inout(inc, RI * m);
    const auto d_po = b.out<double>(6 * no); const auto d_pt = b.out<double>(8 * m);
    if ((rc = b.upload())) return rc;
    hipLaunchKernelGGL(k_fleet_sim_safety_eval, dim3((unsigned)m), dim3(64), 0, f->h->stream, d_pose, d_dt, d_tick, d_par, d_off, d_objs, d_rec, d_inc, d_po,
                       d_pt);
    FLEET_TRY(f, hipGetLastError());
    if ((rc = b.fetch(rec, d_rec, RD * m))) return rc;
    if ((rc = b.fetch(inc, d_inc, RI * m))) return rc;
    if ((rc = b.fetch(per_tick, d_pt, 8 * m))) return rc;
    if ((rc = b.fetch(per_obj, d_po, 6 * no))) return rc;
    return b.finish();
} LTPL_ABI_CATCH(abi_err_of(f))

// ---------------------------------------------------------------------------------------------------------------------
// reactive opponents (ltpl_fleet_sim_react, include/ltpl_hip.h; the rule: fleet_react.hpp)
// ---------------------------------------------------------------------------------------------------------------------
static const char* const kReactParamName[RCT_PARAMS] = {"on", "a_max", "b_comf", "b_max", "headway", "gap0", "look", "lat_gate", "ego_len"};

// q[RCT_PARAMS] in the order of fleet::ReactParams
static bool sim_react_params_ok(const double* q, std::string* why)
{
    if (q[0] != 0.0 && q[0] != 1.0) { *why = "on must be 0 or 1"; return false; }
    for (int c = 1; c < RCT_PARAMS; ++c) {
        const bool positive = c <= 3 || c == 6;              // a_max, b_comf, b_max, look
        if (std::isnan(q[c]) || (std::isinf(q[c]) && !(c == 6 && q[c] > 0.0))) { *why = std::string(kReactParamName[c]) + " must be finite"; return false; }
        if (positive ? !(q[c] > 0.0) : !(q[c] >= 0.0)) { *why = std::string(kReactParamName[c]) + (positive ? " must be positive" : " must not be negative"); return false; }
    }
    return true;
}

// every argument is checked before the first HIP call; *any_on: some planner has on == 1
static int sim_check_react(ltpl_fleet* f, const ltpl_fleet_sim_react_in* in, std::vector<double>* par, bool* any_on)
{
    auto bad = [&](const std::string& why) { f->err = "fleet sim react: " + why; return LTPL_ERR_INVALID_ARG; };
    *any_on = false;
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    if (!in) return LTPL_OK;
    const char* const* nm = kReactParamName;
    const SimCol col[RCT_PARAMS] = {{nm[0], in->on}, {nm[1], in->a_max}, {nm[2], in->b_comf}, {nm[3], in->b_max}, {nm[4], in->headway}, {nm[5], in->gap0},
                                    {nm[6], in->look}, {nm[7], in->lat_gate}, {nm[8], in->ego_len}};
    auto head = [&]() -> const char* {
        return in->tick0 < 0 ? "tick0 must not be negative" : (in->flags & ~(uint32_t)LTPL_SIM_REACT_KEEP_STATE) ? "unknown flag" : nullptr;
    };
    return sim_param_table(f, "react", col, head, [&](int, const double* q, std::string* why) {
        if (!sim_react_params_ok(q, why)) return false;
        *any_on = *any_on || q[0] == 1.0;
        return true;
    }, par);
}

extern "C" int ltpl_fleet_sim_react(ltpl_fleet* f, const ltpl_fleet_sim_react_in* in)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    std::vector<double> par;
    bool any_on = false;
    int rc = sim_check_react(f, in, &par, &any_on);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FleetSim& s = *f->sim;
    if (!in || !any_on) {
        s.react.clear();
        return LTPL_OK;
    }
    const size_t N = (size_t)f->D.N, no = (size_t)s.n_opp;
    constexpr size_t RD = LTPL_FLEET_SIM_REACT_DOUBLES;
    const bool keep = (in->flags & LTPL_SIM_REACT_KEEP_STATE) && s.react.on;
    std::vector<double> rec(N * RD), eff(no ? no : 1);
    if (keep) {
        FLEET_TRY(f, hipMemcpy(rec.data(), s.react.dev.rec, 8 * N * RD, hipMemcpyDeviceToHost));
        if (no) FLEET_TRY(f, hipMemcpy(eff.data(), s.react.dev.eff, 8 * no, hipMemcpyDeviceToHost));
    } else {
        for (size_t p = 0; p < N; ++p) fleet::react_start(rec.data() + p * RD);
        if (no) FLEET_TRY(f, hipMemcpy(eff.data(), s.sd.opp_scale, 8 * no, hipMemcpyDeviceToHost));      // the start state: e = the configured c
    }
    // everything new is allocated first; the fleet keeps its previous model, its tick count, scales and records unless every step succeeds
    SimAllocs al;
    SimReact r{};
    double* d_par = nullptr;
    if ((rc = sim_upload(f, al.p, par.data(), par.size(), &d_par))) return rc;
    if ((rc = sim_upload(f, al.p, eff.data(), no, &r.eff))) return rc;
    if ((rc = sim_upload(f, al.p, rec.data(), rec.size(), &r.rec))) return rc;
    r.par = d_par;
    s.react.commit(al, r, in->tick0);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_react_read(ltpl_fleet* f, double* out, int32_t doubles_per_planner, double* eff_scale)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    int rc = sim_read_records(f, "react", &FleetSim::react, "the model is off (ltpl_fleet_sim_react first)", out, doubles_per_planner,
                              LTPL_FLEET_SIM_REACT_DOUBLES);
    if (rc) return rc;
    const size_t no = (size_t)f->sim->n_opp;
    if (eff_scale && no) FLEET_TRY(f, hipMemcpy(eff_scale, f->sim->react.dev.eff, sizeof(double) * no, hipMemcpyDeviceToHost));
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_react_eval(ltpl_fleet* f, int32_t n_cases, const double* params, const double* ego, const double* dt, const int32_t* tick,
                                         const int32_t* opp_off, const double* opp, double* rec, double* e_out, double* per_opp, double* ego_out)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const std::string& why) { f->err = "fleet sim react eval: " + why; return LTPL_ERR_INVALID_ARG; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first (the race table)");
    if (n_cases < 0) return bad("n_cases must not be negative");
    if (n_cases == 0) return LTPL_OK;
    if (!params || !ego || !dt || !tick || !opp_off || !rec || !ego_out) return bad("an array is missing");
    if (opp_off[0] != 0) return bad("opponent offsets must start at 0");
    for (int q = 0; q < n_cases; ++q) {
        const std::string who = "case " + std::to_string(q) + ": ";
        const int n = opp_off[q + 1] - opp_off[q];
        if (n < 0 || n > SIM_OBJ_CAP) return bad(who + "0 .. 96 opponents");
        std::string why;
        if (!sim_react_params_ok(params + (size_t)q * RCT_PARAMS, &why)) return bad(who + why);
        if (!std::isfinite(dt[q]) || !(dt[q] > 0.0)) return bad(who + "dt must be finite and positive");
        if (tick[q] < 0) return bad(who + "tick must not be negative");
    }
    const size_t m = (size_t)n_cases, no = (size_t)opp_off[n_cases];
    if (no > 0 && (!opp || !e_out || !per_opp)) return bad("opp / e_out / per_opp missing");
    for (size_t i = 0; i < 4 * no; ++i) if (!std::isfinite(opp[i])) return bad("opponent " + std::to_string(i / 4) + ": s, c, e and length must be finite");
    constexpr size_t RD = LTPL_FLEET_SIM_REACT_DOUBLES;
    int rc = fleet_enter(f);
    if (rc) return rc;
    SimHookBlock b(f);
    const auto d_par = b.in(params, RCT_PARAMS * m); const auto d_ego = b.in(ego, 3 * m); const auto d_dt = b.in(dt, m); const auto d_tick = b.in(tick, m);
    const auto d_off = b.in(opp_off, m + 1); const auto d_opp = b.in(opp, 4 * no);
    const auto d_rec = b.inout(rec, RD * m);
    const auto d_e = b.out<double>(no); const auto d_po = b.out<double>(4 * no); const auto d_eo = b.out<double>(3 * m);
    if ((rc = b.upload())) return rc;
    hipLaunchKernelGGL(k_fleet_sim_react_eval, dim3((unsigned)m), dim3(64), 0, f->h->stream, f->sim->sd, d_par, d_ego, d_dt, d_tick, d_off, d_opp, d_rec, d_e,
                       d_po, d_eo);
    FLEET_TRY(f, hipGetLastError());
    if ((rc = b.fetch(rec, d_rec, RD * m))) return rc;
    if ((rc = b.fetch(ego_out, d_eo, 3 * m))) return rc;
    if ((rc = b.fetch(e_out, d_e, no))) return rc;
    if ((rc = b.fetch(per_opp, d_po, 4 * no))) return rc;
    return b.finish();
} LTPL_ABI_CATCH(abi_err_of(f))

// ---------------------------------------------------------------------------------------------------------------------
// campaign statistics (ltpl_fleet_sim_stats, include/ltpl_hip.h; the rule: fleet_stats.hpp)
// ---------------------------------------------------------------------------------------------------------------------
static const char* const kStatsFamily[fleet::STA_FAMILIES] = {"telemetry", "vehicle", "sensor", "tracker", "predictor", "selector", "safety", "react", "state"};
static const int kStatsColumns[fleet::STA_FAMILIES] = {LTPL_FLEET_SIM_TELE_DOUBLES, LTPL_FLEET_SIM_VEH_DOUBLES, LTPL_FLEET_SIM_SENSOR_DOUBLES,
                                                       LTPL_FLEET_SIM_TRACKER_DOUBLES, LTPL_FLEET_SIM_PREDICTOR_DOUBLES, LTPL_FLEET_SIM_SELECTOR_DOUBLES,
                                                       LTPL_FLEET_SIM_SAFETY_DOUBLES, LTPL_FLEET_SIM_REACT_DOUBLES, 1};
#define STA_MAX_GROUPS 4096
#define STA_MAX_MEASURES 64
#define STA_MAX_SERIES_BYTES ((size_t)256 << 20)

// the records of family `fam` as they are now (null: the module is off)
static const double* sim_stats_records(const FleetSim& s, int fam)
{
    switch (fam) {
    case fleet::STA_FAM_TELEMETRY: return s.tele.on ? s.tele.dev.rec : nullptr;
    case fleet::STA_FAM_VEHICLE: return s.veh.on ? s.veh.dev.rec : nullptr;
    case fleet::STA_FAM_SENSOR: return s.sens.on ? s.sens.dev.rec : nullptr;
    case fleet::STA_FAM_TRACKER: return s.trk.on ? s.trk.dev.rec : nullptr;
    case fleet::STA_FAM_PREDICTOR: return s.pred.on ? s.pred.dev.rec : nullptr;
    case fleet::STA_FAM_SELECTOR: return s.sel.on ? s.sel.dev.rec : nullptr;
    case fleet::STA_FAM_SAFETY: return s.saf.on ? s.saf.dev.rec : nullptr;
    case fleet::STA_FAM_REACT: return s.react.on ? s.react.dev.rec : nullptr;
    }
    return nullptr;
}
static int sim_stats_sources(ltpl_fleet* f, SimStats* st)
{
    const FleetSim& s = *f->sim;
    for (double const*& r : st->rec) r = nullptr;
    for (int fam : s.sp.fam) {
        if (fam == fleet::STA_FAM_STATE) continue;
        if (!(st->rec[fam] = sim_stats_records(s, fam))) {
            f->err = std::string("fleet sim stats: family ") + kStatsFamily[fam] + " is off (a measure of the plan reads its records)";
            return LTPL_ERR_INVALID_ARG;
        }
    }
    st->state = f->d_state; st->state_stride = f->D.stride;
    return LTPL_OK;
}
// k_fleet_sim_stats_chunk (or, with `raw`, the hook's kernel) and k_fleet_sim_stats_merge on the fleet's stream
static int sim_stats_launch(ltpl_fleet* f, const SimStats& st, int n_chunks, const double* raw, double* rows, double* tops)
{
    hipStream_t sm = f->h->stream;
    if (n_chunks > 0) {
        if (raw) hipLaunchKernelGGL(k_fleet_sim_stats_eval, dim3((unsigned)n_chunks), dim3(64), 0, sm, st, raw);
        else hipLaunchKernelGGL(k_fleet_sim_stats_chunk, dim3((unsigned)n_chunks), dim3(64), 0, sm, st);
        FLEET_TRY(f, hipGetLastError());
    }
    hipLaunchKernelGGL(k_fleet_sim_stats_merge, dim3((unsigned)(st.G * st.M)), dim3(64), 0, sm, st, rows, tops);
    FLEET_TRY(f, hipGetLastError());
    return LTPL_OK;
}
static int sim_stats_series_row(ltpl_fleet* f, uint32_t tick)
{
    FleetSim& s = *f->sim;
    SimStats st = s.stats.dev;
    int rc = sim_stats_sources(f, &st);
    if (rc) return rc;
    const size_t slot = (size_t)(s.sp.n_rows % s.sp.depth), row = (size_t)st.G * st.M * LTPL_FLEET_SIM_STATS_DOUBLES;
    if ((rc = sim_stats_launch(f, st, s.sp.n_chunks, nullptr, s.sp.ring + slot * row, s.sp.tops))) return rc;
    s.sp.ring_tick[slot] = (int32_t)tick;
    ++s.sp.n_rows;
    return LTPL_OK;
}

// the chunks of groups with the member offsets off[0 .. G]: group, first member and count per chunk, and the groups' chunk offsets
struct StatsChunks { std::vector<int> group, first, cnt, g_choff; };
template <class Off>
static StatsChunks sim_stats_chunks(const Off* off, int G)
{
    StatsChunks c;
    c.g_choff.assign((size_t)G + 1, 0);
    for (int g = 0; g < G; ++g) {
        for (int i = (int)off[g]; i < (int)off[g + 1]; i += fleet::kStatsChunk) {
            c.group.push_back(g); c.first.push_back(i);
            c.cnt.push_back((int)off[g + 1] - i < fleet::kStatsChunk ? (int)off[g + 1] - i : (int)fleet::kStatsChunk);
        }
        c.g_choff[(size_t)g + 1] = (int)c.group.size();
    }
    return c;
}
// lo / hi / bins / top_dir of one measure or case; null: fine
static const char* sim_stats_spec_bad(double lo, double hi, double bins, double top_dir)
{
    if (!(bins >= 1.0 && bins <= (double)fleet::kStatsBins) || bins != std::floor(bins)) return "bins must be 1 .. 16";
    if (!std::isfinite(lo) || !std::isfinite(hi)) return "lo and hi must be finite";
    if (!(lo < hi)) return "lo must be below hi";
    if (top_dir != -1.0 && top_dir != 0.0 && top_dir != 1.0) return "top_dir must be -1, 0 or +1";
    return nullptr;
}

// every argument is checked before the first HIP call
static int sim_check_stats(ltpl_fleet* f, const ltpl_fleet_sim_stats_in* in, bool* keep)
{
    auto bad = [&](const std::string& why, int code = LTPL_ERR_INVALID_ARG) { f->err = "fleet sim stats: " + why; return code; };
    *keep = false;
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    if (!in) return LTPL_OK;
    const FleetSim& s = *f->sim;
    const int N = f->D.N;
    if (in->n_groups < 1 || in->n_groups > STA_MAX_GROUPS) return bad("n_groups must be 1 .. 4096");
    if (!in->group) return bad("group missing");
    for (int p = 0; p < N; ++p)
        if (in->group[p] < -1 || in->group[p] >= in->n_groups) return bad("planner " + std::to_string(p) + ": group must be -1 .. n_groups - 1");
    if (in->n_measures < 1 || in->n_measures > STA_MAX_MEASURES) return bad("n_measures must be 1 .. 64");
    if (!in->family || !in->column || !in->lo || !in->hi || !in->bins || !in->top_dir) return bad("a measure array is missing");
    for (int m = 0; m < in->n_measures; ++m) {
        const std::string who = "measure " + std::to_string(m) + ": ";
        const int fam = in->family[m];
        if (fam < 0 || fam >= fleet::STA_FAMILIES) return bad(who + "unknown family");
        if (in->column[m] < 0 || in->column[m] >= kStatsColumns[fam])
            return bad(who + "column outside the " + std::to_string(kStatsColumns[fam]) + " doubles of family " + kStatsFamily[fam]);
        if (fam != fleet::STA_FAM_STATE && !sim_stats_records(s, fam)) return bad(who + "family " + kStatsFamily[fam] + " is off");
        if (const char* why = sim_stats_spec_bad(in->lo[m], in->hi[m], (double)in->bins[m], (double)in->top_dir[m])) return bad(who + why);
    }
    if (in->top_k < 0 || in->top_k > fleet::kStatsTop) return bad("top_k must be 0 .. 8");
    if (in->period < 0) return bad("period must not be negative");
    if (in->period > 0 && in->depth < 1) return bad("depth must be positive with a period");
    if (in->tick0 < 0) return bad("tick0 must not be negative");
    if (in->flags & ~(uint32_t)LTPL_SIM_STATS_KEEP_SERIES) return bad("unknown flag");
    if (in->period > 0) {
        const size_t row = sizeof(double) * (size_t)in->n_groups * (size_t)in->n_measures * LTPL_FLEET_SIM_STATS_DOUBLES;
        if ((size_t)in->depth > STA_MAX_SERIES_BYTES / row) return bad("the series would take more than 256 MiB", LTPL_ERR_CAPACITY);
    }
    if ((in->flags & LTPL_SIM_STATS_KEEP_SERIES) && s.stats.on && s.sp.period > 0) {
        if (in->period < 1 || in->n_groups != s.stats.dev.G || in->n_measures != s.stats.dev.M || in->depth != s.sp.depth)
            return bad("LTPL_SIM_STATS_KEEP_SERIES: n_groups, n_measures and depth must be the plan's, with a period");
        *keep = true;
    }
    return LTPL_OK;
}

extern "C" int ltpl_fleet_sim_stats(ltpl_fleet* f, const ltpl_fleet_sim_stats_in* in)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    bool keep = false;
    int rc = sim_check_stats(f, in, &keep);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FleetSim& s = *f->sim;
    if (!in) {
        s.stats.clear(); sim_free_list(s.sp.ring_allocs);
        s.sp = FleetSim::StatsPlan{};
        return LTPL_OK;
    }
    const int N = f->D.N, G = in->n_groups, M = in->n_measures;
    std::vector<int> off((size_t)G + 1, 0), members;
    for (int p = 0; p < N; ++p) if (in->group[p] >= 0) ++off[(size_t)in->group[p] + 1];
    for (int g = 0; g < G; ++g) off[(size_t)g + 1] += off[(size_t)g];
    members.resize((size_t)off[(size_t)G]);
    {
        std::vector<int> at(off.begin(), off.end() - 1);
        for (int p = 0; p < N; ++p) if (in->group[p] >= 0) members[(size_t)at[(size_t)in->group[p]]++] = p;     // planners ascending inside a group
    }
    const StatsChunks ch = sim_stats_chunks(off.data(), G);
    const size_t nc = ch.group.size();
    std::vector<int> topk((size_t)M, in->top_k);
    std::vector<double> edges((size_t)M * (fleet::kStatsBins + 1), 0.0);
    for (int m = 0; m < M; ++m) fleet::stats_edges(in->lo[m], in->hi[m], in->bins[m], edges.data() + (size_t)m * (fleet::kStatsBins + 1));
    // everything new is allocated first; the fleet keeps its previous plan and series unless every step succeeds
    SimAllocs al, ring;
    SimStats st{};
    st.G = G; st.M = M; st.spec_stride = 0;
    int* pi = nullptr; double* pd = nullptr;
#define STA_UP(dst, src, n) do { if ((rc = sim_upload(f, al.p, src, (size_t)(n), &pi))) return rc; dst = pi; } while (0)
    STA_UP(st.members, members.data(), members.size());
    STA_UP(st.ch_group, ch.group.data(), nc); STA_UP(st.ch_first, ch.first.data(), nc); STA_UP(st.ch_cnt, ch.cnt.data(), nc);
    STA_UP(st.g_choff, ch.g_choff.data(), G + 1);
    STA_UP(st.ms_fam, in->family, M); STA_UP(st.ms_col, in->column, M); STA_UP(st.ms_bins, in->bins, M); STA_UP(st.ms_dir, in->top_dir, M);
    STA_UP(st.ms_topk, topk.data(), M);
#undef STA_UP
    if ((rc = sim_upload(f, al.p, edges.data(), edges.size(), &pd))) return rc;
    st.ms_edges = pd;
    double* d_rows = nullptr; double* d_tops = nullptr; double* d_ring = nullptr;
    if ((rc = sim_upload(f, al.p, (const double*)nullptr, nc * M * LTPL_FLEET_SIM_STATS_DOUBLES, &st.part_row))) return rc;
    if ((rc = sim_upload(f, al.p, (const double*)nullptr, nc * M * STA_TOP, &st.part_top))) return rc;
    if ((rc = sim_upload(f, al.p, (const double*)nullptr, (size_t)G * M * LTPL_FLEET_SIM_STATS_DOUBLES, &d_rows))) return rc;
    if ((rc = sim_upload(f, al.p, (const double*)nullptr, (size_t)G * M * STA_TOP, &d_tops))) return rc;
    if (in->period > 0 && !keep &&
        (rc = sim_upload(f, ring.p, (const double*)nullptr, (size_t)in->depth * G * M * LTPL_FLEET_SIM_STATS_DOUBLES, &d_ring))) return rc;
    s.stats.commit(al, st, in->tick0);
    FleetSim::StatsPlan& sp = s.sp;
    sp.n_chunks = (int)nc; sp.top_k = in->top_k; sp.period = in->period; sp.depth = in->period > 0 ? in->depth : 0;
    sp.fam.assign(in->family, in->family + M);
    sp.rows = d_rows; sp.tops = d_tops;
    if (!keep) {
        sim_free_list(sp.ring_allocs);
        sp.ring_allocs.swap(ring.p);
        sp.ring = d_ring; sp.n_rows = 0;
        sp.ring_tick.assign((size_t)sp.depth, 0);
    }
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_stats_reduce(ltpl_fleet* f, double* rows_out, int32_t doubles_per_row, double* top_out, int32_t top_k)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const std::string& why) { f->err = "fleet sim stats: " + why; return LTPL_ERR_INVALID_ARG; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    FleetSim& s = *f->sim;
    if (!s.stats.on) return bad("no plan (ltpl_fleet_sim_stats first)");
    if (!rows_out) return bad("rows_out missing");
    if (doubles_per_row != LTPL_FLEET_SIM_STATS_DOUBLES) return bad("row size mismatch");
    if (top_out && top_k != s.sp.top_k) return bad("top_k is not the plan's");
    SimStats st = s.stats.dev;
    int rc = sim_stats_sources(f, &st);
    if (rc) return rc;
    if ((rc = fleet_enter(f))) return rc;
    if ((rc = sim_stats_launch(f, st, s.sp.n_chunks, nullptr, s.sp.rows, s.sp.tops))) return rc;
    const size_t GM = (size_t)st.G * st.M;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    FLEET_TRY(f, hipMemcpy(rows_out, s.sp.rows, sizeof(double) * GM * LTPL_FLEET_SIM_STATS_DOUBLES, hipMemcpyDeviceToHost));
    if (top_out && top_k > 0) {
        std::vector<double> tops(GM * STA_TOP);
        FLEET_TRY(f, hipMemcpy(tops.data(), s.sp.tops, sizeof(double) * tops.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < GM; ++i) for (size_t k = 0; k < 2 * (size_t)top_k; ++k) top_out[i * 2 * (size_t)top_k + k] = tops[i * STA_TOP + k];
    }
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_stats_series(ltpl_fleet* f, int32_t* ticks_out, double* rows_out, int32_t doubles_per_row, int32_t* n_rows_out,
                                           int64_t* n_total_out)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const std::string& why) { f->err = "fleet sim stats: " + why; return LTPL_ERR_INVALID_ARG; };
    if (!f->sim) return bad("ltpl_fleet_sim_setup first");
    FleetSim& s = *f->sim;
    if (!s.stats.on || s.sp.period < 1) return bad("no series (ltpl_fleet_sim_stats with a period first)");
    if (rows_out && doubles_per_row != LTPL_FLEET_SIM_STATS_DOUBLES) return bad("row size mismatch");
    const size_t depth = (size_t)s.sp.depth, held = s.sp.n_rows < (long long)depth ? (size_t)s.sp.n_rows : depth;
    const size_t row = (size_t)s.stats.dev.G * s.stats.dev.M * LTPL_FLEET_SIM_STATS_DOUBLES;
    if (n_rows_out) *n_rows_out = (int32_t)held;
    if (n_total_out) *n_total_out = (int64_t)s.sp.n_rows;
    if (!rows_out && !ticks_out) return LTPL_OK;
    FLEET_TRY(f, hipSetDevice(f->h->device));
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    for (size_t k = 0; k < held; ++k) {                          // oldest first
        const size_t slot = (size_t)((s.sp.n_rows - (long long)held + (long long)k) % (long long)depth);
        if (ticks_out) ticks_out[k] = s.sp.ring_tick[slot];
        if (rows_out) FLEET_TRY(f, hipMemcpy(rows_out + k * row, s.sp.ring + slot * row, sizeof(double) * row, hipMemcpyDeviceToHost));
    }
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_stats_eval(ltpl_fleet* f, int32_t n_cases, const int32_t* val_off, const double* values, const int32_t* planner_idx,
                                         const double* spec, double* rows_out, double* top_out)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    auto bad = [&](const std::string& why) { f->err = "fleet sim stats eval: " + why; return LTPL_ERR_INVALID_ARG; };
    if (n_cases < 0) return bad("n_cases must not be negative");
    if (n_cases == 0) return LTPL_OK;
    if (n_cases > STA_MAX_GROUPS) return bad("at most 4096 cases");
    if (!val_off || !spec || !rows_out || !top_out) return bad("an array is missing");
    if (val_off[0] != 0) return bad("value offsets must start at 0");
    const size_t m = (size_t)n_cases;
    for (size_t q = 0; q < m; ++q) {
        const std::string who = "case " + std::to_string(q) + ": ";
        if (val_off[q + 1] < val_off[q]) return bad(who + "value offsets must not decrease");
        const double* sq = spec + 5 * q;
        if (const char* why = sim_stats_spec_bad(sq[0], sq[1], sq[2], sq[3])) return bad(who + why);
        if (!(sq[4] >= 0.0 && sq[4] <= (double)fleet::kStatsTop) || sq[4] != std::floor(sq[4])) return bad(who + "top_k must be 0 .. 8");
    }
    const size_t nv = (size_t)val_off[m];
    if (nv > 0 && !values) return bad("values missing");
    if (planner_idx) for (size_t i = 0; i < nv; ++i) if (planner_idx[i] < 0 || planner_idx[i] == fleet::kStatsNoPlanner) return bad("a planner index must be 0 .. 2^31 - 2");
    const StatsChunks ch = sim_stats_chunks(val_off, n_cases);
    const size_t nc = ch.group.size();
    std::vector<int> members(nv), zero(m, 0), bins(m), dir(m), topk(m);
    std::vector<double> edges(m * (fleet::kStatsBins + 1), 0.0);
    for (size_t q = 0; q < m; ++q) {
        for (int i = val_off[q]; i < val_off[q + 1]; ++i) members[(size_t)i] = planner_idx ? planner_idx[i] : i - val_off[q];
        const double* sq = spec + 5 * q;
        bins[q] = (int)sq[2]; dir[q] = (int)sq[3]; topk[q] = (int)sq[4];
        fleet::stats_edges(sq[0], sq[1], bins[q], edges.data() + q * (fleet::kStatsBins + 1));
    }
    int rc = fleet_enter(f);
    if (rc) return rc;
    SimHookBlock b(f);
    const auto d_val = b.in(values, nv); const auto d_mem = b.in(members.data(), nv);
    const auto d_cg = b.in(ch.group.data(), nc); const auto d_cf = b.in(ch.first.data(), nc); const auto d_cc = b.in(ch.cnt.data(), nc);
    const auto d_go = b.in(ch.g_choff.data(), m + 1);
    const auto d_fam = b.in(zero.data(), m); const auto d_bins = b.in(bins.data(), m); const auto d_dir = b.in(dir.data(), m); const auto d_topk = b.in(topk.data(), m);
    const auto d_edges = b.in(edges.data(), edges.size());
    const auto d_pr = b.out<double>(nc * LTPL_FLEET_SIM_STATS_DOUBLES); const auto d_pt = b.out<double>(nc * STA_TOP);
    const auto d_rows = b.out<double>(m * LTPL_FLEET_SIM_STATS_DOUBLES); const auto d_tops = b.out<double>(m * STA_TOP);
    if ((rc = b.upload())) return rc;
    SimStats st{};
    st.G = n_cases; st.M = 1; st.spec_stride = 1;
    st.ch_group = d_cg; st.ch_first = d_cf; st.ch_cnt = d_cc; st.g_choff = d_go; st.members = d_mem;
    st.ms_fam = d_fam; st.ms_col = d_fam; st.ms_bins = d_bins; st.ms_dir = d_dir; st.ms_topk = d_topk; st.ms_edges = d_edges;
    st.part_row = d_pr; st.part_top = d_pt;
    if ((rc = sim_stats_launch(f, st, (int)nc, d_val, d_rows, d_tops))) return rc;
    if ((rc = b.fetch(rows_out, d_rows, m * LTPL_FLEET_SIM_STATS_DOUBLES))) return rc;
    if ((rc = b.fetch(top_out, d_tops, m * STA_TOP))) return rc;
    return b.finish();
} LTPL_ABI_CATCH(abi_err_of(f))
