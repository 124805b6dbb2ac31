// fleet_branch.hpp -- included at the end of ltpl_hip.hip, behind fleet_sim.hpp. SNAPSHOT AND BRANCH of the fleet simulation's planner
// state on the device (ltpl_fleet_sim_snapshot / _snapshot_info / _snapshot_drop / _branch, include/ltpl_hip.h, additive to ABI v9).
// The rule: what the tick kernels WRITE travels with a planner's state, what the caller SET stays with the destination --
//   copied   the planner block (Dims::stride bytes of d_state; the planner's error word PlannerS::err lies in it), its window of friction
//            rows (Dims::gg_stride bytes of d_gg) when both sides have windows, now / sel / started / pos_x / pos_y / vel / theta / live,
//            opp_s / opp_tic of its opponents, and the six parts of the table below: what the models' tick kernels write;
//   stays    the race line, the opponents' vel_scale / length, statics, zones, preference list, dt, n_export, the velocity arguments,
//            friction map index and scale, race membership and length as a mate, contact radius, the recorder's ring and indices,
//            the vehicle model's switch and parameters, the tracker's parameters and statistics, the selector's parameters, ordered
//            lists and statistics, the safety monitor's parameters, mask and tick index, the reactive opponents' parameters and tick index.
// The parts. A source HOLDS a part as a live planner while the model is set, and as a snapshot entry taken while it was set:
//   part         copied by                   the destination takes it where        a source without it leaves             the pair is refused where
//   telemetry    bulk kernel, wave 0         telemetry is on and the source's      the destination's record, grid_s and   never
//   (record, grid_s, prog)                   is of the same ltpl_fleet_sim_        prog as they are
//                                            telemetry call (FleetSim::tele_gen)
//   vehicle      bulk kernel, wave 0         the destination drives model 1 (one   -- (refused)                           the destination drives model 1 and the
//   (record: state and statistics)           on the ideal tracker keeps its NaN                                           source drove model 0, or none, when
//                                            record, whatever the source drives)                                          it was copied
//   tracker      bulk kernel, wave 0         the fleet has a tracker               an empty table and next_id 0, the      the source holds more tracks than
//   (table, track count, next_id)                                                  tracker's start state                  the destination's table (C_p)
//   staged list  k_fleet_sim_branch_staged   the fleet has a selector, which       an empty list (cnt 0): the next tick   never (a longer list is cut to the
//   (cnt, cnt entries of g_x .. g_r)         reads the list at the next tick's     scores without objects                 destination's staging slots)
//                                            head
//   safety       k_fleet_sim_branch_safety   the fleet has a monitor               fleet::safety_start (prev_valid 0:     never
//   (record, incident ring)                                                        its next live tick is not evaluated)
//   react        k_fleet_sim_branch_react    the fleet has a model                 fleet::react_start and eff = its own   never
//   (record, effective scales)                                                     configured scales
// Everything else the simulation holds per planner (prev_action, t_now, veh_off, g_v and the noise's true positions in the staging, the
// tick's object arrays, the job pools of the velocity stage -- and cnt and the staging slots without a selector) is written by every tick
// before it is read.
// One kernel serves the three directions live -> snapshot, snapshot -> live and live -> live: it copies between two VIEWS, each a set of
// base pointers indexed by an entry per pair. The live fleet is the view whose entries are planner indices; a snapshot is the same set of
// arrays allocated per slot, with its planners packed (entry k = the k-th planner of the list) and an opponent offset table of its own.
#pragma once

struct BranchView {
    unsigned char* state; unsigned char* gg;            // [entries][stride], [entries][gg_stride] (gg null: no row windows)
    double* now; int* sel; int* started; double* pos_x; double* pos_y; double* vel; double* theta; int* live;
    const int* opp_off; double* opp_s; double* opp_tic; // opponents of entry e: opp_off[e] .. opp_off[e + 1] - 1
    double* rec; double* grid_s; double* prog;          // telemetry part (rec null: none)
    double* veh; const int* veh_model;                  // vehicle records (veh null: none); as a destination: the model of every entry
    double* trk; int* trk_n; double* trk_next; const int* trk_base;   // tracker: rows of entry e from row trk_base[e] on (trk_n null: none)
};

// the staged object list (behaviour selector only): cnt[e] entries of the five arrays from base[e] on; base[e + 1] - base[e] slots
struct StagedView { int* cnt; double* g[5]; const int* base; };

// behind k_fleet_sim_branch, only where the destination has a selector: one wave64 per pair. S.cnt null: the source holds no list
__global__ __launch_bounds__(64) void k_fleet_sim_branch_staged(StagedView S, StagedView T, const int* __restrict__ src_entry,
                                                                const int* __restrict__ dst_entry)
{
    const int k = blockIdx.x, t = threadIdx.x;
    const int es = src_entry[k], ed = dst_entry[k];
    const int cap = T.base[ed + 1] - T.base[ed];
    int n = S.cnt ? S.cnt[es] : 0;
    if (n > cap) n = cap;
    if (n < 0) n = 0;
    if (S.cnt) {
        const int a = S.base[es], b = T.base[ed];
        if (n > S.base[es + 1] - a) n = S.base[es + 1] - a;
#pragma unroll
        for (int c = 0; c < 5; ++c)
            for (int q = t; q < n; q += 64) T.g[c][b + q] = S.g[c][a + q];
    }
    if (t == 0) T.cnt[ed] = n;
}

// the safety monitor's record and ring of entry e (rec null: the source holds none)
struct SafetyView { double* rec; double* inc; };

// behind k_fleet_sim_branch, only where the live fleet has a monitor: one wave64 per pair
__global__ __launch_bounds__(64) void k_fleet_sim_branch_safety(SafetyView S, SafetyView T, const int* __restrict__ src_entry,
                                                                const int* __restrict__ dst_entry)
{
    const int k = blockIdx.x, t = threadIdx.x;
    const size_t es = (size_t)src_entry[k], ed = (size_t)dst_entry[k];
    double* r = T.rec + ed * LTPL_FLEET_SIM_SAFETY_DOUBLES; double* e = T.inc + ed * SAF_RING;
    if (S.rec) {
        if (t < LTPL_FLEET_SIM_SAFETY_DOUBLES) r[t] = S.rec[es * LTPL_FLEET_SIM_SAFETY_DOUBLES + t];
        if (t < SAF_RING) e[t] = S.inc[es * SAF_RING + t];
    } else if (t == 0) fleet::safety_start(r, e);
}
static_assert(LTPL_FLEET_SIM_SAFETY_DOUBLES <= 64 && SAF_RING <= 64, "k_fleet_sim_branch_safety: one lane per double");

// the reactive opponents' effective scales and record of entry e (rec null: the source holds none); eff of entry e from opp_off[e] on
struct ReactView { double* eff; double* rec; const int* opp_off; };

// behind k_fleet_sim_branch, only where the live fleet has a model: one wave64 per pair. `own`: the destination view's configured scales
// (same offsets as T.eff), what a destination starts from whose source holds no state
__global__ __launch_bounds__(64) void k_fleet_sim_branch_react(ReactView S, ReactView T, const double* __restrict__ own,
                                                               const int* __restrict__ src_entry, const int* __restrict__ dst_entry)
{
    const int k = blockIdx.x, t = threadIdx.x;
    const int es = src_entry[k], ed = dst_entry[k];
    const int to = T.opp_off[ed], no = T.opp_off[ed + 1] - to;       // (equal counts on both sides: the host's check)
    double* r = T.rec + (size_t)ed * LTPL_FLEET_SIM_REACT_DOUBLES;
    if (S.rec) {
        const int so = S.opp_off[es];
        if (t < LTPL_FLEET_SIM_REACT_DOUBLES) r[t] = S.rec[(size_t)es * LTPL_FLEET_SIM_REACT_DOUBLES + t];
        for (int q = t; q < no; q += 64) T.eff[to + q] = S.eff[so + q];
    } else {
        if (t == 0) fleet::react_start(r);
        for (int q = t; q < no; q += 64) T.eff[to + q] = own[to + q];
    }
}
static_assert(LTPL_FLEET_SIM_REACT_DOUBLES <= 64, "k_fleet_sim_branch_react: one lane per double");

typedef unsigned int branch_u32x4 __attribute__((ext_vector_type(4)));
#define BRANCH_THREADS 256
#define BRANCH_LOADS 4                                    // 16-byte loads a lane issues before its first store
#define BRANCH_CHUNK ((size_t)BRANCH_THREADS * 16 * BRANCH_LOADS)

// grid (chunks of a planner image, pairs): chunk c < state_chunks covers bytes [c, c + 1) BRANCH_CHUNK of the planner block, the chunks
// behind them the same of the row window. Both sizes are multiples of 256 bytes and both bases are 256-byte aligned (hipMalloc; strides),
// so every 16-byte access is aligned and a group of 16 lanes is inside or outside as a whole: one predicate per load, no tail code.
// Pairs beyond the grid's y extent are walked by the same workgroups. Wave 0 of chunk 0 copies the small parts: lane 0 the scalars, one
// lane per opponent (any count, 0 included) and per double of the telemetry record. dst entries are distinct and, within one view, no
// entry is read and written (checked by the host): plain loads and stores, no ordering between workgroups.
template <bool NT>
__global__ __launch_bounds__(BRANCH_THREADS) void k_fleet_sim_branch(BranchView S, BranchView T, const int* __restrict__ src_entry,
                                                                     const int* __restrict__ dst_entry, int n_pairs, size_t stride,
                                                                     size_t gg_stride, int state_chunks)
{
    const int c = blockIdx.x, t = threadIdx.x;
    for (int k = blockIdx.y; k < n_pairs; k += gridDim.y) {
        const size_t es = (size_t)src_entry[k], ed = (size_t)dst_entry[k];
        const bool rows = c >= state_chunks;
        const size_t bytes = rows ? gg_stride : stride;
        const unsigned char* a = rows ? S.gg + gg_stride * es : S.state + stride * es;
        unsigned char* b = rows ? T.gg + gg_stride * ed : T.state + stride * ed;
        const size_t o0 = (size_t)(rows ? c - state_chunks : c) * BRANCH_CHUNK + (size_t)t * 16;
        branch_u32x4 v[BRANCH_LOADS];
#pragma unroll
        for (int i = 0; i < BRANCH_LOADS; ++i) {
            const size_t o = o0 + (size_t)i * BRANCH_THREADS * 16;
            if (o < bytes) v[i] = *reinterpret_cast<const branch_u32x4*>(a + o);
        }
#pragma unroll
        for (int i = 0; i < BRANCH_LOADS; ++i) {
            const size_t o = o0 + (size_t)i * BRANCH_THREADS * 16;
            if (o < bytes) {
                if constexpr (NT) __builtin_nontemporal_store(v[i], reinterpret_cast<branch_u32x4*>(b + o));
                else *reinterpret_cast<branch_u32x4*>(b + o) = v[i];
            }
        }
        if (c != 0 || t >= 64) continue;
        if (t == 0) {
            T.now[ed] = S.now[es]; T.sel[ed] = S.sel[es]; T.started[ed] = S.started[es]; T.pos_x[ed] = S.pos_x[es]; T.pos_y[ed] = S.pos_y[es];
            T.vel[ed] = S.vel[es]; T.theta[ed] = S.theta[es]; T.live[ed] = S.live[es];
        }
        const int so = S.opp_off[es], no = S.opp_off[es + 1] - so, to = T.opp_off[ed];       // (equal counts on both sides: the host's check)
        for (int q = t; q < no; q += 64) { T.opp_s[to + q] = S.opp_s[so + q]; T.opp_tic[to + q] = S.opp_tic[so + q]; }
        if (S.rec && T.rec) {
            if (t < LTPL_FLEET_SIM_TELE_DOUBLES) T.rec[ed * LTPL_FLEET_SIM_TELE_DOUBLES + t] = S.rec[es * LTPL_FLEET_SIM_TELE_DOUBLES + t];
            else if (t == LTPL_FLEET_SIM_TELE_DOUBLES) T.grid_s[ed] = S.grid_s[es];
            else if (t == LTPL_FLEET_SIM_TELE_DOUBLES + 1) T.prog[ed] = S.prog[es];
        }
        if (S.veh && T.veh && t < LTPL_FLEET_SIM_VEH_DOUBLES && T.veh_model[ed] != 0)
            T.veh[ed * LTPL_FLEET_SIM_VEH_DOUBLES + t] = S.veh[es * LTPL_FLEET_SIM_VEH_DOUBLES + t];
        if (T.trk_n) {
            const int nt = S.trk_n ? S.trk_n[es] : 0;       // (at most the destination's capacity: the host's check)
            if (S.trk_n) {
                const double* a_ = S.trk + (size_t)S.trk_base[es] * LTPL_FLEET_SIM_TRACK_DOUBLES;
                double* b_ = T.trk + (size_t)T.trk_base[ed] * LTPL_FLEET_SIM_TRACK_DOUBLES;
                for (int q = t; q < nt * LTPL_FLEET_SIM_TRACK_DOUBLES; q += 64) b_[q] = a_[q];
            }
            if (t == 0) { T.trk_n[ed] = nt; T.trk_next[ed] = S.trk_n ? S.trk_next[es] : 0.0; }
        }
    }
}
static_assert(LTPL_FLEET_SIM_TELE_DOUBLES + 2 <= 64, "k_fleet_sim_branch: one lane per telemetry double");

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// one side of a copy: the live fleet, or a snapshot's slot. A part the side does not hold is a null view (the table at the top)
struct BranchSide {
    BranchView v;
    StagedView stg;                         // stg.cnt null: no selector
    SafetyView saf;                         // saf.rec null: no monitor
    ReactView rct;                          // rct.rec null: no reactive model
    const double* own;                      // the live fleet's configured scales on rct's offsets: k_fleet_sim_branch_react's `own`
};

struct SimSnap {
    std::vector<void*> allocs;
    BranchSide side{};
    std::vector<int> planners;              // entry k holds planner planners[k]
    std::vector<int> entry_of;              // [N] entry of planner p, -1: not in the snapshot
    std::vector<int> opp_off;               // [entries + 1] host copy of side.v.opp_off
    int tele_gen = 0;                       // a telemetry part was taken from the telemetry numbered tele_gen (FleetSim::tele_gen)
    std::vector<int> veh_model;             // [entries] the model of entry k when the snapshot was taken (empty: the model was off)
    uint64_t bytes = 0;
    bool held() const { return !planners.empty(); }
};
struct SimSnaps { SimSnap slot[LTPL_FLEET_SIM_SNAPSHOTS]; };
static void sim_snaps_free(SimSnaps* s)
{
    if (!s) return;
    for (SimSnap& q : s->slot) sim_free_list(q.allocs);
    delete s;
}

// the live fleet as a side: its entries are planner indices, its parts those of the models that are set
static BranchSide branch_live_side(const ltpl_fleet* f)
{
    const FleetSim& s = *f->sim; const SimDev& d = s.sd;
    BranchSide L{};
    BranchView& v = L.v;
    v.state = f->d_state; v.gg = f->d_gg;
    v.now = d.now; v.sel = d.sel; v.started = d.started; v.pos_x = d.pos_x; v.pos_y = d.pos_y; v.vel = d.vel; v.theta = d.theta; v.live = d.live;
    v.opp_off = d.opp_off; v.opp_s = d.opp_s; v.opp_tic = d.opp_tic;
    if (s.tele.on) { v.rec = s.tele.dev.rec; v.grid_s = s.tele.dev.grid_s; v.prog = s.tele.dev.prog; }
    if (s.veh.on) { v.veh = s.veh.dev.rec; v.veh_model = s.veh.dev.model; }
    if (s.trk.on) { v.trk = s.trk.dev.rows; v.trk_n = s.trk.dev.n; v.trk_next = s.trk.dev.next_id; v.trk_base = s.trk.dev.base; }
    if (s.sel.on) L.stg = StagedView{d.cnt, {d.g_x, d.g_y, d.g_px, d.g_py, d.g_r}, d.obj_base};
    if (s.saf.on) L.saf = SafetyView{s.saf.dev.rec, s.saf.dev.inc};
    if (s.react.on) { L.rct = ReactView{s.react.dev.eff, s.react.dev.rec, d.opp_off}; L.own = d.opp_scale; }
    return L;
}

// The device work of a snapshot and of a branch. The pairs' entries go to the device in the call's one allocation ([src | dst]), in front
// of the first launch: a failing allocation changes nothing. Then the launches back to back on the handle's stream and one
// synchronisation. A part kernel is launched only where the destination side T holds the part; a source side without it is the null
// view its kernel knows. `ms`: device time of the bulk kernel alone
static int branch_copy(ltpl_fleet* f, BranchSide S, BranchSide T, const std::vector<int>& src_entry, const std::vector<int>& dst_entry, float* ms)
{
    const int n = (int)src_entry.size();
    if (ms) *ms = 0.0f;
    if (n == 0) return LTPL_OK;
    if (!S.v.rec || !T.v.rec) S.v.rec = T.v.rec = nullptr;
    const bool rows = S.v.gg && T.v.gg;
    const size_t stride = f->D.stride, gg_stride = f->D.gg_stride;
    const int state_chunks = (int)((stride + BRANCH_CHUNK - 1) / BRANCH_CHUNK), gg_chunks = rows ? (int)((gg_stride + BRANCH_CHUNK - 1) / BRANCH_CHUNK) : 0;
    SimAllocs a;
    int* d_idx = nullptr;
    std::vector<int> idx(src_entry);
    idx.insert(idx.end(), dst_entry.begin(), dst_entry.end());
    int rc = sim_upload(f, a.p, idx.data(), idx.size(), &d_idx);
    if (rc) return rc;
    const int* d_src = d_idx; const int* d_dst = d_idx + n;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct Guard { hipEvent_t* a; hipEvent_t* b; ~Guard() { if (*a) (void)hipEventDestroy(*a); if (*b) (void)hipEventDestroy(*b); } } g{&e0, &e1};
    FLEET_TRY(f, hipEventCreate(&e0)); FLEET_TRY(f, hipEventCreate(&e1));
    hipStream_t st = f->h->stream;
    const dim3 grid((unsigned)(state_chunks + gg_chunks), (unsigned)(n < 65535 ? n : 65535));
    FLEET_TRY(f, hipEventRecord(e0, st));
#ifdef LTPL_EXPERIMENT
    if (getenv("LTPL_SIM_BRANCH_NT") && atoi(getenv("LTPL_SIM_BRANCH_NT")) != 0)        // (the store form: DESIGN 4.5c, measured with tools/sim_branch_rate.py)
        hipLaunchKernelGGL(k_fleet_sim_branch<true>, grid, dim3(BRANCH_THREADS), 0, st, S.v, T.v, d_src, d_dst, n, stride, gg_stride, state_chunks);
    else
#endif
    hipLaunchKernelGGL(k_fleet_sim_branch<false>, grid, dim3(BRANCH_THREADS), 0, st, S.v, T.v, d_src, d_dst, n, stride, gg_stride, state_chunks);
    FLEET_TRY(f, hipGetLastError());
    FLEET_TRY(f, hipEventRecord(e1, st));
    auto part = [&](auto kernel, auto... views) { hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(64), 0, st, views..., d_src, d_dst); };     // one wave64 per pair
    if (T.stg.cnt) { part(k_fleet_sim_branch_staged, S.stg, T.stg); FLEET_TRY(f, hipGetLastError()); }
    if (T.saf.rec) { part(k_fleet_sim_branch_safety, S.saf, T.saf); FLEET_TRY(f, hipGetLastError()); }
    if (T.rct.rec) { part(k_fleet_sim_branch_react, S.rct, T.rct, T.own); FLEET_TRY(f, hipGetLastError()); }
    FLEET_TRY(f, hipStreamSynchronize(st));
    if (ms) FLEET_TRY(f, hipEventElapsedTime(ms, e0, e1));
    return LTPL_OK;
}

static int branch_bad(ltpl_fleet* f, const std::string& why, const char* what = "snapshot") { f->err = std::string("fleet sim ") + what + ": " + why; return LTPL_ERR_INVALID_ARG; }
// the checks every one of the four calls starts with (before the first HIP call); slot -1: the live fleet, where `live_ok`
static int branch_check_slot(ltpl_fleet* f, int32_t slot, bool live_ok)
{
    const char* what = live_ok ? "branch" : "snapshot";
    if (!f->sim) return branch_bad(f, "ltpl_fleet_sim_setup first", what);
    if (slot < (live_ok ? -1 : 0) || slot >= LTPL_FLEET_SIM_SNAPSHOTS)
        return branch_bad(f, "slot " + std::to_string(slot) + " out of range (" + (live_ok ? "-1: the live fleet, " : "") + "0 .. " + std::to_string(LTPL_FLEET_SIM_SNAPSHOTS - 1) + ")", what);
    return LTPL_OK;
}

extern "C" int ltpl_fleet_sim_snapshot(ltpl_fleet* f, int32_t slot, const int32_t* planners, int32_t n_planners)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    int rc = branch_check_slot(f, slot, false);
    if (rc) return rc;
    FleetSim& s = *f->sim;
    const int N = f->D.N;
    std::unique_ptr<SimSnap> q(new SimSnap());
    q->entry_of.assign((size_t)N, -1);
    if (!planners) {
        q->planners.resize((size_t)N);
        for (int p = 0; p < N; ++p) q->planners[(size_t)p] = q->entry_of[(size_t)p] = p;
    } else {
        if (n_planners < 1 || n_planners > N) return branch_bad(f, "a planner list needs 1 .. n entries");
        for (int k = 0; k < n_planners; ++k) {
            const int p = planners[k];
            if (p < 0 || p >= N) return branch_bad(f, "planner index " + std::to_string(p) + " out of range");
            if (q->entry_of[(size_t)p] >= 0) return branch_bad(f, "planner " + std::to_string(p) + " is given twice");
            q->entry_of[(size_t)p] = k;
        }
        q->planners.assign(planners, planners + n_planners);
    }
    const size_t M = q->planners.size();
    q->opp_off.assign(M + 1, 0);
    for (size_t k = 0; k < M; ++k) { const size_t p = (size_t)q->planners[k]; q->opp_off[k + 1] = q->opp_off[k] + (s.opp_off[p + 1] - s.opp_off[p]); }
    const size_t n_opp = (size_t)q->opp_off[M];
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    // everything new is allocated first; the slot keeps its previous snapshot unless every step succeeds
    SimAllocs a;
    BranchView& v = q->side.v;
    uint64_t bytes = 0;
    auto take = [&](auto*& out, size_t n, const int* init = nullptr) {
        using T = std::remove_const_t<std::remove_pointer_t<std::remove_reference_t<decltype(out)>>>;
        void* p = nullptr;
        const size_t b = (n ? n : 1) * sizeof(T);
        if (hipMalloc(&p, b) != hipSuccess) { f->err = "fleet sim snapshot: hipMalloc of " + std::to_string(b) + " bytes failed"; return (int)LTPL_ERR_HIP; }
        a.p.push_back(p); bytes += b;
        if (init && hipMemcpy(p, init, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { f->err = "fleet sim snapshot: upload failed"; return (int)LTPL_ERR_HIP; }
        out = static_cast<T*>(p);
        return (int)LTPL_OK;
    };
#define SNAP_TAKE(...) do { if ((rc = take(__VA_ARGS__))) return rc; } while (0)
    SNAP_TAKE(v.state, f->D.stride * M);
    if (f->d_gg) SNAP_TAKE(v.gg, f->D.gg_stride * M);
    SNAP_TAKE(v.now, M); SNAP_TAKE(v.sel, M); SNAP_TAKE(v.started, M); SNAP_TAKE(v.pos_x, M); SNAP_TAKE(v.pos_y, M); SNAP_TAKE(v.vel, M);
    SNAP_TAKE(v.theta, M); SNAP_TAKE(v.live, M);
    SNAP_TAKE(v.opp_off, M + 1, q->opp_off.data());
    SNAP_TAKE(v.opp_s, n_opp); SNAP_TAKE(v.opp_tic, n_opp);
    if (s.tele.on) { SNAP_TAKE(v.rec, M * LTPL_FLEET_SIM_TELE_DOUBLES); SNAP_TAKE(v.grid_s, M); SNAP_TAKE(v.prog, M); }
    if (s.veh.on) {                                     // (the snapshot's entries carry the source's model: its records are copied as they are)
        q->veh_model.resize(M);
        for (size_t k = 0; k < M; ++k) q->veh_model[k] = s.veh_model[(size_t)q->planners[k]];
        SNAP_TAKE(v.veh, M * LTPL_FLEET_SIM_VEH_DOUBLES);
        SNAP_TAKE(v.veh_model, M, q->veh_model.data());
    }
    if (s.trk.on) {                                     // (with the tracker off the snapshot holds what it held before)
        std::vector<int> tb(M + 1, 0);
        for (size_t k = 0; k < M; ++k) tb[k + 1] = tb[k] + s.trk_cap[(size_t)q->planners[k]];
        SNAP_TAKE(v.trk, (size_t)tb[M] * LTPL_FLEET_SIM_TRACK_DOUBLES); SNAP_TAKE(v.trk_n, M); SNAP_TAKE(v.trk_next, M);
        SNAP_TAKE(v.trk_base, M + 1, tb.data());
    }
    StagedView& sv = q->side.stg;
    if (s.sel.on) {                                     // (a list is state only for a selector; slots as the planners have them now)
        std::vector<int> sb(M + 1, 0);
        for (size_t k = 0; k < M; ++k) sb[k + 1] = sb[k] + s.slots[(size_t)q->planners[k]];
        SNAP_TAKE(sv.cnt, M);
        for (double*& g : sv.g) SNAP_TAKE(g, (size_t)sb[M]);
        SNAP_TAKE(sv.base, M + 1, sb.data());
    }
    SafetyView& fv = q->side.saf;
    if (s.saf.on) { SNAP_TAKE(fv.rec, M * LTPL_FLEET_SIM_SAFETY_DOUBLES); SNAP_TAKE(fv.inc, M * SAF_RING); }
    ReactView& rv = q->side.rct;
    if (s.react.on) { SNAP_TAKE(rv.rec, M * LTPL_FLEET_SIM_REACT_DOUBLES); SNAP_TAKE(rv.eff, n_opp); rv.opp_off = v.opp_off; }
#undef SNAP_TAKE
    std::vector<int> dst(M);
    for (size_t k = 0; k < M; ++k) dst[k] = (int)k;
    BranchSide live = branch_live_side(f);
    if (!s.staged_valid) live.stg = StagedView{};       // (a staging that holds no list is a source without one)
    if ((rc = branch_copy(f, live, q->side, q->planners, dst, nullptr))) return rc;
    q->allocs.swap(a.p);
    q->tele_gen = s.tele_gen; q->bytes = bytes;
    if (!s.snaps) s.snaps = new SimSnaps();
    SimSnap& old = s.snaps->slot[slot];
    sim_free_list(old.allocs);
    old = std::move(*q);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_snapshot_info(ltpl_fleet* f, int32_t slot, int32_t* n_planners, int32_t* planners, int32_t cap, uint64_t* bytes)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    int rc = branch_check_slot(f, slot, false);
    if (rc) return rc;
    const SimSnaps* sn = f->sim->snaps;
    const SimSnap* q = sn && sn->slot[slot].held() ? &sn->slot[slot] : nullptr;
    const int n = q ? (int)q->planners.size() : 0;
    if (planners && cap < n) return branch_bad(f, "the planner buffer holds " + std::to_string(cap) + " of " + std::to_string(n) + " entries");
    if (n_planners) *n_planners = n;
    if (planners && n) std::memcpy(planners, q->planners.data(), sizeof(int32_t) * (size_t)n);
    if (bytes) *bytes = q ? q->bytes : 0;
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_snapshot_drop(ltpl_fleet* f, int32_t slot)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    int rc = branch_check_slot(f, slot, false);
    if (rc) return rc;
    SimSnaps* sn = f->sim->snaps;
    if (!sn || !sn->slot[slot].held()) return LTPL_OK;
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    sim_free_list(sn->slot[slot].allocs);
    sn->slot[slot] = SimSnap();
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_branch(ltpl_fleet* f, int32_t slot, const int32_t* src, const int32_t* dst, int32_t n_pairs, float* ms)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    if (ms) *ms = 0.0f;
    int rc = branch_check_slot(f, slot, true);
    if (rc) return rc;
    FleetSim& s = *f->sim;
    const int N = f->D.N;
    const SimSnap* q = nullptr;
    auto bad = [&](const std::string& why) { return branch_bad(f, why, "branch"); };
    if (slot >= 0) {
        q = s.snaps && s.snaps->slot[slot].held() ? &s.snaps->slot[slot] : nullptr;
        if (!q) return bad("slot " + std::to_string(slot) + " is empty");
    }
    if (n_pairs < 0) return bad("n_pairs must not be negative");
    if (n_pairs == 0) return LTPL_OK;                        // nothing to copy: no allocation, no launch
    if (!src || !dst) return bad("src / dst missing");
    auto pair = [&](int k) { return "pair " + std::to_string(k) + " (src " + std::to_string(src[k]) + ", dst " + std::to_string(dst[k]) + "): "; };
    std::vector<char> is_dst((size_t)N, 0);
    for (int k = 0; k < n_pairs; ++k) {
        if (src[k] < 0 || src[k] >= N || dst[k] < 0 || dst[k] >= N) return bad(pair(k) + "planner index out of range");
        if (is_dst[(size_t)dst[k]]) return bad(pair(k) + "the destination is given twice");
        is_dst[(size_t)dst[k]] = 1;
    }
    std::vector<int> se, de;
    se.reserve((size_t)n_pairs); de.reserve((size_t)n_pairs);
    for (int k = 0; k < n_pairs; ++k) {
        const int a = src[k], b = dst[k];
        int no_src;
        if (q) {
            const int e = q->entry_of[(size_t)a];
            if (e < 0) return bad(pair(k) + "the source is not a planner of snapshot " + std::to_string(slot));
            no_src = q->opp_off[(size_t)e + 1] - q->opp_off[(size_t)e];
            se.push_back(e);
        } else {
            if (a == b) continue;                            // a planner onto itself: nothing to do
            if (is_dst[(size_t)a]) return bad(pair(k) + "with the live fleet as source no planner may be both a source and a destination");
            no_src = s.opp_off[(size_t)a + 1] - s.opp_off[(size_t)a];
            se.push_back(a);
        }
        const int no_dst = s.opp_off[(size_t)b + 1] - s.opp_off[(size_t)b];
        if (no_src != no_dst) return bad(pair(k) + "the source has " + std::to_string(no_src) + " opponents, the destination " + std::to_string(no_dst));
        if (s.veh.on && s.veh_model[(size_t)b] != 0) {      // (a destination on the ideal tracker takes no vehicle record)
            const bool src_has = q ? !q->veh_model.empty() && q->veh_model[(size_t)se.back()] != 0 : s.veh_model[(size_t)a] != 0;
            if (!src_has) return bad(pair(k) + "the destination drives the vehicle model, the source has no vehicle state (model 0 when it was copied)");
        }
        de.push_back(b);
    }
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    BranchSide S = q ? q->side : branch_live_side(f);
    if (s.trk.on && S.v.trk_n && !se.empty()) {              // the sources' track counts against the destinations' capacities
        const size_t ns = q ? q->planners.size() : (size_t)N;
        std::vector<int> nt(ns);
        FLEET_TRY(f, hipMemcpy(nt.data(), S.v.trk_n, sizeof(int) * ns, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < se.size(); ++k)
            if (nt[(size_t)se[k]] > s.trk_cap[(size_t)de[k]])
                return bad("the source of destination " + std::to_string(de[k]) + " holds " + std::to_string(nt[(size_t)se[k]]) + " tracks, the destination's table " +
                           std::to_string(s.trk_cap[(size_t)de[k]]));
    }
    if (q && q->tele_gen != s.tele_gen) S.v.rec = nullptr;      // (a telemetry set since then started its records anew)
    // no list yet, or a fresh staging: every planner gets the empty list a run would start from, the destinations' are then written over
    // it. (No change a caller can see, should the copy fail: nothing reads cnt while the flag is down, and a run sets both the same way.)
    if (s.sel.on && !s.staged_valid) {
        FLEET_TRY(f, hipMemset(s.sd.cnt, 0, sizeof(int) * (size_t)N));
        s.staged_valid = true;
    }
    if ((rc = branch_copy(f, S, branch_live_side(f), se, de, ms))) return rc;
    f->cur.has_paths = false;           // (as after a run: a per-call calc_vel_profile needs its own calc_paths first)
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))
