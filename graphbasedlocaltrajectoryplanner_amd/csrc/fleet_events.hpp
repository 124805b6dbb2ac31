// fleet_events.hpp -- included at the end of ltpl_hip.hip, behind fleet_branch.hpp. SCRIPTED EVENTS of the fleet simulation
// (ltpl_fleet_sim_events / _events_read, include/ltpl_hip.h, additive to ABI v9): a per-planner list of events, each a condition and one
// write into the planner's CONFIGURATION (the opponents' vel_scale / length, statics, preference list, the velocity arguments of
// ltpl_fleet_sim_vel, the grip factor on a friction map), executed at the head of every tick of ltpl_fleet_sim_run:
//   k_fleet_sim_events_timed   the LTPL_SIM_WHEN_TICK events of THIS tick, one lane each: the host buckets them by tick when the list is
//                              set and launches the kernel over the tick's bucket only (not at all when it is empty)
//   k_fleet_sim_triggers       the state-conditioned and LTPL_SIM_WHEN_AFTER events, launched in every tick while the list holds some: one
//                              lane per planner walks its triggers (at most LTPL_FLEET_SIM_MAX_TRIGGERS) in list order, so of two that
//                              write one target in one tick the later wins. Its own launch behind the timed kernel: timed first
// Conditions read the state tick k - 1 left (pos_x / pos_y / vel, opp_s, the error word), never configuration. The kernels' pointers live
// in a struct of their own (SimEvt): SimDev and k_fleet_sim_step carry none of them. The target pointers are bound at every launch --
// ltpl_fleet_sim_vel and ltpl_fleet_friction* may re-allocate their buffers between runs. Plain vector loads and stores.
// The host mirror in the same operation order is sim.EventScript.
#pragma once
#include <tuple>

#define SIM_SET_KINDS (LTPL_SIM_SET_FRICTION_SCALE + 1)

struct SimEvt {
    // the list: events of all planners, planner by planner in list order
    const int* planner;                    // [n_events]
    const int* when_kind; const int* when_ref; const double* when_value;   // when_ref: OPP_WITHIN the opponent's element of opp_s; AFTER the event
    const int* set_kind; const int* set_elem; const double* set_value;     // set_elem: the element of the kind's target array
    int* fired;                            // [n_events] schedule tick in which the event fired, -1: not yet
    const int* timed;                      // [n_timed] the timed events, ordered by tick
    const int* trig_off; const int* trig;  // [N + 1], [n_trig] the triggers of planner p
    // state the conditions read
    const unsigned char* state; size_t stride;     // planner blocks: the error word
    const double* pos_x; const double* pos_y; const double* vel; const double* opp_s;
    int n_rl; const double* race;
    // targets, bound at every launch
    double* opp_scale; double* opp_len; double* st_x; double* st_y; double* st_th; double* st_v; double* st_len; int* pref;
    double* vel_max; double* gg_scale; double* gg_ax; double* gg_ay; double* safety_d; int* incl_emerg; double* fr_scale;
};

__device__ __forceinline__ bool sim_evt_failed(const SimEvt& e, int p)
{
    return reinterpret_cast<const fleet::PlannerS*>(e.state + e.stride * (size_t)p)->err != 0;
}
__device__ __forceinline__ void sim_evt_write(const SimEvt& e, int kind, int elem, double v)
{
    switch (kind) {
    case LTPL_SIM_SET_OPP_VEL_SCALE: e.opp_scale[elem] = v; break;
    case LTPL_SIM_SET_OPP_LENGTH: e.opp_len[elem] = v; break;
    case LTPL_SIM_SET_STATIC_X: e.st_x[elem] = v; break;
    case LTPL_SIM_SET_STATIC_Y: e.st_y[elem] = v; break;
    case LTPL_SIM_SET_STATIC_THETA: e.st_th[elem] = v; break;
    case LTPL_SIM_SET_STATIC_V: e.st_v[elem] = v; break;
    case LTPL_SIM_SET_STATIC_LENGTH: e.st_len[elem] = v; break;
    case LTPL_SIM_SET_PREF: e.pref[elem] = (int)v; break;
    case LTPL_SIM_SET_VEL_MAX: e.vel_max[elem] = v; break;
    case LTPL_SIM_SET_GG_SCALE: e.gg_scale[elem] = v; break;
    case LTPL_SIM_SET_GG_AX: e.gg_ax[elem] = v; break;
    case LTPL_SIM_SET_GG_AY: e.gg_ay[elem] = v; break;
    case LTPL_SIM_SET_SAFETY_D: e.safety_d[elem] = v; break;
    case LTPL_SIM_SET_INCL_EMERG: e.incl_emerg[elem] = (int)v; break;
    case LTPL_SIM_SET_FRICTION_SCALE: e.fr_scale[elem] = v; break;
    default: break;
    }
}

// entries [first, first + count) of e.timed: the bucket of schedule tick `tick`. No two of them write the same target (checked when the list
// is set). The emergency flag is written for a failed planner as well: the host's shadow of the flags, which shapes the launches of the
// velocity stage, follows the list without seeing error words (the event is not marked fired; a failed planner runs no jobs)
__global__ __launch_bounds__(64) void k_fleet_sim_events_timed(SimEvt e, int first, int count, int tick)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const int ev = e.timed[first + i];
    const int kind = e.set_kind[ev];
    const bool failed = sim_evt_failed(e, e.planner[ev]);
    if (failed && kind != LTPL_SIM_SET_INCL_EMERG) return;
    sim_evt_write(e, kind, e.set_elem[ev], e.set_value[ev]);
    if (!failed) e.fired[ev] = tick;
}

__global__ __launch_bounds__(64) void k_fleet_sim_triggers(SimEvt e, int n, int tick)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    const int a = e.trig_off[p], b = e.trig_off[p + 1];
    if (a == b || sim_evt_failed(e, p)) return;
    const double px = e.pos_x[p], py = e.pos_y[p], vel = e.vel[p];
    for (int i = a; i < b; ++i) {
        const int ev = e.trig[i];
        if (e.fired[ev] >= 0) continue;
        const int kind = e.when_kind[ev];
        const double v = e.when_value[ev];
        bool fire = false;
        if (kind == LTPL_SIM_WHEN_OPP_WITHIN) {
            const double* s_rl = e.race; const double* cx = s_rl + e.n_rl; const double* cy = cx + e.n_rl;
            const double s = e.opp_s[e.when_ref[ev]];
            const int j = fleet::sim_segment(s, s_rl, e.n_rl);
            const double dx = fleet::sim_interp(s, s_rl, e.n_rl, j, [&](int r) { return cx[r]; }) - px;
            const double dy = fleet::sim_interp(s, s_rl, e.n_rl, j, [&](int r) { return cy[r]; }) - py;
            fire = dx * dx + dy * dy <= v * v;
        } else if (kind == LTPL_SIM_WHEN_VEL_BELOW) fire = vel < v;
        else if (kind == LTPL_SIM_WHEN_VEL_ABOVE) fire = vel > v;
        else if (kind == LTPL_SIM_WHEN_AFTER) {
            const int t0 = e.fired[e.when_ref[ev]];           // (an earlier trigger of this lane's own list)
            fire = t0 >= 0 && (long long)tick == (long long)t0 + (long long)v;
        }
        if (!fire) continue;
        sim_evt_write(e, e.set_kind[ev], e.set_elem[ev], e.set_value[ev]);
        e.fired[ev] = tick;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
struct SimEvents {
    std::vector<void*> allocs;
    SimEvt ev{};                            // the list's device arrays; state and target pointers are bound by sim_events_bind
    int n_events = 0, n_trig = 0;
    int tick = 0;                           // schedule tick: ticks of ltpl_fleet_sim_run since the list was set
    std::vector<int> tk_tick, tk_off;       // the timed events by tick: distinct ticks ascending; entries tk_off[i] .. tk_off[i + 1] - 1 of ev.timed
    size_t cursor = 0;                      // first bucket whose tick is >= `tick`
    std::vector<int> em_off, em_planner, em_value;     // LTPL_SIM_SET_INCL_EMERG events of bucket i: em_off[i] .. em_off[i + 1] - 1 (the host's shadow)
    bool has_friction = false;              // some event writes the grip factor: a run needs maps
};
static void sim_events_free(SimEvents* e)
{
    if (!e) return;
    sim_free_list(e->allocs);
    delete e;
}

static int sim_events_check_run(ltpl_fleet* f)
{
    const SimEvents* e = f->sim->events;
    if (e && e->has_friction && !f->fr_scale) {
        f->err = "fleet sim events: the list holds a LTPL_SIM_SET_FRICTION_SCALE event and no friction maps are set (ltpl_fleet_friction first)";
        return LTPL_ERR_INVALID_ARG;
    }
    return LTPL_OK;
}

static void sim_events_bind(ltpl_fleet* f, SimEvt* v)
{
    const FleetSim& s = *f->sim; const SimDev& d = s.sd; const fleet::FVelIn& vin = s.velt.vin;
    v->state = f->d_state; v->stride = f->D.stride;
    v->pos_x = d.pos_x; v->pos_y = d.pos_y; v->vel = d.vel; v->opp_s = d.opp_s; v->n_rl = d.n_rl; v->race = d.race;
    v->opp_scale = const_cast<double*>(d.opp_scale); v->opp_len = const_cast<double*>(d.opp_len);
    v->st_x = const_cast<double*>(d.st_x); v->st_y = const_cast<double*>(d.st_y); v->st_th = const_cast<double*>(d.st_th);
    v->st_v = const_cast<double*>(d.st_v); v->st_len = const_cast<double*>(d.st_len); v->pref = const_cast<int*>(d.pref);
    v->vel_max = const_cast<double*>(vin.vel_max); v->gg_scale = const_cast<double*>(vin.gg_scale); v->gg_ax = const_cast<double*>(vin.gg_ax);
    v->gg_ay = const_cast<double*>(vin.gg_ay); v->safety_d = const_cast<double*>(vin.safety_d); v->incl_emerg = const_cast<int*>(vin.incl_emerg);
    v->fr_scale = f->fr_scale;
}

// head of a tick of ltpl_fleet_sim_run: the timed events of the schedule tick, then the triggers; t->any_emerg from the host's shadow of
// the emergency flags (FleetSim::emerg / n_emerg, stored by ltpl_fleet_sim_vel), which the passed timed events update. The shadow belongs to
// the simulation, not to the list: ltpl_fleet_sim_run reads it at every call, so a flag an event wrote shapes the launches of later runs
// as well, with another list or with none
static int sim_events_tick(ltpl_fleet* f, FleetTickIn* t)
{
    FleetSim& s = *f->sim; SimEvents& e = *s.events;
    hipStream_t st = f->h->stream;
    SimEvt v = e.ev;
    sim_events_bind(f, &v);
    const int k = e.tick;
    while (e.cursor < e.tk_tick.size() && e.tk_tick[e.cursor] < k) ++e.cursor;
    if (e.cursor < e.tk_tick.size() && e.tk_tick[e.cursor] == k) {
        const size_t c = e.cursor;
        const int first = e.tk_off[c], count = e.tk_off[c + 1] - first;
        hipLaunchKernelGGL(k_fleet_sim_events_timed, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st, v, first, count, k);
        FLEET_TRY(f, hipGetLastError());
        for (int i = e.em_off[c]; i < e.em_off[c + 1]; ++i) {
            int& flag = s.emerg[(size_t)e.em_planner[(size_t)i]];
            s.n_emerg += e.em_value[(size_t)i] - flag;
            flag = e.em_value[(size_t)i];
        }
    }
    if (e.n_trig > 0) {
        const int N = f->D.N;
        hipLaunchKernelGGL(k_fleet_sim_triggers, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, v, N, k);
        FLEET_TRY(f, hipGetLastError());
    }
    t->any_emerg = s.n_emerg > 0 ? 1 : 0;
    ++e.tick;
    return LTPL_OK;
}

// every argument is checked before the first HIP call; the message names the planner and the event (its place in the planner's list)
static int sim_check_events(ltpl_fleet* f, const ltpl_fleet_sim_events_in* in)
{
    const int N = f->D.N;
    if (!f->sim) { f->err = "fleet sim events: ltpl_fleet_sim_setup first"; return LTPL_ERR_INVALID_ARG; }
    if (!in || in->n_events == 0) return LTPL_OK;
    auto bad = [&](const std::string& why, int code = LTPL_ERR_INVALID_ARG) { f->err = "fleet sim events: " + why; return code; };
    if (in->n_events < 0) return bad("n_events must not be negative");
    if (!in->ev_off || !in->when_kind || !in->when_index || !in->when_value || !in->set_kind || !in->set_index || !in->set_value) return bad("an array is missing");
    if (in->ev_off[0] != 0 || in->ev_off[N] != in->n_events) return bad("ev_off must run from 0 to n_events");
    for (int p = 0; p < N; ++p) if (in->ev_off[p + 1] < in->ev_off[p]) return bad("ev_off must not decrease");
    const FleetSim& s = *f->sim;
    struct Key { int tick, kind, elem, planner, local; };
    std::vector<Key> timed;
    for (int p = 0; p < N; ++p) {
        const int e0 = in->ev_off[p], ne = in->ev_off[p + 1] - e0;
        const int n_opp = s.opp_off[(size_t)p + 1] - s.opp_off[(size_t)p], n_st = s.st_off[(size_t)p + 1] - s.st_off[(size_t)p];
        const int n_pref = s.pref_off[(size_t)p + 1] - s.pref_off[(size_t)p];
        int n_trig = 0;
        for (int j = 0; j < ne; ++j) {
            const int e = e0 + j;
            const std::string who = "planner " + std::to_string(p) + " event " + std::to_string(j) + ": ";
            const int wk = in->when_kind[e], wi = in->when_index[e], sk = in->set_kind[e], si = in->set_index[e];
            const double wv = in->when_value[e], sv = in->set_value[e];
            switch (wk) {
            case LTPL_SIM_WHEN_TICK:
                if (wi < 0) return bad(who + "a tick must not be negative");
                break;
            case LTPL_SIM_WHEN_OPP_WITHIN:
                if (wi < 0 || wi >= n_opp) return bad(who + "opponent " + std::to_string(wi) + " out of range (the planner has " + std::to_string(n_opp) + ")");
                if (!std::isfinite(wv) || !(wv >= 0.0)) return bad(who + "a distance must be finite and not negative");
                break;
            case LTPL_SIM_WHEN_VEL_BELOW: case LTPL_SIM_WHEN_VEL_ABOVE:
                if (!std::isfinite(wv)) return bad(who + "a speed must be finite");
                break;
            case LTPL_SIM_WHEN_AFTER:
                if (wi < 0 || wi >= j) return bad(who + "LTPL_SIM_WHEN_AFTER refers to event " + std::to_string(wi) + ": it must be an earlier event of the same planner");
                if (in->when_kind[e0 + wi] == LTPL_SIM_WHEN_TICK) return bad(who + "LTPL_SIM_WHEN_AFTER refers to a timed event (use LTPL_SIM_WHEN_TICK)");
                if (!(wv >= 1.0) || !(wv <= 2147483647.0) || wv != std::floor(wv)) return bad(who + "a delay must be integral and at least 1");
                break;
            default: return bad(who + "unknown condition kind " + std::to_string(wk));
            }
            if (wk != LTPL_SIM_WHEN_TICK && ++n_trig > LTPL_FLEET_SIM_MAX_TRIGGERS)
                return bad("planner " + std::to_string(p) + ": more than " + std::to_string(LTPL_FLEET_SIM_MAX_TRIGGERS) + " triggers", LTPL_ERR_CAPACITY);
            if (sk < 0 || sk >= SIM_SET_KINDS) return bad(who + "unknown write kind " + std::to_string(sk));
            const bool opp = sk == LTPL_SIM_SET_OPP_VEL_SCALE || sk == LTPL_SIM_SET_OPP_LENGTH;
            const bool stat = sk >= LTPL_SIM_SET_STATIC_X && sk <= LTPL_SIM_SET_STATIC_LENGTH;
            const int cnt = opp ? n_opp : stat ? n_st : sk == LTPL_SIM_SET_PREF ? n_pref : 1;
            if (si < 0 || si >= cnt)
                return bad(who + (opp ? "opponent " : stat ? "static object " : sk == LTPL_SIM_SET_PREF ? "preference entry " : "set_index ") + std::to_string(si) +
                           " out of range (" + std::to_string(cnt) + ")");
            if (sk == LTPL_SIM_SET_PREF) {
                if (!(sv >= LTPL_ACT_STRAIGHT && sv <= LTPL_ACT_EMERGENCY) || sv != std::floor(sv)) return bad(who + "unknown action for a preference list");
            } else if (sk == LTPL_SIM_SET_INCL_EMERG) {
                if (wk != LTPL_SIM_WHEN_TICK) return bad(who + "LTPL_SIM_SET_INCL_EMERG comes with LTPL_SIM_WHEN_TICK only (the host derives the launches from it)", LTPL_ERR_UNSUPPORTED);
                if (sv != 0.0 && sv != 1.0) return bad(who + "incl_emerg_traj is 0 or 1");
            } else {
                if (!std::isfinite(sv)) return bad(who + "a value must be finite");
                const bool positive = sk == LTPL_SIM_SET_OPP_LENGTH || sk == LTPL_SIM_SET_STATIC_LENGTH || sk == LTPL_SIM_SET_VEL_MAX || sk == LTPL_SIM_SET_GG_SCALE ||
                                      sk == LTPL_SIM_SET_GG_AX || sk == LTPL_SIM_SET_GG_AY || sk == LTPL_SIM_SET_FRICTION_SCALE;
                if (positive && !(sv > 0.0)) return bad(who + "the value must be positive");
                if ((sk == LTPL_SIM_SET_OPP_VEL_SCALE || sk == LTPL_SIM_SET_SAFETY_D) && !(sv >= 0.0)) return bad(who + "the value must not be negative");
            }
            if (wk == LTPL_SIM_WHEN_TICK) timed.push_back(Key{wi, sk, si, p, j});
        }
    }
    std::sort(timed.begin(), timed.end(), [](const Key& a, const Key& b) {
        return std::tie(a.planner, a.tick, a.kind, a.elem, a.local) < std::tie(b.planner, b.tick, b.kind, b.elem, b.local); });
    for (size_t i = 1; i < timed.size(); ++i) {
        const Key& a = timed[i - 1]; const Key& b = timed[i];
        if (a.planner == b.planner && a.tick == b.tick && a.kind == b.kind && a.elem == b.elem)
            return bad("planner " + std::to_string(b.planner) + " event " + std::to_string(b.local) + ": writes the target of event " + std::to_string(a.local) +
                       " in the same tick " + std::to_string(b.tick));
    }
    return LTPL_OK;
}

extern "C" int ltpl_fleet_sim_events(ltpl_fleet* f, const ltpl_fleet_sim_events_in* in)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    int rc = sim_check_events(f, in);
    if (rc) return rc;
    FleetSim& s = *f->sim;
    if (!in || in->n_events == 0) {
        if (!s.events) return LTPL_OK;
        if ((rc = fleet_enter(f))) return rc;
        FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
        sim_events_free(s.events); s.events = nullptr;
        return LTPL_OK;
    }
    const int N = f->D.N, n = in->n_events;
    std::unique_ptr<SimEvents, void (*)(SimEvents*)> q(new SimEvents(), sim_events_free);
    q->n_events = n;
    // the host resolves local indices to the elements of the target arrays
    std::vector<int> planner((size_t)n), when_ref((size_t)n, 0), set_elem((size_t)n), trig_off((size_t)N + 1, 0), trig, timed;
    const std::vector<int> fired((size_t)n, -1);
    for (int p = 0; p < N; ++p) {
        for (int e = in->ev_off[p]; e < in->ev_off[p + 1]; ++e) {
            planner[(size_t)e] = p;
            const int wk = in->when_kind[e], sk = in->set_kind[e];
            if (wk == LTPL_SIM_WHEN_OPP_WITHIN) when_ref[(size_t)e] = s.opp_off[(size_t)p] + in->when_index[e];
            else if (wk == LTPL_SIM_WHEN_AFTER) when_ref[(size_t)e] = in->ev_off[p] + in->when_index[e];
            if (wk == LTPL_SIM_WHEN_TICK) timed.push_back(e); else trig.push_back(e);
            const int base = sk == LTPL_SIM_SET_OPP_VEL_SCALE || sk == LTPL_SIM_SET_OPP_LENGTH ? s.opp_off[(size_t)p]
                           : sk >= LTPL_SIM_SET_STATIC_X && sk <= LTPL_SIM_SET_STATIC_LENGTH ? s.st_off[(size_t)p]
                           : sk == LTPL_SIM_SET_PREF ? s.pref_off[(size_t)p] : p;
            set_elem[(size_t)e] = base + in->set_index[e];
            if (sk == LTPL_SIM_SET_FRICTION_SCALE) q->has_friction = true;
        }
        trig_off[(size_t)p + 1] = (int)trig.size();
    }
    q->n_trig = (int)trig.size();
    std::stable_sort(timed.begin(), timed.end(), [&](int a, int b) { return in->when_index[a] < in->when_index[b]; });
    for (size_t i = 0; i < timed.size(); ++i) {
        const int e = timed[i], tk = in->when_index[e];
        if (q->tk_tick.empty() || q->tk_tick.back() != tk) { q->tk_tick.push_back(tk); q->tk_off.push_back((int)i); q->em_off.push_back((int)q->em_planner.size()); }
        if (in->set_kind[e] == LTPL_SIM_SET_INCL_EMERG) { q->em_planner.push_back(planner[(size_t)e]); q->em_value.push_back(in->set_value[e] != 0.0 ? 1 : 0); }
    }
    q->tk_off.push_back((int)timed.size()); q->em_off.push_back((int)q->em_planner.size());
    if ((rc = fleet_enter(f))) return rc;
    FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
    // everything new is allocated first; the fleet keeps its previous list, tick and fired ticks unless every step succeeds
    SimAllocs a;
    SimEvt& v = q->ev;
    int* pi = nullptr; double* pd = nullptr;
#define SIM_UP(dst, src, cnt) do { if ((rc = sim_upload(f, a.p, src, (size_t)(cnt), &dst))) return rc; } while (0)
    SIM_UP(pi, planner.data(), n); v.planner = pi;
    SIM_UP(pi, in->when_kind, n); v.when_kind = pi; SIM_UP(pi, when_ref.data(), n); v.when_ref = pi; SIM_UP(pd, in->when_value, n); v.when_value = pd;
    SIM_UP(pi, in->set_kind, n); v.set_kind = pi; SIM_UP(pi, set_elem.data(), n); v.set_elem = pi; SIM_UP(pd, in->set_value, n); v.set_value = pd;
    SIM_UP(v.fired, fired.data(), n);
    SIM_UP(pi, timed.data(), timed.size()); v.timed = pi;
    SIM_UP(pi, trig_off.data(), N + 1); v.trig_off = pi; SIM_UP(pi, trig.data(), trig.size()); v.trig = pi;
#undef SIM_UP
    q->allocs.swap(a.p);
    sim_events_free(s.events);
    s.events = q.release();
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))

extern "C" int ltpl_fleet_sim_events_read(ltpl_fleet* f, int32_t* fired_tick, int32_t* n_events, int32_t* tick)
try {
    if (!f) return LTPL_ERR_INVALID_ARG;
    if (!f->sim) { f->err = "fleet sim events: ltpl_fleet_sim_setup first"; return LTPL_ERR_INVALID_ARG; }
    const SimEvents* e = f->sim->events;
    if (n_events) *n_events = e ? e->n_events : 0;
    if (tick) *tick = e ? e->tick : 0;
    if (e && fired_tick) {
        FLEET_TRY(f, hipSetDevice(f->h->device));
        FLEET_TRY(f, hipStreamSynchronize(f->h->stream));
        FLEET_TRY(f, hipMemcpy(fired_tick, e->ev.fired, sizeof(int32_t) * (size_t)e->n_events, hipMemcpyDeviceToHost));
    }
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(f))
