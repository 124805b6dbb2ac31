// tick_host.hpp -- host side of the tick (path stage + velocity stage in one call): TickLayout, packing and binding of the staging
// buffers, the launches of the fused kernel / the batch pipeline / the graph / the resident kernel, and the entry points ltpl_tick_batch,
// ltpl_tick_batch_compact, ltpl_batch_upload / _run / _run_profile / _download. Included by ltpl_hip.hip behind ltpl_vel_profile (needs
// ltpl_handle, Arena, ensure, InLayout / OutLayout and the *_kernel_of tables).
#pragma once
// ---- fused tick ------------------------------------------------------------------------------------------------------
struct TickLayout {
    InLayout in; size_t axm, vel_plan, vel_est, pos_x, pos_y, veh_vel, in_total;
    OutLayout out; size_t vx, ax, vel_bound, too_close, out_total;
    int n_scen, cap_nodes, cap_pts;
    DevPathsIn di; DevPathsOut dout; DevVelParams p; DevTickVelIn dvin; DevTickVelOut dvout;
    int vel_off, vel_stride, vel_cap; size_t lds;
    int variant;
    // two-kernel batch pipeline (n_scen >= pipeline_min_scen)
    bool pipeline; size_t prep_odist, prep_vobj, prep_ox, prep_oy, prep_idx;
    DevVelPrep dprep; int prep_off, prep_stride;
    VelPlanesLayout planes{};       // the tiled planes of the lane kernels as offsets (bytes == 0: not the pipeline) ...
    VelPlanes vp{};                 // ... and bound to a buffer set (tick_bind_outputs)
};

static int tick_prepare(ltpl_handle* h, const ltpl_paths_in* in, const ltpl_tick_vel_in* vin, int cap_nodes, int cap_pts,
                        TickLayout* t)
{
    int rc = validate_and_layout(h, in, &t->in);
    if (rc) return rc;
    if (!vin || !vin->params) { h->err = "velocity inputs missing"; return LTPL_ERR_INVALID_ARG; }
    if (cap_nodes < h->caps.max_path_nodes || cap_pts < h->caps.max_path_pts) { h->err = "output capacity too small"; return LTPL_ERR_CAPACITY; }
    const int n = in->n_scen;
    for (int s = 0; s < n; ++s)
        if (vin->vel_plan[s] > vin->params->v_max + 0.1) {
            h->err = "vel_plan > v_max + 0.1: the brake-prefix branch is not part of the fused tick (the reference raises at OTH.py:919)";
            return LTPL_ERR_UNSUPPORTED;
        }
    t->n_scen = n; t->cap_nodes = cap_nodes; t->cap_pts = cap_pts;
    t->variant = vel_variant(vin->params);
    Arena a; a.size = t->in.total;
    t->axm = a.add(sizeof(double) * 2 * (size_t)vin->params->n_ax_max_machines);
    t->vel_plan = a.add(sizeof(double) * (size_t)n); t->vel_est = a.add(sizeof(double) * (size_t)n);
    t->pos_x = a.add(sizeof(double) * (size_t)n); t->pos_y = a.add(sizeof(double) * (size_t)n);
    t->veh_vel = a.add(sizeof(double) * (size_t)(t->in.n_veh + 1));
    t->in_total = a.size;
    layout_out(n, cap_nodes, cap_pts, &t->out);
    Arena b; b.size = t->out.total;
    t->vx = b.add(sizeof(double) * (size_t)n * LTPL_MAX_ACTIONS * (size_t)cap_pts);
    t->ax = b.add(sizeof(double) * (size_t)n * LTPL_MAX_ACTIONS * (size_t)cap_pts);
    t->vel_bound = b.add(sizeof(int) * (size_t)n * LTPL_MAX_ACTIONS);
    t->too_close = b.add(sizeof(int) * (size_t)n * LTPL_MAX_ACTIONS);
    t->pipeline = h->long_horizon || (!h->force_fused && (!h->fused_fits || n >= h->pipeline_min_scen));
    t->prep_odist = b.add(sizeof(double) * (size_t)n * LTPL_MAX_ACTIONS);
    t->prep_vobj = b.add(sizeof(double) * (size_t)n * LTPL_MAX_ACTIONS);
    t->prep_ox = b.add(sizeof(double) * (size_t)n * LTPL_MAX_ACTIONS);
    t->prep_oy = b.add(sizeof(double) * (size_t)n * LTPL_MAX_ACTIONS);
    t->prep_idx = b.add(sizeof(int) * (size_t)n * LTPL_MAX_ACTIONS);
    t->out_total = b.size;
    t->planes = vel_planes_layout(n, cap_pts, t->pipeline);
    t->prep_off = 0; t->prep_stride = 0;
    t->vel_cap = h->caps.max_path_pts;
    t->vel_stride = (int)vel_scratch_bytes(t->vel_cap, false, true);
    t->vel_off = h->lp4.total;
    t->lds = fused_tick_lds(h->lp4.total, t->vel_cap);
    if (!t->pipeline && t->lds > FUSED_TICK_LDS_BUDGET) { h->err = "fused tick exceeds the LDS budget"; return LTPL_ERR_CAPACITY; }   // (LTPL_FORCE_FUSED)
    return LTPL_OK;
}

// device-side output pointers of a tick layout for one buffer set (output slab + tiled planes)
static void tick_bind_outputs(TickLayout* t, unsigned char* dob, unsigned char* planes)
{
    bind_out(dob, t->out, t->cap_nodes, t->cap_pts, &t->dout);
    bind_at(t->dvout.vx, dob, t->vx); bind_at(t->dvout.ax, dob, t->ax); bind_at(t->dvout.vel_bound, dob, t->vel_bound); bind_at(t->dvout.too_close, dob, t->too_close);
    bind_at(t->dprep.obj_dist, dob, t->prep_odist); bind_at(t->dprep.v_obj, dob, t->prep_vobj); bind_at(t->dprep.obj_x, dob, t->prep_ox);
    bind_at(t->dprep.obj_y, dob, t->prep_oy); bind_at(t->dprep.idx_s_opp, dob, t->prep_idx);
    if (t->pipeline && planes) {
        const VelPlanesLayout& L = t->planes;
        static_assert(sizeof(ke_t) <= 2 * sizeof(double), "operand plane: two doubles per row and tile");
        bind_at(t->vp.KE, planes, L.KE); bind_at(t->vp.P0, planes, L.P0); bind_at(t->vp.P1, planes, L.P1); bind_at(t->vp.P2, planes, L.P2);
        bind_at(t->vp.P3, planes, L.P3); bind_at(t->vp.XY, planes, L.XY); bind_at(t->vp.flags, planes, L.flags); bind_at(t->vp.fseg, planes, L.fseg);
        bind_at(t->dout.job_slot, planes, L.job_slot); bind_at(t->dout.job_cnt, planes, L.job_cnt);
        t->vp.cap_pts = t->cap_pts; t->vp.plane_rows = L.plane_rows; t->dout.n_slots_pad = L.n_slots_pad;
        t->dout.vke = t->vp.KE; t->dout.vxy = t->vp.XY;
    }
}

static int tick_pack(ltpl_handle* h, const ltpl_paths_in* in, const ltpl_tick_vel_in* vin, TickLayout* t,
                     unsigned char* hb, unsigned char* db, unsigned char* dob)
{
    pack_in(in, t->in, hb, db, &t->di, h->scen_order != 0);
    const int n = in->n_scen;
    memcpy(hb + t->axm, vin->params->ax_max_machines, sizeof(double) * 2 * (size_t)vin->params->n_ax_max_machines);
    memcpy(hb + t->vel_plan, vin->vel_plan, sizeof(double) * (size_t)n);
    memcpy(hb + t->vel_est, vin->vel_est, sizeof(double) * (size_t)n);
    memcpy(hb + t->pos_x, vin->pos_est_x, sizeof(double) * (size_t)n);
    memcpy(hb + t->pos_y, vin->pos_est_y, sizeof(double) * (size_t)n);
    if (t->in.n_veh > 0) memcpy(hb + t->veh_vel, vin->veh_vel, sizeof(double) * (size_t)t->in.n_veh);
    int rc = make_vel_params(h, vin->params, reinterpret_cast<const double*>(db + t->axm), &t->p);
    if (rc) return rc;
    t->dvin.gg_ax = vin->gg_ax; t->dvin.gg_ay = vin->gg_ay; t->dvin.safety_d = vin->safety_d;
    t->dvin.v_max_offset = vin->v_max_offset;
    bind_at(t->dvin.vel_plan, db, t->vel_plan); bind_at(t->dvin.vel_est, db, t->vel_est); bind_at(t->dvin.pos_est_x, db, t->pos_x);
    bind_at(t->dvin.pos_est_y, db, t->pos_y); bind_at(t->dvin.veh_vel, db, t->veh_vel);
    if ((rc = grow_device(h, &h->d_planes, &h->d_planes_cap, t->planes.bytes))) return rc;
    tick_bind_outputs(t, dob, static_cast<unsigned char*>(h->d_planes));
    return LTPL_OK;
}

static int tick_launch_paths(ltpl_handle* h, const TickLayout& t, hipStream_t st)
{
    if (t.dout.job_cnt) HIP_TRY(h, hipMemsetAsync(t.dout.job_cnt, 0, 3 * sizeof(int), st));
    return launch_paths(h, (t.n_scen >= h->nw1_min_scen && h->batch_nw == 1) ? 1 : NUM_WAVES, t.n_scen, st, t.di, t.dout);
}

static int tick_launch_vel(ltpl_handle* h, const TickLayout& t, hipStream_t st, hipEvent_t ev_after_prep = nullptr)
{
    // slots without a path: vel_bound = too_close = 0 (the job kernels only touch slots that own a job)
    HIP_TRY(h, hipMemsetAsync(t.dvout.vel_bound, 0, sizeof(int) * (size_t)t.n_scen * LTPL_MAX_ACTIONS, st));
    HIP_TRY(h, hipMemsetAsync(t.dvout.too_close, 0, sizeof(int) * (size_t)t.n_scen * LTPL_MAX_ACTIONS, st));
#ifdef LTPL_EXPERIMENT
    if (!(h->exp_skip & 1))
#endif
    hipLaunchKernelGGL(k_follow_prep, dim3((t.n_scen + 63) / 64), dim3(64), 0, st, h->lat, t.di, t.dout,
                       t.dvin, t.dprep, t.vp, t.n_scen, h->lp4.dbg);
    HIP_TRY(h, hipGetLastError());
    if (ev_after_prep) HIP_TRY(h, hipEventRecord(ev_after_prep, st));
    const int n_slots = t.n_scen * LTPL_MAX_ACTIONS;
    const int nb0 = (n_slots + 63) / 64, nb1 = (t.n_scen + 63) / 64;
    const int emit_generic = t.n_scen >= LTPL_EMIT_MIN_SCEN ? 1 : 0;
    const int emit = emit_generic | ((emit_generic && t.n_scen >= h->follow_emit_min_scen) ? 2 : 0);
#ifdef LTPL_EXPERIMENT
    if (!(h->exp_skip & 2))
#endif
    hipLaunchKernelGGL(lanes_kernel_of(t.variant), dim3(nb0 + 2 * nb1), dim3(64), 0, st, h->lat, t.di, t.dout,
                       t.p, t.dvin, t.dprep, t.vp, n_slots, t.n_scen, nb0, h->lp4.dbg, t.dvout, emit);
    HIP_TRY(h, hipGetLastError());
#ifdef LTPL_EXPERIMENT
    if (!(h->exp_skip & 4))
#endif
    hipLaunchKernelGGL(k_vel_final, dim3(emit_generic ? nb1 : nb0 + nb1, h->final_y), dim3(64), 0, st, t.dout, t.dvin, t.dvout, t.vp, n_slots, t.n_scen,
                       emit_generic ? nb0 : 0);
    HIP_TRY(h, hipGetLastError());
    return LTPL_OK;
}

static int tick_launch(ltpl_handle* h, const TickLayout& t, hipEvent_t* ev = nullptr)
{
    // ev (optional, 4 events): recorded before the path kernel, after it, after the follow preparation, after the lane kernels
    if (ev) HIP_TRY(h, hipEventRecord(ev[0], h->stream));
    if (t.pipeline) {
        int rc = tick_launch_paths(h, t, h->stream);
        if (rc) return rc;
        if (ev) HIP_TRY(h, hipEventRecord(ev[1], h->stream));
        if ((rc = tick_launch_vel(h, t, h->stream, ev ? ev[2] : nullptr))) return rc;
        if (ev) HIP_TRY(h, hipEventRecord(ev[3], h->stream));
        return LTPL_OK;
    }
    hipLaunchKernelGGL(tick_kernel_of(t.variant, h->plan_class4 == 1), dim3(t.n_scen), dim3(WG_THREADS), t.lds, h->stream, h->lat, t.di, t.dout, h->lp4, t.p,
                       t.dvin, t.dvout, t.vel_off, t.vel_stride, t.vel_cap);
    HIP_TRY(h, hipGetLastError());
    if (ev) { HIP_TRY(h, hipEventRecord(ev[1], h->stream)); HIP_TRY(h, hipEventRecord(ev[2], h->stream)); HIP_TRY(h, hipEventRecord(ev[3], h->stream)); }
    return LTPL_OK;
}

static void tick_scatter(const unsigned char* hb, const TickLayout& t, ltpl_paths_out* out, ltpl_tick_vel_out* vout)
{
    scatter_out(hb, t.out, t.n_scen, out);
    const size_t A = LTPL_MAX_ACTIONS, n = (size_t)t.n_scen;
    if (out->cap_pts == t.cap_pts) {
        memcpy(vout->vx, hb + t.vx, sizeof(double) * n * A * (size_t)t.cap_pts);
        memcpy(vout->ax, hb + t.ax, sizeof(double) * n * A * (size_t)t.cap_pts);
    }
    memcpy(vout->vel_bound, hb + t.vel_bound, sizeof(int) * n * A);
    memcpy(vout->too_close, hb + t.too_close, sizeof(int) * n * A);
}

static int tick_set_lds_limit(ltpl_handle* h, size_t lds, int variant)
{
    if (!h->fused_fits) return LTPL_OK;                   // the fused kernel is not used
    const bool plan_a = h->plan_class4 == 1;
    return raise_lds_limit(h, reinterpret_cast<const void*>(tick_kernel_of(variant, plan_a)), lds, (plan_a ? LDS_SLOT_TICK_A : LDS_SLOT_TICK) + variant);
}

// The fused single tick as one hipGraph launch (LTPL_TICK_GRAPH=1): copy node (packed inputs, H2D) -> kernel node (k_tick) -> copy node
// (outputs, D2H; absent with zero-copy outputs). Built once; every tick re-parameterises the nodes of the executable graph (sizes and the
// pointers into the staging buffers follow the tick's counts) and launches it. A change of topology or kernel rebuilds the graph.
static int tick_launch_graph(ltpl_handle* h, TickLayout& t, bool zc)
{
    const void* func = reinterpret_cast<const void*>(tick_kernel_of(t.variant, h->plan_class4 == 1));
    int vel_off = t.vel_off, vel_stride = t.vel_stride, vel_cap = t.vel_cap;
    void* kargs[] = {&h->lat, &t.di, &t.dout, &h->lp4, &t.p, &t.dvin, &t.dvout, &vel_off, &vel_stride, &vel_cap};
    hipKernelNodeParams kp{};
    kp.func = const_cast<void*>(func); kp.gridDim = dim3(t.n_scen); kp.blockDim = dim3(WG_THREADS); kp.sharedMemBytes = (unsigned)t.lds;
    kp.kernelParams = kargs; kp.extra = nullptr;
    const int has_out = zc ? 0 : 1;
    bool ok = h->tg_exec && h->tg_func == func && h->tg_has_out == has_out;
    if (ok) {
        ok = hipGraphExecMemcpyNodeSetParams1D(h->tg_exec, h->tg_n_in, h->d_in, h->h_in, t.in_total, hipMemcpyHostToDevice) == hipSuccess &&
             hipGraphExecKernelNodeSetParams(h->tg_exec, h->tg_n_k, &kp) == hipSuccess &&
             (!has_out || hipGraphExecMemcpyNodeSetParams1D(h->tg_exec, h->tg_n_out, h->h_out, h->d_out, t.out_total, hipMemcpyDeviceToHost) == hipSuccess);
        if (!ok) (void)hipGetLastError();
    }
    if (!ok) {
        if (h->tg_exec) { (void)hipGraphExecDestroy(h->tg_exec); h->tg_exec = nullptr; }
        if (h->tg_graph) { (void)hipGraphDestroy(h->tg_graph); h->tg_graph = nullptr; }
        HIP_TRY(h, hipGraphCreate(&h->tg_graph, 0));
        HIP_TRY(h, hipGraphAddMemcpyNode1D(&h->tg_n_in, h->tg_graph, nullptr, 0, h->d_in, h->h_in, t.in_total, hipMemcpyHostToDevice));
        HIP_TRY(h, hipGraphAddKernelNode(&h->tg_n_k, h->tg_graph, &h->tg_n_in, 1, &kp));
        if (has_out) HIP_TRY(h, hipGraphAddMemcpyNode1D(&h->tg_n_out, h->tg_graph, &h->tg_n_k, 1, h->h_out, h->d_out, t.out_total, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipGraphInstantiate(&h->tg_exec, h->tg_graph, nullptr, nullptr, 0));
        h->tg_func = func; h->tg_has_out = has_out;
    }
    HIP_TRY(h, hipGraphLaunch(h->tg_exec, h->stream));
    return LTPL_OK;
}

// ---- the persistent single tick (k_tick_persistent): host side --------------------------------------------------------------------------
typedef void (*ptick_kernel_t)(const TickKArgs*, TickMailbox*, const unsigned char*, unsigned char*, unsigned, unsigned long long);
static ptick_kernel_t ptick_kernel_of(int v)
{
    return with_vel_variant(v, [](auto em, auto axm1) -> ptick_kernel_t { return k_tick_persistent<em.value, axm1.value, PlanA4>; });
}

// Tell the resident kernel to leave and wait until it has (every entry point that reuses the staging buffers or synchronises the device
// calls this first; ltpl_destroy too). Cheap when nothing is resident.
static void persist_stop(ltpl_handle* h)
{
    ltpl_handle::PersistTick& P = h->pt;
    if (!P.running) return;
    __atomic_store_n(&P.mb->cmd, PT_CMD_EXIT, __ATOMIC_RELAXED);
    if (++P.seq == 0u) ++P.seq;
    __atomic_store_n(&P.mb->seq, P.seq, __ATOMIC_RELEASE);
    (void)hipStreamSynchronize(P.stream);                     // the kernel sees the command within one poll (or had idled out already)
    P.busy_clk += P.mb->busy_clk; P.busy_n += P.mb->n_done;
    P.running = 0;
}

static int persist_start(ltpl_handle* h, const TickLayout& t, unsigned start_seq)
{
    ltpl_handle::PersistTick& P = h->pt;
    if (!P.stream) {
        // at the device's highest stream priority: the runtime keeps its hardware queues per priority, and nothing else of the library
        // asks for this one by default -- the resident kernel, which never completes, then has a hardware queue that no stream of
        // another handle (or fleet) shares, whatever their number. On a normal-priority stream it shared one of the (4 by default)
        // queues with every other stream of the process mapped there: a kernel another handle launched behind it waited for the idle
        // limit, and every persistent tick started the resident kernel again
        int lo_p = 0, hi_p = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);
        HIP_TRY(h, hipStreamCreateWithPriority(&P.stream, hipStreamNonBlocking, hi_p));
    }
    if (!P.mb) {
        HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&P.mb), sizeof(TickMailbox), hipHostMallocDefault));
        memset(P.mb, 0, sizeof(TickMailbox));
    }
    if (!P.d_args) HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&P.d_args), 2048));
    int rc = raise_lds_limit(h, reinterpret_cast<const void*>(ptick_kernel_of(t.variant)), t.lds, LDS_SLOT_PTICK + t.variant);
    if (rc) return rc;
    P.mb->exited = 0; P.mb->n_done = 0; P.mb->busy_clk = 0; P.mb->cmd = PT_CMD_TICK;
    __atomic_store_n(&P.mb->seq, start_seq, __ATOMIC_RELEASE);
    const unsigned long long idle_limit = (unsigned long long)(P.idle_ms * 1e5);           // wall_clock64 counts at 100 MHz
    hipLaunchKernelGGL(ptick_kernel_of(t.variant), dim3(1), dim3(WG_THREADS), t.lds, P.stream, (const TickKArgs*)P.d_args, P.mb,
                       static_cast<const unsigned char*>(h->h_in), static_cast<unsigned char*>(h->d_in), start_seq, idle_limit);
    HIP_TRY(h, hipGetLastError());
    P.running = 1; P.variant = t.variant; P.lds = t.lds; P.h_in = h->h_in; P.d_in = h->d_in; P.seq = start_seq; ++P.launches;
    return LTPL_OK;
}

// one tick through the resident kernel: staging buffers packed as for k_tick (zero-copy outputs, polled completion word)
static int persist_tick(ltpl_handle* h, TickLayout& t)
{
    ltpl_handle::PersistTick& P = h->pt;
    // the kernel idled out since the last tick (its last store: `exited`), or serves another kernel variant / other buffers: (re)start
    if (P.running && __atomic_load_n(&P.mb->exited, __ATOMIC_ACQUIRE) != 0u) {
        HIP_TRY(h, hipStreamSynchronize(P.stream));
        P.busy_clk += P.mb->busy_clk; P.busy_n += P.mb->n_done; P.running = 0;
    }
    if (P.running && (P.variant != t.variant || P.lds != t.lds || P.h_in != h->h_in || P.d_in != h->d_in)) persist_stop(h);
    int rc;
    if (!P.running && (rc = persist_start(h, t, P.seq))) return rc;
    TickKArgs ka;
    memset(&ka, 0, sizeof(ka));
    ka.pk.lat = h->lat; ka.pk.in = t.di; ka.pk.out = t.dout; ka.pk.lp = h->lp4;
    ka.p = t.p; ka.vin = t.dvin; ka.vout = t.dvout; ka.vel_off = t.vel_off; ka.vel_stride = t.vel_stride; ka.vel_cap = t.vel_cap;
    memcpy(P.mb->args, &ka, sizeof(ka));
    P.mb->in_bytes = (unsigned)align_up(t.in_total, 16);
    P.mb->cmd = PT_CMD_TICK;
    if (++P.seq == 0u) ++P.seq;
    __atomic_store_n(&P.mb->seq, P.seq, __ATOMIC_RELEASE);
    const unsigned want = t.dout.done.seq;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 1;; ++spins) {
        if (__atomic_load_n(h->h_flag, __ATOMIC_ACQUIRE) == want) break;
        if ((spins & 0xfffu) != 0u) continue;
        if (__atomic_load_n(&P.mb->exited, __ATOMIC_ACQUIRE) != 0u) {
            // the kernel left (idle limit) between our check and our post: it cannot have seen this tick -- unless the completion word says so
            HIP_TRY(h, hipStreamSynchronize(P.stream));
            P.busy_clk += P.mb->busy_clk; P.busy_n += P.mb->n_done; P.running = 0;
            if (__atomic_load_n(h->h_flag, __ATOMIC_ACQUIRE) == want) break;
            const unsigned posted = P.seq;
            if ((rc = persist_start(h, t, posted - 1u))) return rc;    // the new kernel starts "one behind" ...
            P.seq = posted;
            __atomic_store_n(&P.mb->seq, posted, __ATOMIC_RELEASE);  // ... and finds the tick that is still in the mailbox
            continue;
        }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2000)) {
            __atomic_store_n(&P.mb->cmd, PT_CMD_EXIT, __ATOMIC_RELAXED);
            h->err = "persistent tick: no completion within 2 s"; return LTPL_ERR_HIP;
        }
    }
    ++P.ticks;
    return LTPL_OK;
}

extern "C" int ltpl_tick_persistent_stop(ltpl_handle* h)
try {
    if (!h) return LTPL_ERR_INVALID_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    persist_stop(h);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(h))

extern "C" int ltpl_tick_persistent_stats(ltpl_handle* h, ltpl_persistent_stats* st)
try {
    if (!h || !st) return LTPL_ERR_INVALID_ARG;
    const ltpl_handle::PersistTick& P = h->pt;
    st->enabled = P.enabled; st->resident = (P.running && P.mb && __atomic_load_n(&P.mb->exited, __ATOMIC_ACQUIRE) == 0u) ? 1 : 0;
    st->ticks = (long long)P.ticks; st->launches = (long long)P.launches;
    unsigned long long clk = P.busy_clk, n = P.busy_n;
    if (P.running && P.mb) { clk += P.mb->busy_clk; n += P.mb->n_done; }
    st->device_us_mean = n ? (double)clk / (double)n / 100.0 : 0.0;
    st->device_us_last = (P.mb ? (double)P.mb->last_clk : 0.0) / 100.0;
    st->idle_ms = P.idle_ms;
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(h))

extern "C" int ltpl_tick_batch(ltpl_handle* h, const ltpl_paths_in* in, const ltpl_tick_vel_in* vin, ltpl_paths_out* out,
                               ltpl_tick_vel_out* vout)
try {
    if (!h) return LTPL_ERR_INVALID_ARG;
    if (!out || !vout) { h->err = "null output"; return LTPL_ERR_INVALID_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    const bool persistent = h->pt.enabled && in && in->n_scen == 1 && h->zc_out && !h->d_dbg;
    drop_resident(h, persistent);
    TickLayout t;
    int rc = tick_prepare(h, in, vin, out->cap_nodes, out->cap_pts, &t);
    if (rc) return rc;
    if (persistent && !t.pipeline) {
        // (growing a staging buffer frees the old one: the resident kernel leaves first -- persist_tick starts it again on the new buffers)
        if (t.in_total > h->h_in_cap || t.in_total > h->d_in_cap || t.out_total > h->h_out_cap || t.out_total > h->d_out_cap) persist_stop(h);
        if ((rc = ensure(h, &h->h_in, &h->h_in_cap, &h->d_in, &h->d_in_cap, align_up(t.in_total, 16)))) return rc;
        if ((rc = ensure(h, &h->h_out, &h->h_out_cap, &h->d_out, &h->d_out_cap, t.out_total))) return rc;
        if ((rc = tick_pack(h, in, vin, &t, static_cast<unsigned char*>(h->h_in), static_cast<unsigned char*>(h->d_in),
                            static_cast<unsigned char*>(h->h_out)))) return rc;
        t.dout.done = next_done_signal(h);
        if ((rc = persist_tick(h, t))) return rc;
        tick_scatter(static_cast<const unsigned char*>(h->h_out), t, out, vout);
        return LTPL_OK;
    }
    persist_stop(h);
    if ((rc = ensure(h, &h->h_in, &h->h_in_cap, &h->d_in, &h->d_in_cap, t.in_total))) return rc;
    if ((rc = ensure(h, &h->h_out, &h->h_out_cap, &h->d_out, &h->d_out_cap, t.out_total))) return rc;
    // single ticks (fused kernel): outputs straight into the page-locked buffer, completion through the polled word (see plan_paths_impl)
    const bool zc = h->zc_out && !t.pipeline && in->n_scen <= 8;
    const bool polled = zc && h->poll && !h->d_dbg;
    if ((rc = tick_pack(h, in, vin, &t, static_cast<unsigned char*>(h->h_in), static_cast<unsigned char*>(h->d_in),
                        static_cast<unsigned char*>(zc ? h->h_out : h->d_out)))) return rc;
    if (polled) t.dout.done = next_done_signal(h);
    if ((rc = tick_set_lds_limit(h, t.lds, t.variant))) return rc;
    if (h->tick_graph && !t.pipeline) {
        if ((rc = tick_launch_graph(h, t, zc))) return rc;
    } else {
        HIP_TRY(h, hipMemcpyAsync(h->d_in, h->h_in, t.in_total, hipMemcpyHostToDevice, h->stream));
        if ((rc = tick_launch(h, t))) return rc;
        if (!zc) HIP_TRY(h, hipMemcpyAsync(h->h_out, h->d_out, t.out_total, hipMemcpyDeviceToHost, h->stream));
    }
    if (polled) { if ((rc = wait_done(h, t.dout.done.seq))) return rc; }
    else HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (t.pipeline) dbg_report_lanes(h); else dbg_report(h, "k_tick", in->n_scen);
    tick_scatter(static_cast<const unsigned char*>(h->h_out), t, out, vout);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(h))

extern "C" void* ltpl_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
extern "C" void ltpl_host_free(void* p) { if (p) (void)hipHostFree(p); }

extern "C" int ltpl_tick_batch_compact(ltpl_handle* h, const ltpl_paths_in* in, const ltpl_tick_vel_in* vin, ltpl_traj_out* out)
try {
    if (!h) return LTPL_ERR_INVALID_ARG;
    if (!out || !out->rows || !out->action_id || !out->n_rows || !out->vel_bound || !out->reduced || !out->row_off || out->capacity_rows < 0) {
        h->err = "null output"; return LTPL_ERR_INVALID_ARG;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    drop_resident(h);
    TickLayout t;
    int rc = tick_prepare(h, in, vin, h->caps.max_path_nodes, h->caps.max_path_pts, &t);
    if (rc) return rc;
    const size_t n_slots = (size_t)in->n_scen * LTPL_MAX_ACTIONS;
    // device scratch behind the regular output slab: rows kept, offsets, total, packed rows
    Arena b; b.size = t.out_total;
    const size_t o_rows = b.add(sizeof(int) * n_slots), o_off = b.add(sizeof(long long) * n_slots), o_tot = b.add(sizeof(long long));
    const size_t o_pack = b.add(sizeof(double) * 7 * (size_t)out->capacity_rows);
    if ((rc = ensure(h, &h->h_in, &h->h_in_cap, &h->d_in, &h->d_in_cap, t.in_total))) return rc;
    // host staging only for the small per-slot arrays (+ the packed rows when the caller's buffer is not page-locked)
    hipPointerAttribute_t attr; bool pinned = false;
    if (hipPointerGetAttributes(&attr, out->rows) == hipSuccess) pinned = attr.type == hipMemoryTypeHost;
    else (void)hipGetLastError();
    Arena hs;
    const size_t s_rows = hs.add(sizeof(int) * n_slots), s_act = hs.add(sizeof(int) * n_slots), s_vb = hs.add(sizeof(int) * n_slots);
    const size_t s_red = hs.add(sizeof(int) * n_slots), s_off = hs.add(sizeof(long long) * n_slots), s_tot = hs.add(sizeof(long long));
    const size_t s_pack = hs.add(pinned ? 0 : sizeof(double) * 7 * (size_t)out->capacity_rows);
    if ((rc = ensure(h, &h->h_out, &h->h_out_cap, &h->d_out, &h->d_out_cap, b.size > hs.size ? b.size : hs.size))) return rc;
    if ((rc = tick_pack(h, in, vin, &t, static_cast<unsigned char*>(h->h_in), static_cast<unsigned char*>(h->d_in),
                        static_cast<unsigned char*>(h->d_out)))) return rc;
    if ((rc = tick_set_lds_limit(h, t.lds, t.variant))) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->d_in, h->h_in, t.in_total, hipMemcpyHostToDevice, h->stream));
    if ((rc = tick_launch(h, t))) return rc;
    unsigned char* dob = static_cast<unsigned char*>(h->d_out);
    int* d_rows = reinterpret_cast<int*>(dob + o_rows); long long* d_off = reinterpret_cast<long long*>(dob + o_off);
    long long* d_tot = reinterpret_cast<long long*>(dob + o_tot); double* d_pack = reinterpret_cast<double*>(dob + o_pack);
    hipLaunchKernelGGL(k_compact_offsets, dim3(1), dim3(1024), 0, h->stream, t.dout.valid, t.dout.n_pts, (int)n_slots, out->max_rows, d_rows, d_off, d_tot);
    hipLaunchKernelGGL(k_compact_rows, dim3((unsigned)n_slots), dim3(64), 0, h->stream, t.dout, t.dvout, d_rows, d_off, d_pack, (long long)out->capacity_rows);
    HIP_TRY(h, hipGetLastError());
    // small arrays first (they tell how many packed bytes there are)
    unsigned char* hb = static_cast<unsigned char*>(h->h_out);
    int* h_rows = reinterpret_cast<int*>(hb + s_rows); int* h_act = reinterpret_cast<int*>(hb + s_act);
    int* h_vb = reinterpret_cast<int*>(hb + s_vb); int* h_red = reinterpret_cast<int*>(hb + s_red);
    long long* h_off = reinterpret_cast<long long*>(hb + s_off); long long* h_tot = reinterpret_cast<long long*>(hb + s_tot);
    HIP_TRY(h, hipMemcpyAsync(h_rows, d_rows, sizeof(int) * n_slots, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h_act, t.dout.action_id, sizeof(int) * n_slots, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h_vb, t.dvout.vel_bound, sizeof(int) * n_slots, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h_red, t.dout.reduced, sizeof(int) * n_slots, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h_off, d_off, sizeof(long long) * n_slots, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h_tot, d_tot, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const long long total = *h_tot;
    out->total_rows = total;
    if (total > out->capacity_rows) { h->err = "ltpl_traj_out.capacity_rows too small (total_rows holds the need)"; return LTPL_ERR_CAPACITY; }
    double* h_pack = pinned ? out->rows : reinterpret_cast<double*>(hb + s_pack);
    if (total > 0) {
        HIP_TRY(h, hipMemcpyAsync(h_pack, d_pack, sizeof(double) * 7 * (size_t)total, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (!pinned) memcpy(out->rows, h_pack, sizeof(double) * 7 * (size_t)total);
    }
    memcpy(out->n_rows, h_rows, sizeof(int) * n_slots); memcpy(out->action_id, h_act, sizeof(int) * n_slots);
    memcpy(out->vel_bound, h_vb, sizeof(int) * n_slots); memcpy(out->reduced, h_red, sizeof(int) * n_slots);
    memcpy(out->row_off, h_off, sizeof(long long) * n_slots);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(h))

// device-resident batch (benchmarks): inputs stay in HBM, the fused kernel is replayed on the handle's stream
extern "C" int ltpl_batch_upload(ltpl_handle* h, const ltpl_paths_in* in, const ltpl_tick_vel_in* vin, int32_t cap_nodes,
                                 int32_t cap_pts)
try {
    if (!h) return LTPL_ERR_INVALID_ARG;
    HIP_TRY(h, hipSetDevice(h->device));
    drop_resident(h);
    std::unique_ptr<TickLayout> owned(new TickLayout());        // (the handle's from `h->resident = ...` on: every return before that frees it)
    TickLayout* t = owned.get();
    int rc = tick_prepare(h, in, vin, cap_nodes, cap_pts, t);
    if (rc) return rc;
    if ((rc = ensure(h, &h->h_in, &h->h_in_cap, &h->d_in, &h->d_in_cap, t->in_total))) return rc;
    if ((rc = ensure(h, &h->h_out, &h->h_out_cap, &h->d_out, &h->d_out_cap, t->out_total))) return rc;
    if ((rc = tick_pack(h, in, vin, t, static_cast<unsigned char*>(h->h_in), static_cast<unsigned char*>(h->d_in),
                        static_cast<unsigned char*>(h->d_out)))) return rc;
    if ((rc = tick_set_lds_limit(h, t->lds, t->variant))) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->d_in, h->h_in, t->in_total, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->resident = owned.release();
    h->last_set = 0;
    if (t->pipeline && !h->no_overlap) {
        // further buffer sets for the software pipeline of ltpl_batch_run
        for (int i = 0; i < ltpl_handle::VEL_STREAMS; ++i) if (!h->vel_stream[i]) {
            // LTPL_VEL_STREAM_PRIO=1 (experiment): the velocity streams at the device's highest stream priority (their waves are dispatched
            // ahead of the path kernel's whenever a slot frees up)
            static const bool hi = getenv("LTPL_VEL_STREAM_PRIO") && atoi(getenv("LTPL_VEL_STREAM_PRIO")) != 0;
            // LTPL_VEL_CUS=<n> (round-5 experiment): the velocity streams confined to n compute units by a CU mask. The velocity waves are few,
            // long-lived (a serial recurrence over the rows of a profile) and hold 197 VGPRs: next to one of them a SIMD keeps two path waves
            // instead of four. Confined, they run among themselves on a corner of the chip. 0 / unset: no mask.
            static const int vel_cus = getenv("LTPL_VEL_CUS") ? atoi(getenv("LTPL_VEL_CUS")) : 0;
            bool made = false;
            if (vel_cus > 0) {
                const int ncu = h->caps.num_cus > 0 ? h->caps.num_cus : 256;
                std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
                for (int c = 0; c < vel_cus && c < ncu; ++c) mask[(size_t)c >> 5] |= 1u << (c & 31);
                made = hipExtStreamCreateWithCUMask(&h->vel_stream[i], (uint32_t)mask.size(), mask.data()) == hipSuccess;
                if (!made) { (void)hipGetLastError(); h->vel_stream[i] = nullptr; }
            }
            if (made) continue;
            if (hi) { int lo_p = 0, hi_p = 0; (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p); HIP_TRY(h, hipStreamCreateWithPriority(&h->vel_stream[i], hipStreamNonBlocking, hi_p)); }
            else HIP_TRY(h, hipStreamCreateWithFlags(&h->vel_stream[i], hipStreamNonBlocking));
        }
        {
            const char* ps = getenv("LTPL_PATH_STREAMS");
            h->path_streams = (ps && atoi(ps) == 2) ? 2 : 1;
            if (h->path_streams == 2 && !h->path_stream2) HIP_TRY(h, hipStreamCreateWithFlags(&h->path_stream2, hipStreamNonBlocking));
            if (!h->ev_begin) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_begin, hipEventDisableTiming));
        }
        for (int i = 0; i < ltpl_handle::PIPE_SETS; ++i) {
            if (!h->ev_paths[i]) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_paths[i], hipEventDisableTiming));
            if (!h->ev_vel[i]) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_vel[i], hipEventDisableTiming));
        }
        for (int i = 0; i < ltpl_handle::PIPE_SETS - 1; ++i) {
            if ((rc = grow_device(h, &h->d_out_x[i], &h->d_out_x_cap[i], t->out_total))) return rc;
            if ((rc = grow_device(h, &h->d_planes_x[i], &h->d_planes_x_cap[i], t->planes.bytes))) return rc;
            std::unique_ptr<TickLayout> tx(new TickLayout(*t));
            tick_bind_outputs(tx.get(), static_cast<unsigned char*>(h->d_out_x[i]), static_cast<unsigned char*>(h->d_planes_x[i]));
            h->resident_x[i] = tx.release();
        }
    }
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(h))

extern "C" int ltpl_batch_run(ltpl_handle* h, int reps, float* ms_total)
try {
    if (!h) return LTPL_ERR_INVALID_ARG;
    if (!h->resident) { h->err = "no resident batch: call ltpl_batch_upload first"; return LTPL_ERR_INVALID_ARG; }
    if (reps < 1) { h->err = "reps < 1"; return LTPL_ERR_INVALID_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ms_total) {
        HIP_TRY(h, hipEventCreate(&e0)); HIP_TRY(h, hipEventCreate(&e1));
        HIP_TRY(h, hipEventRecord(e0, h->stream));
    }
    if (h->resident_x[0] && ms_total) {
        while (h->ev_step.size() < 2 * (size_t)reps) { hipEvent_t e; HIP_TRY(h, hipEventCreate(&e)); h->ev_step.push_back(e); }
    }
    h->last_paths_ms = 0.0f; h->last_paths_n = 0;
    if (h->resident_x[0]) {
        // software pipeline over steps: path kernel of step r on `stream`, velocity kernels of step r on `vel_stream[r % VEL_STREAMS]` (alternating:
        // the chains of consecutive steps run next to each other), PIPE_SETS buffer sets; the path kernel of step r + PIPE_SETS waits
        // until the velocity kernels of step r released its set
        constexpr int K = ltpl_handle::PIPE_SETS;
        const bool two = h->path_streams == 2 && h->path_stream2;
        if (two) {      // the second path stream starts behind everything queued on `stream` so far
            HIP_TRY(h, hipEventRecord(h->ev_begin, h->stream));
            HIP_TRY(h, hipStreamWaitEvent(h->path_stream2, h->ev_begin, 0));
        }
        for (int r = 0; r < reps; ++r) {
            const int set = r % K;
            const TickLayout& T = set ? *h->resident_x[set - 1] : *h->resident;
            hipStream_t sp = (two && (r & 1)) ? h->path_stream2 : h->stream;
            if (r >= K) HIP_TRY(h, hipStreamWaitEvent(sp, h->ev_vel[set], 0));
            if (ms_total) HIP_TRY(h, hipEventRecord(h->ev_step[2 * (size_t)r], sp));
            int rc = tick_launch_paths(h, T, sp);
            if (rc) return rc;
            if (ms_total) HIP_TRY(h, hipEventRecord(h->ev_step[2 * (size_t)r + 1], sp));
            HIP_TRY(h, hipEventRecord(h->ev_paths[set], sp));
            hipStream_t sv = h->vel_stream[r % ltpl_handle::VEL_STREAMS];
            HIP_TRY(h, hipStreamWaitEvent(sv, h->ev_paths[set], 0));
            if ((rc = tick_launch_vel(h, T, sv))) return rc;
            HIP_TRY(h, hipEventRecord(h->ev_vel[set], sv));
            h->last_set = set;
        }
        // everything joins `stream` again (the caller's events / synchronisation are on it)
        for (int i = 0; i < K && i < reps; ++i) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_vel[i], 0));
    } else {
        for (int r = 0; r < reps; ++r) { int rc = tick_launch(h, *h->resident); if (rc) return rc; }
    }
    if (ms_total) {
        HIP_TRY(h, hipEventRecord(e1, h->stream));
        HIP_TRY(h, hipEventSynchronize(e1));
        HIP_TRY(h, hipEventElapsedTime(ms_total, e0, e1));
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        if (h->resident_x[0]) {
            for (int r = 0; r < reps; ++r) {
                float ms = 0.0f;
                HIP_TRY(h, hipEventElapsedTime(&ms, h->ev_step[2 * (size_t)r], h->ev_step[2 * (size_t)r + 1]));
                h->last_paths_ms += ms;
            }
            h->last_paths_n = reps;
        }
    } else {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(h))

extern "C" int ltpl_batch_last_paths_ms(ltpl_handle* h, float* ms_avg)
{
    if (!h || !ms_avg) return LTPL_ERR_INVALID_ARG;
    *ms_avg = h->last_paths_n > 0 ? h->last_paths_ms / (float)h->last_paths_n : 0.0f;
    return LTPL_OK;
}

extern "C" int ltpl_batch_run_profile(ltpl_handle* h, int reps, float* ms_kernels)
try {
    if (!h) return LTPL_ERR_INVALID_ARG;
    if (!h->resident) { h->err = "no resident batch: call ltpl_batch_upload first"; return LTPL_ERR_INVALID_ARG; }
    if (reps < 1 || !ms_kernels) { h->err = "reps < 1 or null output"; return LTPL_ERR_INVALID_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    hipEvent_t ev[4];
    for (int i = 0; i < 4; ++i) HIP_TRY(h, hipEventCreate(&ev[i]));
    ms_kernels[0] = ms_kernels[1] = ms_kernels[2] = 0.0f;
    for (int r = 0; r < reps; ++r) {
        int rc = tick_launch(h, *h->resident, ev);
        if (rc) return rc;
        HIP_TRY(h, hipEventSynchronize(ev[3]));
        for (int k = 0; k < 3; ++k) { float ms = 0.0f; HIP_TRY(h, hipEventElapsedTime(&ms, ev[k], ev[k + 1])); ms_kernels[k] += ms; }
    }
    for (int i = 0; i < 4; ++i) (void)hipEventDestroy(ev[i]);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(h))

extern "C" int ltpl_batch_download(ltpl_handle* h, ltpl_paths_out* out, ltpl_tick_vel_out* vout)
try {
    if (!h) return LTPL_ERR_INVALID_ARG;
    if (!h->resident) { h->err = "no resident batch"; return LTPL_ERR_INVALID_ARG; }
    if (!out || !vout || out->cap_nodes != h->resident->cap_nodes || out->cap_pts != h->resident->cap_pts) {
        h->err = "output capacities differ from ltpl_batch_upload"; return LTPL_ERR_INVALID_ARG;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const void* src = (h->resident_x[0] && h->last_set >= 1) ? h->d_out_x[h->last_set - 1] : h->d_out;
    HIP_TRY(h, hipMemcpyAsync(h->h_out, src, h->resident->out_total, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    tick_scatter(static_cast<const unsigned char*>(h->h_out), *h->resident, out, vout);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(h))

static void free_resident(TickLayout* t) { delete t; }
