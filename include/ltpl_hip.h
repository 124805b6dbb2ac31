/*
 * ltpl_hip.h -- C ABI of libltpl_hip.so, the MI355X (gfx950) backend for the online hot path of graph_ltpl.
 *
 * The reference (TUMFTM/GraphBasedLocalTrajectoryPlanner) is pure Python and has no FFI; the natural seams are two
 * Python call sites that it resolves by fully qualified attribute lookup on every tick:
 *
 *   seam (1)  graph_ltpl/online_graph/src/main_online_path_gen.py:11-21,333-334   main_online_path_gen(...)
 *             called from graph_ltpl/online_graph/src/OnlineTrajectoryHandler.py:416-427
 *   seam (2)  graph_ltpl/online_graph/src/VpForwardBackward.py:11-255             class VpForwardBackward
 *             constructed at OnlineTrajectoryHandler.py:137-144, called at :676, :747-752, :789-798, :872-878, :967-972
 *
 * Every entry point below names the reference interface it replaces. All functions are extern "C", take plain
 * pointers / sizes (C-contiguous float64 / int32 host buffers owned by the caller) and return an int status
 * (LTPL_OK == 0). "No path found" is NOT an error (valid == 0). No C++ exception crosses the ABI. A handle owns its
 * device memory, pinned staging and one HIP stream; calls on one handle are synchronous on return and must not be
 * issued concurrently; different handles may be used from different threads / processes.
 *
 * Environment switches (all read ONCE, at ltpl_create / ltpl_planner_create). Every switch of the RELEASE library selects among
 * code paths that produce identical results (the GPU test-suite runs them); none skips work:
 *   LTPL_NO_FIXED_PLAN=1        batch kernel with the runtime LDS plan instead of a compile-time plan class (any lattice)
 *   LTPL_FORCE_LONG_HORIZON=1   parent tables in global memory (the mode lattices with very long planning ranges get automatically)
 *   LTPL_BATCH_NW=4             four-wave teams also for batches; LTPL_NW1_MIN_SCEN=<n>: smallest batch that uses one-wave teams (64)
 *   LTPL_FORCE_FUSED=1          fused k_tick also for batches; LTPL_NO_OVERLAP=1: resident batches on one stream (no pipelining)
 *   LTPL_NO_SCEN_ORDER=1        batches of >= 2048 scenarios planned in the caller's order instead of sorted by start layer (identical results)
 *   LTPL_FOLLOW_EMIT_MIN_SCEN=<n>  smallest pipeline batch whose follow jobs are finished by the lane kernel instead of k_vel_final (8192)
 *   LTPL_PIPELINE_MIN_SCEN=<n>  smallest tick batch that runs the one-wave pipeline instead of the fused tick kernel (default: more than two
 *                               fused workgroups per compute unit -- 513 on the MI355X, 257 where only one fits; rounds 1-5: 64). Lattices
 *                               whose fused tick (four-wave plan + velocity scratch) needs more than 150 KiB of LDS run the pipeline at
 *                               every batch size, single ticks included: the long-horizon mode and e.g. C5 with a 120 .. 190 m horizon
 *   LTPL_FINAL_Y=<n>            row-chunk blocks per tile of the final velocity kernel (8)
 *   LTPL_ZC_OUT=0 / LTPL_ZC_IN=1   zero-copy outputs (default on) / inputs (default off) of calls with <= 8 scenarios
 *   LTPL_POLL=1 (+ LTPL_POLL_SYNC_EVERY, LTPL_POLL_QUERY)   completion of small calls through a polled word instead of a stream sync
 *   LTPL_NO_SELFTEST=1          skip the create-time self-test (one-wave vs four-wave kernel on probe scenarios)
 *   LTPL_HOST_PROF=1            host-side timing table of the entry points on stderr at exit
 *   LTPL_FLEET_NO_FUSE=1        fleet tape runs with one kernel per stage instead of the fused stage kernels (read by ltpl_fleet_create)
 *   LTPL_FLEET_FOLLOW_WAVES=1/0 fleet follow jobs one WAVE per job / one LANE per job (default: lanes from 12 288 planners on; ltpl_fleet_create)
 *   LTPL_NO_LAYER_GRID=1        closest reference-line layer of an obstacle position by the scan over all layers, no create-time grid
 *   LTPL_PERSISTENT_TICK=1      ltpl_create behaves like ltpl_create_ex(LTPL_CREATE_PERSISTENT_TICK); LTPL_PERSIST_IDLE_MS=<ms>: idle limit (250)
 *   LTPL_TICK_GRAPH=1           the single fused tick (copy in -> kernel [-> copy out]) as ONE hipGraph launch (measured: slower; off)
 *   LTPL_VEL_CUS=<n>            velocity streams of the resident-batch pipeline confined to n compute units by a CU mask (measured: the
 *                               velocity chain becomes the bottleneck below ~128 CUs, no gain above; off)
 * Timing / fault-injection switches (LTPL_ABLATE, LTPL_EXP_SKIP, LTPL_LDS_POISON, LTPL_SCRATCH_POISON, LTPL_DEBUG_TIMING,
 * LTPL_DEBUG_OCC) skip work, overwrite memory or instrument kernels; they are compiled into the EXPERIMENT build only
 * (-DLTPL_EXPERIMENT -> libltpl_hip_exp.so, used by tools/ and one fault-injection test) and do not exist in libltpl_hip.so.
 * The experiment build also exports the check entry points of tests/test_gpu_wave_ops.py (host arrays in, one launch, host arrays out):
 * ltpl_exp_wave_ops_check, ltpl_exp_heading_atan2, ltpl_exp_heading_sincos, ltpl_exp_fast_rcp, ltpl_exp_rsqrt_cubed -- the device
 * helpers of csrc/paths_team.hpp applied to caller-provided values -- and ltpl_exp_project of tests/test_gpu_projection.py: the device's
 * projections of a point on a polyline (get_s_coord_dev, globrl_index_dev, lane_globrl_index, project_on_polyline of csrc/fleet_core.hpp)
 * for caller-provided queries on a caller-provided polyline.
 */
#ifndef LTPL_HIP_H
#define LTPL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LTPL_ABI_VERSION 9        /* v7 (round 5, additive): ltpl_paths_kernel_symbol, ltpl_layer_grid, ltpl_fleet_digest; v8 (additive): ltpl_assembly_records;
                                     v9 (round 6, additive): ltpl_create_ex, ltpl_tick_persistent_stop / _stats;
                                     additive to v9: ltpl_fleet_sim_race / _heading, ltpl_fleet_friction / _scale / _rows,
                                     ltpl_fleet_sim_snapshot / _snapshot_info / _snapshot_drop / _branch,
                                     ltpl_fleet_sim_noise / _estimate / _noise_draws,
                                     ltpl_fleet_sim_vehicle / _vehicle_read / _vehicle_step,
                                     ltpl_fleet_sim_sensor / _sensor_read / _sensor_eval,
                                     ltpl_fleet_sim_tracker / _tracker_read / _tracker_eval,
                                     ltpl_fleet_sim_predictor / _predictor_read / _predictor_eval,
                                     ltpl_fleet_sim_selector / _selector_read / _selector_eval,
                                     ltpl_fleet_sim_safety / _safety_read / _safety_eval,
                                     ltpl_fleet_sim_react / _react_read / _react_eval,
                                     ltpl_fleet_sim_stats / _stats_reduce / _stats_series / _stats_eval */

/* status codes */
#define LTPL_OK               0
#define LTPL_ERR_INVALID_ARG  1
#define LTPL_ERR_NO_DEVICE    2
#define LTPL_ERR_HIP          3
#define LTPL_ERR_CAPACITY     4
#define LTPL_ERR_UNSUPPORTED  5
#define LTPL_ERR_EXCEPTION    6    /* a C++ exception (out of host memory, ...) was caught at the ABI; message in ltpl_last_error */

/* action primitives: ACTION_ID_MAP, OnlineTrajectoryHandler.py:14-17 */
#define LTPL_ACT_STRAIGHT 0
#define LTPL_ACT_FOLLOW   1
#define LTPL_ACT_LEFT     2
#define LTPL_ACT_RIGHT    3
#define LTPL_ACT_NONE    (-1)
#define LTPL_ACT_EMERGENCY 4   /* key 'emergency' of the exported trajectory set (OnlineTrajectoryHandler.py:1028-1034) */

#define LTPL_MAX_ACTIONS     3   /* at most 3 primitives are offered per tick (main_online_path_gen.py:128-174) */
#define LTPL_MAX_LAST_NODES  8   /* nodes of the previous solution used for the cost discount (w_last_edges)      */

/* per-scenario flag bits of ltpl_paths_in.flags */
#define LTPL_FLAG_ACTION_SETS     1   /* action_sets=True                    main_online_path_gen.py:15          */
#define LTPL_FLAG_OBJ_IN_CONST    2   /* obj_in_const_path                   main_online_path_gen.py:77,118-122  */
#define LTPL_FLAG_OBJ_BESIDES     4   /* object_besides_const_path           main_online_path_gen.py:78,104-105  */
#define LTPL_FLAG_HAS_PSI_S       8   /* const_path_seg is not None -> psi_s main_online_path_gen.py:300-303     */

typedef struct ltpl_handle ltpl_handle;

/* ------------------------------------------------------------------------------------------------------------------
 * Offline lattice, struct-of-arrays (what GraphBase holds in igraph attributes: GraphBase.py:93-119,163-194,409-439).
 * Node global id = layer_node_off[layer] + node. Edges are stored CSC by destination node, in-edges sorted by source
 * node id; an edge always connects layer l to layer (l+1) mod num_layers (gen_edges.py:52-61).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t num_layers;
    int32_t num_nodes;
    int32_t num_edges;
    int32_t num_samples;
    int32_t num_glob_rl;            /* rows of glob_rl                                                            */
    int32_t closed;                 /* GraphBase.closed; 0 = open track (planning range clamped to the last layer)   */
    int32_t plan_horizon_mode;      /* 0 = 'distance', 1 = 'layers'        gen_local_node_template.py:104-133     */
    int32_t reserved0;
    double  min_plan_horizon;
    double  lat_resolution;
    double  lat_offset;
    double  veh_width;
    double  veh_length;
    double  sampled_resolution;
    double  vel_decrease_lat;
    /* per layer [num_layers] */
    const int32_t* layer_node_off;  /* [num_layers + 1]                                                           */
    const int32_t* raceline_index;
    const double*  s_raceline;
    const double*  refline_x;
    const double*  refline_y;
    const double*  vel_raceline;
    /* per node [num_nodes] */
    const double*  node_x;
    const double*  node_y;
    const double*  vgoal_cost;      /* cost of the virtual goal edge of that node              GraphBase.py:188   */
    /* per edge [num_edges] */
    const int32_t* in_ptr;          /* [num_nodes + 1]                                                            */
    const int32_t* edge_src;        /* source node index inside the previous layer                                */
    const double*  edge_cost;       /* offline_cost                                                               */
    const double*  edge_len;        /* spline_length                                                              */
    const int32_t* samp_ptr;        /* [num_edges + 1]                                                            */
    /* per sample [num_samples]: columns 0,1,2,4 of spline_param (GraphBase.py:425-436); kappa (col 3) is never read
     * online because main_online_path_gen.py:318-322 overwrites it                                               */
    const double*  samp_x;
    const double*  samp_y;
    const double*  samp_psi;
    const double*  samp_len;
    /* fine global race line, row-major [num_glob_rl][5] = s, x, y, kappa, vel    (GraphBase.glob_rl)             */
    const double*  glob_rl;
    /* track bounds per layer (ObjectListInterface.set_track_data, ObjectListInterface.py:49-73; fed from GraphBase at
     * Graph_LTPL.py:232-235): bound1 = refline + normvec * width_right, bound2 = refline - normvec * width_left       */
    const double*  normvec_x;       /* [num_layers]                                                               */
    const double*  normvec_y;
    const double*  width_right;
    const double*  width_left;
    /* ABI v3, only read by the planner entry points (ltpl_planner_*); may be NULL otherwise:
     * race line point per layer (GraphBase.raceline, main_online_path_gen.py:86-101) and heading per node
     * (vertex attribute psi, GraphBase.py:163-168; OnlineTrajectoryHandler.py:232-246)                              */
    const double*  raceline_x;      /* [num_layers]                                                               */
    const double*  raceline_y;
    const double*  node_psi;        /* [num_nodes]                                                                */
} ltpl_lattice_desc;

typedef struct {
    int32_t max_path_nodes;         /* capacity needed per path: nodes                                            */
    int32_t max_path_pts;           /* capacity needed per path: samples                                          */
    int32_t max_horizon_edges;
    int32_t device;
    int32_t num_cus;
    int32_t lds_bytes_paths;        /* dynamic LDS of the path kernel                                             */
} ltpl_caps;

/* ------------------------------------------------------------------------------------------------------------------
 * seam (1): batched main_online_path_gen. One "scenario" = one call of the reference function.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n_scen;
    int32_t n_w_last;               /* len(w_last_edges)                                                          */
    const double*  w_last_edges;    /* [n_w_last]  online cost factors     gen_local_node_template.py:155-162     */
    const int32_t* start_layer;     /* [n_scen]                                                                   */
    const int32_t* start_node;      /* [n_scen]                                                                   */
    const int32_t* flags;           /* [n_scen]  LTPL_FLAG_*                                                      */
    const int32_t* last_action;     /* [n_scen]  LTPL_ACT_* of last_action_id or LTPL_ACT_NONE                    */
    const int32_t* const_closest;   /* [n_scen]  object index chosen by the constant-segment test
                                                 (main_online_path_gen.py:97-115) or -1                           */
    const double*  psi_s;           /* [n_scen]  const_path_seg[-1, 2] when LTPL_FLAG_HAS_PSI_S                   */
    /* vehicles: vehicle k of scenario s is v = veh_off[s] + k; its positions are pos_off[v] .. pos_off[v+1]-1,
     * the first one being VehObject.get_pos(), the others VehObject.get_prediction() rows
     * (gen_local_node_template.py:169-189)                                                                       */
    const int32_t* veh_off;         /* [n_scen + 1]                                                               */
    const int32_t* pos_off;         /* [n_veh_total + 1]                                                          */
    const double*  veh_radius;      /* [n_veh_total]                                                              */
    const double*  pos_x;           /* [n_pos_total]                                                              */
    const double*  pos_y;           /* [n_pos_total]                                                              */
    /* zone-blocked nodes ("overtaking_zones" filter, gen_local_node_template.py:96): global node ids             */
    const int32_t* zone_off;        /* [n_scen + 1]                                                               */
    const int32_t* zone_gid;        /* [n_zone_total]                                                             */
    /* previous solution (last_solution_nodes): n_last[s] <= LTPL_MAX_LAST_NODES leading nodes                    */
    const int32_t* n_last;          /* [n_scen]                                                                   */
    const int32_t* last_layer;      /* [n_scen * LTPL_MAX_LAST_NODES]                                             */
    const int32_t* last_node;       /* [n_scen * LTPL_MAX_LAST_NODES]                                             */
} ltpl_paths_in;

typedef struct {
    int32_t cap_nodes;              /* caller-chosen capacities, >= ltpl_caps.max_path_nodes / max_path_pts       */
    int32_t cap_pts;
    /* per scenario */
    int32_t* end_layer;             /* [n_scen]                                                                   */
    int32_t* closest_obj_index;     /* [n_scen]     -1 = None                                                     */
    int32_t* closest_obj_node;      /* [n_scen * 2] layer, node; -1 = None                                        */
    int32_t* n_actions;             /* [n_scen]     number of action slots used (template length)                 */
    /* per scenario and action slot a < LTPL_MAX_ACTIONS, index s * LTPL_MAX_ACTIONS + a; slots are in the order the
     * reference inserts its dict keys (follow / straight first)                                                  */
    int32_t* action_id;             /* final name (after the follow -> straight rename, :232-237) or NONE         */
    int32_t* valid;                 /* 1 = key present in the reference's dicts                                   */
    int32_t* reduced;               /* action_set_red_len                                                         */
    int32_t* goal_layer;            /* layer the path ends in                                                     */
    int32_t* n_nodes;               /* entries of nodes / node_idx / coeff behind n_nodes and rows of path_param (and of vx / ax of the
                                     * tick outputs) behind n_pts are UNSPECIFIED padding, as are slots a >= n_actions and invalid slots */
    int32_t* n_pts;
    int32_t* n_ties;                /* exact cost ties met while picking predecessors along this sweep            */
    int32_t* nodes;                 /* [.. * cap_nodes]      node index per layer, layer i = (start + i) mod L    */
    int32_t* node_idx;              /* [.. * cap_nodes]      row of every node in path_param                      */
    double*  coeff;                 /* [.. * cap_nodes * 8]  (n_nodes-1) rows [x a0..a3, y a0..a3]                */
    double*  path_param;            /* [.. * cap_pts * 5]    n_pts rows [x, y, psi, kappa, el_length]             */
} ltpl_paths_out;

/* ------------------------------------------------------------------------------------------------------------------
 * seam (2): the arithmetic behind class VpForwardBackward.
 * ------------------------------------------------------------------------------------------------------------------ */
#define LTPL_VEL_FB      0   /* VpForwardBackward.calc_vel_profile  :194-227 -> tph.calc_vel_profile(closed=False) */
#define LTPL_VEL_BRAKE   1   /* tph.calc_vel_profile_brake behind check_brake_prefix :115-122, calc_vel_brake_em  */
#define LTPL_VEL_FOLLOW  2   /* VpForwardBackward.calc_vel_profile_follow :141-192 -> calc_vel_profile_follow.py  */
#define LTPL_VEL_FOLLOW_CONTROLLED 3   /* the same without the final intersection with the unconstrained profile
                                          (calc_vel_profile_follow.py:78-294 only): a caller that wants the two independent halves of
                                          the follow mode in parallel submits this job + an LTPL_VEL_FB job without v_end and takes
                                          the element-wise minimum (:297-310) itself                                          */

typedef struct {
    double  dyn_model_exp;          /* VpForwardBackward.__init__ :22-29                                          */
    double  drag_coeff;
    double  m_veh;
    double  len_veh;
    double  v_max;                  /* update_dyn_parameters :65-84                                               */
    int32_t n_ax_max_machines;
    int32_t follow_control_type;    /* 0 = 'PD', 1 = 'PDtan'          calc_vel_profile_follow.py:65-75            */
    const double* ax_max_machines;  /* [n_ax_max_machines * 2] rows [v, ax]                                       */
    double  c_p, k_p, k_d, tan_w;   /* follow controller parameters   params/ltpl_config_online.ini:41-50         */
} ltpl_vel_params;

typedef struct {
    int32_t mode;                   /* LTPL_VEL_*                                                                 */
    int32_t n;                      /* kappa.size                                                                 */
    int32_t n_el;                   /* el_lengths.size: n-1 (FB, BRAKE) or n (FOLLOW, OTH.py:791 hands over n)    */
    int32_t has_v_end;
    const double* kappa;            /* [n]                                                                        */
    const double* el_lengths;       /* [n_el]                                                                     */
    const double* loc_gg;           /* [n * 2] rows [ax_max, ay_max], gg_scale already applied                    */
    double  v_start;
    double  v_end;
    /* FOLLOW only (calc_vel_profile_follow.py:78-95) */
    double  v_ego, v_obj, safety_d, obj_dist, obj_x, obj_y;
} ltpl_vel_job;

typedef struct {
    double*  vx;                    /* [n] output profile                                                         */
    int32_t  too_close;             /* FOLLOW: calc_vel_profile_follow.py:146-149                                 */
    int32_t  vel_bound;             /* FOLLOW: vel_bound_fulfilled                                                */
} ltpl_vel_result;

/* ------------------------------------------------------------------------------------------------------------------
 * fused tick: seam (1) followed by the per-primitive velocity stage of OnlineTrajectoryHandler.calc_vel_profile
 * (OTH.py:688-941) on the freshly planned paths (no constant prefix: cut_index_pos = 0, vel_course empty).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
    const ltpl_vel_params* params;
    double  gg_ax, gg_ay;           /* constant local gg (ax, ay) times gg_scale   OTH.py:651-666                 */
    double  gg_brake_scale;         /* old_gg_scale / gg_scale used by the brake prefix  VpForwardBackward.py:114 */
    double  safety_d;
    double  v_max_offset;           /* ACTIONSET.v_max_offset                      OTH.py:102,907                 */
    const double* vel_plan;         /* [n_scen]                                                                   */
    const double* vel_est;          /* [n_scen]                                                                   */
    const double* pos_est_x;        /* [n_scen]                                                                   */
    const double* pos_est_y;        /* [n_scen]                                                                   */
    const double* veh_vel;          /* [n_veh_total] VehObject.get_vel()                                          */
} ltpl_tick_vel_in;

typedef struct {
    double*  vx;                    /* [n_scen * LTPL_MAX_ACTIONS * cap_pts]                                      */
    double*  ax;                    /* [n_scen * LTPL_MAX_ACTIONS * cap_pts]                                      */
    int32_t* vel_bound;             /* [n_scen * LTPL_MAX_ACTIONS]                                                */
    int32_t* too_close;             /* [n_scen * LTPL_MAX_ACTIONS]                                                */
} ltpl_tick_vel_out;

/* ------------------------------------------------------------------------------------------------------------------
 * object ingestion: the arithmetic of ObjectListInterface.process_object_list
 * (ObjectListInterface.py:75-153) for objects of type "physical": on-track test check_inside_bounds
 * (check_inside_bounds.py:7-59), constant-velocity prediction over dt (:117-127, dt = 0.2 s) and radius = length / 2 (:133).
 * One flat list of objects (the caller concatenates the objects of all scenarios).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n_obj;
    int32_t reserved0;
    double  dt;                     /* prediction horizon, 0.2 in the reference                                  */
    const double* x;                /* [n_obj] object_el['X']                                                     */
    const double* y;                /* [n_obj] object_el['Y']                                                     */
    const double* theta;            /* [n_obj] heading, 0 = north                                                 */
    const double* v;                /* [n_obj]                                                                    */
    const double* length;           /* [n_obj]                                                                    */
} ltpl_objects_in;

typedef struct {
    int32_t* on_track;              /* [n_obj] 1 = inside the track bounds                                        */
    double*  pred_x;                /* [n_obj] X - sin(theta) v dt                                                */
    double*  pred_y;                /* [n_obj] Y + cos(theta) v dt                                                */
    double*  radius;                /* [n_obj] length / 2                                                         */
} ltpl_objects_out;

/* --- lifecycle ---------------------------------------------------------------------------------------------------- */
/* Uploads the lattice to HBM once (replaces the pickled GraphBase handed to OnlineTrajectoryHandler,
 * Graph_LTPL.py:202-229). device < 0 selects the current device. */
int ltpl_create(const ltpl_lattice_desc* lattice, int device, ltpl_handle** out_handle);
/* v9: the same with flags. LTPL_CREATE_PERSISTENT_TICK: single-scenario ltpl_tick_batch calls are served by a RESIDENT kernel (one
 * workgroup, started at the first such call) that receives every tick through a mailbox in page-locked memory instead of being launched
 * per tick -- the latency form for the reference's own use, one car and one tick at a time inside its 0.1 s budget
 * (OnlineTrajectoryHandler.py:353-366). Results are bit-identical to the launched form (same device code). Engaged for lattices whose
 * single-tick kernel has a compile-time LDS plan (ltpl_persistent_stats.enabled tells); otherwise the call behaves like ltpl_create.
 * A resident kernel never completes, so device-wide synchronisations of the process (hipDeviceSynchronize, hipFree) wait for it: every
 * other entry point of the handle stops it first, ltpl_tick_persistent_stop does so on request, and it leaves by itself after
 * LTPL_PERSIST_IDLE_MS (250) ms without a tick -- the next tick starts it again. Environment: LTPL_PERSISTENT_TICK=1 sets the flag for
 * ltpl_create. */
#define LTPL_CREATE_PERSISTENT_TICK 1u
int ltpl_create_ex(const ltpl_lattice_desc* lattice, int device, uint32_t flags, ltpl_handle** out_handle);
typedef struct {
    int32_t enabled;                /* 1: single ticks of this handle go through the resident kernel                         */
    int32_t resident;               /* 1: the kernel is resident right now                                                    */
    int64_t ticks;                  /* ticks served through the mailbox                                                       */
    int64_t launches;               /* kernel starts (first tick, after idling out, after another entry point stopped it)     */
    double  device_us_mean;         /* device-side time per tick: "sequence number seen" .. "outputs fenced out", mean / last */
    double  device_us_last;
    double  idle_ms;                /* idle limit in force                                                                    */
} ltpl_persistent_stats;
int ltpl_tick_persistent_stop(ltpl_handle* handle);       /* the resident kernel leaves now (no-op when none is resident)           */
int ltpl_tick_persistent_stats(ltpl_handle* handle, ltpl_persistent_stats* stats);
int ltpl_destroy(ltpl_handle* handle);
int ltpl_get_caps(const ltpl_handle* handle, ltpl_caps* caps);
const char* ltpl_last_error(const ltpl_handle* handle);   /* NULL handle -> last create() error */
int ltpl_version(void);
/* diagnostics: symbol-name prefix (Itanium mangling) of the path kernel this handle launches for batches (team_waves = 1) or single
 * ticks (team_waves = 4) -- the LDS plan class is chosen per lattice at ltpl_create. Profiles under profiles/ carry a digest of that
 * kernel's instruction stream; bench.py uses this to check that a committed counter pass describes the library it runs. */
const char* ltpl_paths_kernel_symbol(const ltpl_handle* handle, int32_t team_waves);

/* --- seam (1): main_online_path_gen.py:11 ------------------------------------------------------------------------- */
int ltpl_plan_paths(ltpl_handle* handle, const ltpl_paths_in* in, ltpl_paths_out* out);

/* --- diagnostics of seam (1): the same call with the obstacle x edge mask exported (GraphBase.get_intersec_edges_in_range,
 *     GraphBase.py:567-646; the set of edges gen_local_node_template.py:164-203 deletes from the "default" filter) exactly as the
 *     path kernel computed it in its LDS bitmap: blocked[s * num_edges + e] = 1 if edge e (global id) is blocked in scenario s.
 *     The kernel tests every edge of an obstacle's 3-layer window that lies in the planning range, whether or not its end nodes
 *     are removed by the zone filter (the reference only tests edges of the active "planning_range" filter; edges at removed
 *     nodes cannot be used either way). team_waves: 0 = the form ltpl_plan_paths would choose for n_scen, 1 = one-wave batch
 *     kernel, 4 = four-wave latency kernel. tests/test_edge_mask.py compares the bitmap with the oracle's bit for bit. ------- */
int ltpl_plan_paths_mask(ltpl_handle* handle, const ltpl_paths_in* in, ltpl_paths_out* out, int32_t team_waves, uint8_t* blocked);

/* --- constant-segment test in front of seam (1): main_online_path_gen.py:76-122 (host side, O(#objects) projections on the
 *     race line). seg = rows [x, y, psi, kappa, el] of const_path_seg (n_rows may be 0), pos_est = 2 doubles or NULL;
 *     flags_out receives LTPL_FLAG_OBJ_IN_CONST | LTPL_FLAG_OBJ_BESIDES bits, closest_out the object index or -1 ---------- */
int ltpl_const_segment_test(const ltpl_handle* handle, const double* seg, int32_t n_rows, const double* pos_est, int32_t n_veh,
                            const double* veh_x, const double* veh_y, const double* veh_radius, int32_t* flags_out,
                            int32_t* closest_out);

/* --- global s coordinate of a position on the race line: get_s_coord(ref_line=raceline, s_array=s_raceline, closed=True)
 *     (get_s_coord.py:8-99; call sites Graph_LTPL.py:436-440 for the log row, main_online_path_gen.py:86-101) ------------- */
int ltpl_raceline_s(const ltpl_handle* handle, double x, double y, double* s_out);

/* --- diagnostics (host only, no device needed): the per-edge capsule table ltpl_create derives for the obstacle mask
 *     (GraphBase.get_intersec_edges_in_range, GraphBase.py:567-646). The path kernel decides "no sample of the edge is within
 *     the obstacle's threshold" / "some sample is" from it without reading the samples whenever either is certain, and runs the
 *     reference's exact sample test otherwise. capsules_out: 8 floats per edge (Ax, Ay, ABx, ABy, 1 / |AB|^2, dev, (gap / 2)^2,
 *     packed sample range); slack_out: the fp32 rounding bound added to both decisions. tests/test_capsule_cull.py checks the
 *     conservativeness of the decisions against the exact test on the real lattices. ------------------------------------- */
int ltpl_edge_capsules(int32_t n_edges, const int32_t* samp_ptr, const double* samp_x, const double* samp_y, int32_t n_samples,
                       float* capsules_out, float* slack_out);

/* --- diagnostics (host only, no device needed): the closest-layer grid ltpl_create derives for the path kernel's first phase (closest
 *     reference-line layer of an obstacle position = np.argmin over all layers, get_intersec_edges.py:40-51). Per grid cell the at most two
 *     intervals of layers that can be closest to any point of the cell; the kernel evaluates the reference's exact distances on those and on
 *     all layers for positions outside the grid / in cells marked "full scan". origin_cell: x0, y0, 1 / cell size; dims: nx, ny; cells (may
 *     be NULL to query the dimensions first): 4 ints per cell, row-major in y: first layer and length of interval 1 and 2, length -1 = full
 *     scan. tests/test_layer_grid.py checks against the brute-force argmin that the true answer is always among the candidates. --------- */
int ltpl_layer_grid(int32_t n_layers, const double* ref_x, const double* ref_y, double* origin_cell, int32_t* dims, int32_t* cells,
                    int32_t cap_cells);

/* --- diagnostics (host only, no device needed): the per-node / per-edge records ltpl_create derives for the path assembly
 *     (main_online_path_gen.py:260-328: the nodes of a path -> its edges -> the spline samples' coordinates and end headings). node_rec_out:
 *     4 ints per node = first in-edge (CSC id) + the source nodes of its first 12 in-edges as bytes (0xff = none); edge_rec_out: 10 doubles
 *     per edge = first sample | #samples << 32 (bit pattern), edge length, x, y of the first and of the last sample, sin, cos of the first
 *     and of the last sample's heading. tests/test_assembly_records.py checks them against the lattice arrays they replace. ----------- */
int ltpl_assembly_records(int32_t n_nodes, int32_t n_edges, const int32_t* in_ptr, const int32_t* edge_src, const double* edge_len,
                          const int32_t* samp_ptr, const double* samp_x, const double* samp_y, const double* samp_psi,
                          int32_t* node_rec_out, double* edge_rec_out);

/* --- object ingestion: ObjectListInterface.py:75-153, check_inside_bounds.py:7-59 --------------------------------- */
int ltpl_process_objects(ltpl_handle* handle, const ltpl_objects_in* in, ltpl_objects_out* out);

/* --- seam (2): VpForwardBackward.py:86,141,194,229 ---------------------------------------------------------------- */
int ltpl_vel_profile(ltpl_handle* handle, const ltpl_vel_params* params, int n_jobs, const ltpl_vel_job* jobs,
                     ltpl_vel_result* results);

/* --- fused tick (throughput path): Graph_LTPL.calc_paths + calc_vel_profile arithmetic, Graph_LTPL.py:300,344 ------ */
int ltpl_tick_batch(ltpl_handle* handle, const ltpl_paths_in* in, const ltpl_tick_vel_in* vin,
                    ltpl_paths_out* out, ltpl_tick_vel_out* vout);

/* Compact result form of ltpl_tick_batch for callers that only need what Graph_LTPL.calc_vel_profile hands out (the
 * trajectory set, Graph_LTPL.py:396-408): rows [s, x, y, psi, kappa, vx, ax] of every valid action slot, trimmed to max_rows
 * (EXPORT.nmbr_export_points) and packed back to back on the DEVICE, so that only the bytes in use cross PCIe (the capacity
 * slabs of ltpl_paths_out / ltpl_tick_vel_out are mostly padding). `rows` may be any host memory; memory from ltpl_host_alloc
 * (page-locked) is written by DMA directly, other memory goes through the handle's staging buffer. */
typedef struct {
    int32_t  max_rows;              /* rows kept per trajectory, 0 = all                                          */
    int32_t  reserved0;
    int64_t  capacity_rows;         /* capacity of `rows` in rows of 7 doubles                                    */
    /* per scenario and action slot, index s * LTPL_MAX_ACTIONS + a */
    int32_t* action_id;             /* LTPL_ACT_* or LTPL_ACT_NONE                                                */
    int32_t* n_rows;                /* 0 = no trajectory in this slot                                             */
    int32_t* vel_bound;             /* OTH.py:906-911                                                             */
    int32_t* reduced;               /* action_set_red_len                                                         */
    int64_t* row_off;               /* first row of the slot in `rows`                                            */
    double*  rows;                  /* [total_rows * 7]                                                           */
    int64_t  total_rows;            /* out                                                                        */
} ltpl_traj_out;
int ltpl_tick_batch_compact(ltpl_handle* handle, const ltpl_paths_in* in, const ltpl_tick_vel_in* vin, ltpl_traj_out* out);
void* ltpl_host_alloc(size_t bytes);      /* page-locked host memory for ltpl_traj_out.rows; NULL on failure      */
void  ltpl_host_free(void* p);

/* Device-resident variant for benchmarks: upload the batch once, replay the fused kernel, download on demand.
 * The resident batch lives in the handle's staging buffers: ANY other entry point on the same handle (ltpl_plan_paths,
 * ltpl_tick_batch, ltpl_vel_profile, ltpl_process_objects, the planner calls) drops it, after which ltpl_batch_run /
 * ltpl_batch_download return LTPL_ERR_INVALID_ARG ("no resident batch") until the next ltpl_batch_upload.
 * ltpl_batch_run enqueues `reps` launches on the handle's stream and, when ms_total != NULL, brackets them with HIP
 * events on that stream and waits. */
int ltpl_batch_upload(ltpl_handle* handle, const ltpl_paths_in* in, const ltpl_tick_vel_in* vin,
                      int32_t cap_nodes, int32_t cap_pts);
int ltpl_batch_run(ltpl_handle* handle, int reps, float* ms_total);
int ltpl_batch_download(ltpl_handle* handle, ltpl_paths_out* out, ltpl_tick_vel_out* vout);
/* Profiling variant of ltpl_batch_run: HIP events between the kernels of the pipeline on the handle's stream.
 * ms_kernels[3] = summed durations over `reps` of {path kernel, follow preparation, velocity lane kernel}. */
int ltpl_batch_run_profile(ltpl_handle* handle, int reps, float* ms_kernels);
/* Average duration (ms) of the path kernel inside the last timed ltpl_batch_run, measured with HIP events recorded around
 * every launch of it on the handle's stream, i.e. under the same overlap with the velocity kernels as the timed region. */
int ltpl_batch_last_paths_ms(ltpl_handle* handle, float* ms_avg);

/* ------------------------------------------------------------------------------------------------------------------
 * Offline lattice build: the per-edge arithmetic of gen_edges.py:11-164 (two-point cubic from node
 * pose to node pose, arc-length sampling tph.interp_splines(stepsize_approx), heading / curvature tph.calc_head_curv_an,
 * turn-radius / velocity filter :127-140), of GraphBase.update_edge (element lengths, spline length, GraphBase.py:421-436) and
 * the curvature terms of gen_offline_cost.py:57-62 for ALL candidate edges of a track in one launch (lane = edge). Needs no
 * lattice handle. The host side (node skeleton, pruning, assembly) is graphbasedlocaltrajectoryplanner_amd/offline_build.py.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n_edges;
    int32_t cap_samples;            /* capacity per edge of ltpl_offline_edges_out.samples                        */
    double  stepsize_approx;        /* SAMPLING.stepsize_approx                                                   */
    double  kappa_max_turn;         /* 1 / VEHICLE.veh_turn                                                       */
    const double*  start_x;         /* [n_edges] pose of the start node                                           */
    const double*  start_y;
    const double*  start_psi;
    const double*  end_x;           /* [n_edges] pose of the end node                                             */
    const double*  end_y;
    const double*  end_psi;
    const double*  kappa_max_vel;   /* [n_edges] 10 / (vel_raceline[start layer] * min_vel_race)^2   gen_edges.py:131-132 */
    const int32_t* raceline_edge;   /* [n_edges] 1: race line node -> race line node: coefficients are GIVEN (closed spline
                                                 through the race line, gen_edges.py:40-42,75-78) and the filter does not apply */
    const double*  given_coeff;     /* [n_edges * 8] x a0..a3, y a0..a3 (only read where raceline_edge != 0)      */
} ltpl_offline_edges_in;

/* n_samples is reported for every edge. An edge that does not fit (n_samples > cap_samples) and an edge whose nodes coincide
 * (n_samples < 2: its 15-point length is 0) get valid = 0 and length = kappa_avg = kappa_range = 0; their coefficients are written.
 * Of `samples`, rows [0, n_samples) of an edge that fits are written, the element length of row n_samples - 1 being 0. Rows at and
 * beyond n_samples, and ALL rows of an edge that did not fit or has n_samples < 2, are unspecified (not cleared). */
typedef struct {
    int32_t* n_samples;             /* [n_edges]  (> cap_samples: the edge did not fit, samples not written)      */
    int32_t* valid;                 /* [n_edges]  1 = kept by the curvature filter                                */
    double*  coeff;                 /* [n_edges * 8]                                                              */
    double*  length;                /* [n_edges]  spline_length = sum of the element lengths                      */
    double*  kappa_avg;             /* [n_edges]  sum |kappa| / n_samples                  gen_offline_cost.py:57 */
    double*  kappa_range;           /* [n_edges]  |max kappa - min kappa|                  gen_offline_cost.py:61 */
    double*  samples;               /* [n_edges * cap_samples * 5] rows x, y, psi, kappa, el_length               */
} ltpl_offline_edges_out;

int ltpl_offline_edges(int device, const ltpl_offline_edges_in* in, ltpl_offline_edges_out* out);

/* ------------------------------------------------------------------------------------------------------------------
 * ABI v3 -- the planner: the iterative memory of class OnlineTrajectoryHandler
 * (graph_ltpl/online_graph/src/OnlineTrajectoryHandler.py:24-1040) behind the C ABI, batched over n_scen independent
 * planners that share one lattice handle (section 8f rank 2). One tick =
 *   ltpl_planner_calc_paths        Graph_LTPL.calc_paths        (Graph_LTPL.py:300-340) = OTH.update_objects + OTH.calc_paths
 *   ltpl_planner_calc_vel_profile  Graph_LTPL.calc_vel_profile  (Graph_LTPL.py:344-408) = OTH.get_ref_idx + OTH.calc_vel_profile
 * Object ingestion in front of it is ltpl_process_objects; zone bookkeeping (ObjectListInterface.update_zone) stays with
 * the caller, who passes the node ids the "overtaking_zones" filter currently removes (as for ltpl_plan_paths).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct ltpl_planner ltpl_planner;

#define LTPL_PLANNER_MAX_KEYS 4     /* <= 3 primitives per tick + 'emergency' */

typedef struct {
    int32_t n_scen;
    int32_t n_w_last;               /* COST.w_last_edges                 OTH.py:109                               */
    const double* w_last_edges;
    double  v_max_offset;           /* ACTIONSET.v_max_offset            OTH.py:102                               */
    double  delaycomp;              /* DELAY.delaycomp                   OTH.py:117                               */
    double  calc_time_safety;       /* CALC_TIME.calc_time_safety        OTH.py:121                               */
    int32_t calc_time_buffer_len;   /* CALC_TIME.calc_time_buffer_len    OTH.py:122   (1 .. 16; reference default 5)  */
    int32_t filt_window_width;      /* SMOOTHING.filt_window_width       OTH.py:107 (only 1 is supported)         */
    double  dyn_model_exp, drag_coeff, m_veh;          /* OTH.__init__ arguments -> VpForwardBackward (OTH.py:137-144) */
    int32_t follow_control_type;    /* 0 = 'PD', 1 = 'PDtan'             OTH.py:112-114                           */
    int32_t reserved0;
    double  c_p, k_p, k_d, tan_w;
} ltpl_planner_config;

typedef struct {
    const int32_t* prev_action;     /* [n_scen] LTPL_ACT_* incl. LTPL_ACT_EMERGENCY: prev_action_id (Graph_LTPL.py:300)   */
    const double*  t_now;           /* [n_scen] the caller's time.time() (OTH.py:353-354,395)                     */
    /* objects of the tick (output of ObjectListInterface.process_object_list): same layout as ltpl_paths_in        */
    const int32_t* veh_off;         /* [n_scen + 1]                                                               */
    const int32_t* pos_off;         /* [n_veh_total + 1]                                                          */
    const double*  veh_radius;      /* [n_veh_total]                                                              */
    const double*  veh_vel;         /* [n_veh_total] VehObject.get_vel()                                          */
    const double*  pos_x;           /* [n_pos_total] own position first, then the prediction                      */
    const double*  pos_y;
    const int32_t* zone_off;        /* [n_scen + 1]                                                               */
    const int32_t* zone_gid;        /* [n_zone_total] global node ids removed by the "overtaking_zones" filter    */
} ltpl_planner_paths_in;

typedef struct {                    /* arguments of Graph_LTPL.calc_vel_profile (Graph_LTPL.py:344-351)           */
    const double*  pos_est_x;       /* [n_scen]                                                                   */
    const double*  pos_est_y;
    const double*  vel_est;
    const double*  vel_max;         /* [n_scen] one value per planner (ABI v6; ltpl_planner_* groups its velocity jobs per car), > 0                 */
    const double*  gg_scale;
    const double*  gg_ax;           /* [n_scen] constant local_gg tuple (ax, ay)                                  */
    const double*  gg_ay;
    const double*  safety_d;
    const int32_t* incl_emerg_traj; /* [n_scen]                                                                   */
    int32_t n_ax_max_machines;      /* rows of ax_max_machines (all tables together)                              */
    int32_t n_ax_tables;            /* ABI v6: 0 or 1 = ONE machine table for every planner of the call (was reserved0)            */
    const double*  ax_max_machines; /* [n_ax_max_machines * 2] rows [v, ax]                                       */
    /* ABI v4 -- LOCATION DEPENDENT FRICTION, local_gg as a dict {action id: [rows x (ax, ay)]} (OnlineTrajectoryHandler.py:649-666;
     * Graph_LTPL.py:360-365). Both NULL: constant friction (gg_ax / gg_ay). Otherwise rows gg_row_off[s * LTPL_PLANNER_MAX_KEYS + k]
     * .. gg_row_off[s * LTPL_PLANNER_MAX_KEYS + k + 1] of gg_rows belong to planner s and its k-th path key (key order of
     * ltpl_planner_paths_view); a key's row count must equal n_rows of that path (every path coordinate is represented by a row),
     * a key with zero rows falls back to (gg_ax, gg_ay)                                                            */
    const int32_t* gg_row_off;      /* [n_scen * LTPL_PLANNER_MAX_KEYS + 1]                                       */
    const double*  gg_rows;         /* [total rows * 2] rows [ax, ay]                                             */
    /* ABI v6 -- A FLEET OF DIFFERENT CARS (ltpl_fleet_*, and since the round-4 merge of the two state machines ltpl_planner_* as well:
     * the host planner groups its jobs per car; every table 1 .. 64 rows, every vel_max > 0, checked before any memory is cut):
     * Graph_LTPL.calc_vel_profile
     * takes vel_max and ax_max_machines per call, i.e. per vehicle (Graph_LTPL.py:344-351). n_ax_tables > 1: ax_max_machines holds that
     * many tables back to back, table t = rows ax_table_off[t] .. ax_table_off[t + 1] (ax_table_off[n_ax_tables] = n_ax_max_machines),
     * planner s uses table ax_table_idx[s]. Both NULL with n_ax_tables <= 1: one table for all.                                    */
    const int32_t* ax_table_off;    /* [n_ax_tables + 1] first row of every table                                  */
    const int32_t* ax_table_idx;    /* [n_scen] table of every planner                                              */
} ltpl_planner_vel_in;

/* Sizes a caller needs for the query buffers below: rows per (stitched) path / trajectory, nodes per path. */
typedef struct { int32_t cap_rows; int32_t cap_nodes; } ltpl_planner_caps;

typedef struct {
    /* state after calc_paths: path_dict of Graph_LTPL.calc_paths, keys in the reference's dict order             */
    int32_t  n_keys;
    int32_t  key_id[LTPL_PLANNER_MAX_KEYS];
    int32_t  n_rows[LTPL_PLANNER_MAX_KEYS];
    int32_t  n_nodes[LTPL_PLANNER_MAX_KEYS];
    int32_t  red_len[LTPL_PLANNER_MAX_KEYS];
    int32_t  start_node[2];
    int32_t  const_rows;            /* rows of const_path_seg or -1 (None)                                        */
    int32_t  closest_obj_index;     /* -1 = None                                                                  */
    double*  path_param[LTPL_PLANNER_MAX_KEYS];   /* caller buffers [cap_rows * 5] or NULL                        */
    double*  coeff[LTPL_PLANNER_MAX_KEYS];        /* caller buffers [cap_nodes * 8] or NULL                       */
    int32_t* nodes[LTPL_PLANNER_MAX_KEYS];        /* caller buffers [cap_nodes * 2] pairs (layer, node), -1 = None */
    int32_t* node_idx[LTPL_PLANNER_MAX_KEYS];     /* caller buffers [cap_nodes]                                   */
} ltpl_planner_paths_view;

typedef struct {
    /* result of calc_vel_profile: action_set / action_set_id of Graph_LTPL.calc_vel_profile (untrimmed)          */
    int32_t  n_keys;
    int32_t  key_id[LTPL_PLANNER_MAX_KEYS];
    int32_t  traj_id[LTPL_PLANNER_MAX_KEYS];
    int32_t  n_rows[LTPL_PLANNER_MAX_KEYS];
    int32_t  cut_index_pos, cut_layer;            /* outputs of get_ref_idx (OTH.py:601)                          */
    double   vel_plan, acc_plan;
    int32_t  n_vel_course;
    /* action_set_path_id of OTH.py:696-697,1034: one id per key of the tick INCLUDING keys dropped for a broken velocity
     * bound (the reference never removes them from this dict)                                                    */
    int32_t  n_ids;
    int32_t  id_key[LTPL_PLANNER_MAX_KEYS];
    int32_t  id_val[LTPL_PLANNER_MAX_KEYS];
    double*  traj[LTPL_PLANNER_MAX_KEYS];         /* caller buffers [cap_rows * 7] rows [s, x, y, psi, kappa, vx, ax] or NULL */
    double*  vel_course;                          /* caller buffer [cap_rows] or NULL                             */
} ltpl_planner_traj_view;

int ltpl_planner_create(ltpl_handle* handle, const ltpl_planner_config* cfg, ltpl_planner** out_planner);
int ltpl_planner_destroy(ltpl_planner* planner);
int ltpl_planner_get_caps(const ltpl_planner* planner, ltpl_planner_caps* caps);
const char* ltpl_planner_last_error(const ltpl_planner* planner);
/* OnlineTrajectoryHandler.set_initial_pose (OTH.py:181-270) for planner `scen` */
int ltpl_planner_set_start(ltpl_planner* planner, int32_t scen, double x, double y, double heading, double vel,
                           double max_heading_offset, int32_t* in_track, int32_t* cor_heading);
int ltpl_planner_calc_paths(ltpl_planner* planner, const ltpl_planner_paths_in* in);
/* The same call in two halves for callers that own the zone bookkeeping (gen_local_node_template.py:42-99 decides on the
 * START NODE OF THIS SEARCH): _begin = OTH.update_objects + OTH.py:308-414 (the zone members of `in` are ignored; the start
 * nodes are then visible through ltpl_planner_get_paths), _finish = seam (1) + OTH.py:429-513 with the zone node ids. */
int ltpl_planner_calc_paths_begin(ltpl_planner* planner, const ltpl_planner_paths_in* in);
int ltpl_planner_calc_paths_finish(ltpl_planner* planner, const int32_t* zone_off, const int32_t* zone_gid);
/* OnlineTrajectoryHandler.get_ref_idx (OTH.py:518-601) on its own; optional -- ltpl_planner_calc_vel_profile runs it when it was
 * not called for the tick. Results: cut_index_pos .. vel_course of ltpl_planner_traj_view. */
int ltpl_planner_get_ref_idx(ltpl_planner* planner, const double* pos_est_x, const double* pos_est_y);
int ltpl_planner_calc_vel_profile(ltpl_planner* planner, const ltpl_planner_vel_in* in);
/* copy-out of planner `scen`'s state (fills the counts, copies the arrays whose pointers are non-NULL) */
int ltpl_planner_get_paths(const ltpl_planner* planner, int32_t scen, ltpl_planner_paths_view* view);
int ltpl_planner_get_trajectories(const ltpl_planner* planner, int32_t scen, ltpl_planner_traj_view* view);

/* ------------------------------------------------------------------------------------------------------------------
 * ABI v5 -- the FLEET: the same planner (the iterative memory of OnlineTrajectoryHandler, OTH.py:24-1040) for MANY vehicles on
 * one lattice with the state in DEVICE memory. Every stage of a tick that ltpl_planner_* runs on the host per planner
 * (OTH.py:308-414 in front of seam (1), :429-513 behind it, get_ref_idx :518-601, the slicing / job construction / trajectory
 * assembly / backup and emergency branches of calc_vel_profile :603-1040) runs as a kernel with one wave64 per planner
 * (csrc/fleet_core.hpp) between the launches of the path kernel and the velocity kernel: no host work per planner, no host
 * synchronisation inside a tick. Entry points and structs are those of ltpl_planner_* (same argument meaning, same views), so a
 * caller switches by the prefix. Differences, all reported and none silent:
 *   - local_gg in both forms since ABI v6 (gg_row_off / gg_rows: friction rows per planner and path key; rows that do not match
 *     the coordinates of the path are an error of that planner, OTH.py:641-646);
 *   - the conditions on which the reference raises (OTH.py:334, :712, :830, :919, :923, :1029, ...) are detected per planner on the
 *     device: the call returns the status of the FIRST failing planner ("fleet: planner N: ..."), that planner keeps its error
 *     state (its later ticks are skipped) until ltpl_fleet_set_start gives it a new pose; the other planners are not affected;
 *   - calc_time_buffer_len <= 16; capacities as ltpl_planner_caps.
 * The TAPE form replays pre-uploaded inputs: ltpl_fleet_tape_append packs the inputs of one tick (both calls' arguments) into
 * device memory, ltpl_fleet_tape_run advances all planners through ticks [first, first + count) back to back on the handle's
 * stream and reports the device time between the first and the last launch -- the closed-loop throughput of the hot path with
 * state carried from tick to tick (bench.py extra.closed_loop_device).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct ltpl_fleet ltpl_fleet;

int ltpl_fleet_create(ltpl_handle* handle, const ltpl_planner_config* cfg /* n_scen = planners */, ltpl_fleet** out_fleet);
int ltpl_fleet_destroy(ltpl_fleet* fleet);
int ltpl_fleet_get_caps(const ltpl_fleet* fleet, ltpl_planner_caps* caps);
const char* ltpl_fleet_last_error(const ltpl_fleet* fleet);
/* OnlineTrajectoryHandler.set_initial_pose for one planner (computed on the host, uploaded as that planner's state) */
int ltpl_fleet_set_start(ltpl_fleet* fleet, int32_t planner, double x, double y, double heading, double vel,
                         double max_heading_offset, int32_t* in_track, int32_t* cor_heading);
/* the same start pose for the planners [first, past_last) in one call (start spline computed once, block image copied on the device) */
int ltpl_fleet_set_start_range(ltpl_fleet* fleet, int32_t first, int32_t past_last, double x, double y, double heading, double vel,
                               double max_heading_offset, int32_t* in_track, int32_t* cor_heading);
int ltpl_fleet_calc_paths(ltpl_fleet* fleet, const ltpl_planner_paths_in* in);
int ltpl_fleet_calc_paths_begin(ltpl_fleet* fleet, const ltpl_planner_paths_in* in);
int ltpl_fleet_calc_paths_finish(ltpl_fleet* fleet, const int32_t* zone_off, const int32_t* zone_gid);
int ltpl_fleet_get_ref_idx(ltpl_fleet* fleet, const double* pos_est_x, const double* pos_est_y);
int ltpl_fleet_calc_vel_profile(ltpl_fleet* fleet, const ltpl_planner_vel_in* in);
/* copy-out of one planner's state (a device-to-host copy of its block, then as ltpl_planner_get_*) */
int ltpl_fleet_get_paths(ltpl_fleet* fleet, int32_t planner, ltpl_planner_paths_view* view);
int ltpl_fleet_get_trajectories(ltpl_fleet* fleet, int32_t planner, ltpl_planner_traj_view* view);
/* digest of EVERY planner's result of the last tick, computed on the device (one wave per planner, read only): per planner
 * LTPL_FLEET_DIGEST_DOUBLES doubles -- [0] error word, [1] cut_index_pos, [2] cut_layer, [3] n_keys, [4] n_ids, [5] vel_plan,
 * [6] n_vel_course, [7] acc_plan; per key k: [8 + 7 k ..] key id, trajectory id, rows, s of the last row, vx of the first and the last row,
 * sum of vx; per id k: [8 + 7 K + 2 k ..] key id, id value (K = LTPL_PLANNER_MAX_KEYS). What the reference's tick recordings hold for every
 * tick: a whole fleet is checked against a recording without copying planner blocks (bench.py extra.closed_loop_device_mixed). */
#define LTPL_FLEET_DIGEST_DOUBLES (8 + 9 * LTPL_PLANNER_MAX_KEYS)
int ltpl_fleet_digest(ltpl_fleet* fleet, double* out /* [n_planners * LTPL_FLEET_DIGEST_DOUBLES] */, int32_t doubles_per_planner);
int ltpl_fleet_tape_clear(ltpl_fleet* fleet);
int ltpl_fleet_tape_append(ltpl_fleet* fleet, const ltpl_planner_paths_in* paths_in, const ltpl_planner_vel_in* vel_in);
int ltpl_fleet_tape_run(ltpl_fleet* fleet, int32_t first, int32_t count, float* ms_total /* may be NULL */);

/* ------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- CLOSED-LOOP SIMULATION of the fleet on the device: the example driver's loop (main_std_example.py:98-135)
 * around every planner, with no host work per tick. Tick k of planner p (csrc/fleet_sim.hpp, one wave64 per planner):
 *   1. now += dt (fp64 accumulation, t_now of the tick = now);
 *   2. the action: the first entry of the planner's preference list that is a key of the previous tick's exported trajectory set (before
 *      the first tick: {'straight': None}); none -> the planner's error word is set (the driver's KeyError) and the planner stops;
 *   3. the opponents (ObjectlistDummy, objectlist_dummy.py:148-170): toc = now - tic, tic = now, 1 ms steps of
 *      s += interp(s, s_rl, vel_rl * vel_scale) * 0.001 while t < toc (s = 0 at s >= s_rl[-1]), then x, y, psi (psi > pi -> - 2 pi), v
 *      interpolated on the race line; the planner's static objects follow in list order;
 *   4. object ingestion (on-track test, 0.2 s constant-velocity prediction, radius = length / 2: ltpl_process_objects' device code);
 *      objects off the track are dropped, the others compacted into the fleet's object layout (count, exclusive scan, write);
 *   5. the ego tracker (vdc_dummy.py:5-58, iter_time = dt) on the previous tick's trajectory of the selected action, trimmed to n_export
 *      rows: the two nearest rows (exact ties: the LOWER indices; numpy leaves their order open), s = distance + s of the lower one,
 *      1 ms steps of max(interp(s) * 0.001, 0.0001), then x, y, vx interpolated; <= 2 rows: the pose stays, vel_est = vx[0];
 *   6. the fleet's tick on these inputs (paths_pre, path kernel, paths_post, velocity stages), zones constant per planner.
 * np.interp is replayed in numpy's operation order (clamping at both ends, fp[j] on a knot, the NaN fallback). Opponent poses depend on
 * the clock and the race line alone and are bit-identical to the reference's.
 * ------------------------------------------------------------------------------------------------------------------ */
#define LTPL_FLEET_SIM_MAX_PREF     5     /* entries of a preference list (LTPL_ACT_*, emergency allowed)              */
#define LTPL_FLEET_SIM_MAX_EXPORT 256     /* n_export cap (the reference's nmbr_export_points: 115, Graph_LTPL.py:400-406) */
/* trace record per tick and planner: [0] sel action, [1] t_now, [2] pos_est x, [3] pos_est y, [4] vel_est, [5] on-track vehicles,
 * [6] / [7] X / Y of the first vehicle (NaN without one), then the tick's ltpl_fleet_digest row */
#define LTPL_FLEET_SIM_TRACE_DOUBLES (8 + LTPL_FLEET_DIGEST_DOUBLES)

typedef struct {
    int32_t n_rl;                   /* rows of the race-line table, >= 2                                          */
    const double*  race;            /* [n_rl * 5] rows [s_rl, x, y, psi, vel_rl], s_rl non-decreasing (shared by the fleet)  */
    const int32_t* opp_off;         /* [n + 1] opponents of planner p: opp_off[p] .. opp_off[p + 1]               */
    const double*  opp_s0;          /* [n_opp] initial arc length                                                 */
    const double*  opp_vel_scale;   /* [n_opp] factor on vel_rl                                                   */
    const double*  opp_length;      /* [n_opp] object length (radius = length / 2)                                */
    const int32_t* static_off;      /* [n + 1] static objects of planner p, behind its opponents in the object list */
    const double*  static_x;        /* [n_static] ...                                                             */
    const double*  static_y;
    const double*  static_theta;
    const double*  static_v;
    const double*  static_length;
    double  t0;                     /* clock before the first tick                                                */
    double  tic0;                   /* time of every opponent's previous call                                      */
    double  dt;                     /* clock step per tick (also vdc_dummy's iter_time), > 0                       */
    int32_t n_export;               /* exported trajectory rows, 1 .. LTPL_FLEET_SIM_MAX_EXPORT                     */
    const int32_t* pref_off;        /* [n + 1] preference list of planner p: 1 .. LTPL_FLEET_SIM_MAX_PREF entries    */
    const int32_t* pref_action;     /* LTPL_ACT_* in order of preference                                           */
    const double*  pos_est_x;       /* [n] initial pose estimate / velocity                                        */
    const double*  pos_est_y;
    const double*  vel_est;
    const int32_t* zone_off;        /* [n + 1] node ids the "overtaking_zones" filter removes (constant per run)   */
    const int32_t* zone_gid;
} ltpl_fleet_sim_in;

/* (re)initialises the simulation of every planner; the planners' own memory (ltpl_fleet_set_start) is not touched */
int ltpl_fleet_sim_setup(ltpl_fleet* fleet, const ltpl_fleet_sim_in* in);
/* velocity arguments of the following runs (pos_est / vel_est members ignored; gg_row_off / gg_rows: LTPL_ERR_UNSUPPORTED -- location
 * dependent friction of a simulation comes from the fleet's maps, ltpl_fleet_friction below) */
int ltpl_fleet_sim_vel(ltpl_fleet* fleet, const ltpl_planner_vel_in* in);
/* n_ticks ticks back to back on the handle's stream; trace (may be NULL): [n_ticks][n][doubles_per_tick_planner] with
 * doubles_per_tick_planner == LTPL_FLEET_SIM_TRACE_DOUBLES, copied out once at the end; ms_total (may be NULL): device time of the run.
 * Returns the status of the first failing planner like ltpl_fleet_tape_run; the trace is written either way. */
int ltpl_fleet_sim_run(ltpl_fleet* fleet, int32_t n_ticks, double* trace, int32_t doubles_per_tick_planner, float* ms_total);
/* copy-out of the simulation state (every pointer may be NULL): [n] pose estimate, velocity, last selected action, clock;
 * [n_opp] opponent arc length and time of its last call */
int ltpl_fleet_sim_state(ltpl_fleet* fleet, double* pos_est_x, double* pos_est_y, double* vel_est, int32_t* sel_action, double* now,
                         double* opp_s, double* opp_tic);

/* ------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- RACES: planners of one fleet that see one another. A race is a contiguous range of planners,
 * race_off[r] .. race_off[r + 1] - 1. The tracker of step 5 above also yields a heading theta: psi (column 3) of the same trimmed
 * trajectory at the same s and segment j as x, y and vx --
 *     j < 0: psi[0]     j >= n - 1: psi[n - 1]     ts[j + 1] == ts[j]: psi[j]
 *     else:  d = psi[j + 1] - psi[j]; d > pi: d -= 2 pi, d < -pi: d += 2 pi; theta = psi[j] + d * ((s - ts[j]) / (ts[j + 1] - ts[j]));
 *            theta > pi: theta -= 2 pi, theta <= -pi: theta += 2 pi
 * (the pose unchanged -- not started, <= 2 rows -- keeps theta; before the first trajectory theta = heading0). After EVERY planner's
 * tracker of the tick (a kernel boundary), each mate q != p of p's race, in ascending planner order, becomes the object
 * {X: pos_x[q], Y: pos_y[q], theta: theta[q], v: vel[q], length: length[q]} of step 4's ingestion; the survivors follow p's opponents and
 * statics, trace field [5] counts them, [6] / [7] hold the first surviving object of the whole list. A failed planner takes no objects
 * and stays in its mates' lists at its last pose, speed and heading. Opponents + statics + (race size - 1) <= 96 for every planner
 * (else LTPL_ERR_CAPACITY). Races of size 1 change nothing: the same kernels run, the trace is bit-identical.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n_races;                /* >= 1                                                                       */
    const int32_t* race_off;        /* [n_races + 1] non-decreasing, 0 .. n                                        */
    const double*  length;          /* [n] object length of planner p as a mate (radius = length / 2), finite > 0  */
    const double*  heading0;        /* [n] heading before the first trajectory, finite                             */
} ltpl_fleet_sim_race_in;

/* after ltpl_fleet_sim_setup (which clears the races), before the first ltpl_fleet_sim_run (after it: LTPL_ERR_INVALID_ARG): sets the races
 * and every planner's heading to heading0. A failing call (LTPL_ERR_HIP) leaves the previous races in place. */
int ltpl_fleet_sim_race(ltpl_fleet* fleet, const ltpl_fleet_sim_race_in* in);
/* [n] heading of every planner's tracked pose */
int ltpl_fleet_sim_heading(ltpl_fleet* fleet, double* theta);

/* ------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- FRICTION MAPS resident on the device: location dependent grip for a fleet (local_gg as a dict,
 * OnlineTrajectoryHandler.py:633-666: one [ax, ay] row per path coordinate of every offered key). A map is a regular grid of nodes,
 * interpolated bilinearly and clamped at its border. For x (y likewise, with y0, dy, ny, fy, v):
 *     tx = (x - x0) / dx;  fx = floor(tx), not (fx >= 0): fx = 0, fx > nx - 2: fx = nx - 2;  u = tx - fx, u < 0: u = 0, u > 1: u = 1
 *     lo = (1 - u) a[fy][fx] + u a[fy][fx + 1];  hi = (1 - u) a[fy + 1][fx] + u a[fy + 1][fx + 1];  value = ((1 - v) lo + v hi) * scale
 * in exactly this order of fp64 operations, for ax and ay each (host mirror: friction.FrictionGrid.rows, equal bit for bit).
 * A planner with a map takes the rows of every offered key from the map -- columns x, y of the stitched path_param times the planner's
 * scale -- on every route that runs the fleet's velocity stage (ltpl_fleet_calc_vel_profile, ltpl_fleet_tape_run, ltpl_fleet_sim_run with or
 * without races). The call's constant tuple (gg_ax / gg_ay) is not used for that planner -- the reference does not read a tuple either when
 * it is handed a dict --, gg_scale applies on top, rows handed over for a key through gg_row_off / gg_rows take precedence, and the
 * emergency profile on a backup plan with rows is reported as with caller rows (OTH.py:1029-1036).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n_maps;                 /* 0: clears the maps (every other member is ignored)                          */
    const double*  x0;              /* [n_maps] coordinates of node (0, 0), finite                                 */
    const double*  y0;
    const double*  dx;              /* [n_maps] node spacing, finite > 0                                           */
    const double*  dy;
    const int32_t* nx;              /* [n_maps] nodes per row / rows, >= 2                                         */
    const int32_t* ny;
    const int32_t* node_off;        /* [n_maps + 1] first node of every map in `nodes`: node_off[m + 1] - node_off[m] == nx[m] * ny[m] */
    const double*  nodes;           /* [node_off[n_maps]][2] = [ax, ay] of node (iy, ix) at node_off[m] + iy * nx[m] + ix; finite > 0  */
    const int32_t* map_idx;         /* [n] map of planner p, -1: the planner keeps its constant tuple               */
    const double*  scale;           /* [n] grip factor of planner p on its map, finite > 0                          */
} ltpl_fleet_friction_in;

/* OTH.py:633-666. Sets (or clears) the fleet's maps; between ticks or runs at any time, also after ltpl_fleet_sim_run. Every argument is
 * checked before the first HIP call; a failing call leaves the previous maps in place. After n_maps = 0 the planners plan on the call's
 * constant tuple again (same results as a fleet handed rows up to that tick and tuples from then on); a backup plan stored while on a map
 * keeps its own rows (OTH.py:963-968), so the brake / emergency launches of such a fleet stay in their rows form. */
int ltpl_fleet_friction(ltpl_fleet* fleet, const ltpl_fleet_friction_in* in);
/* OTH.py:633-666. scale [n]: new grip factors on the maps set before (a map that loses grip in the middle of a run), finite > 0 */
int ltpl_fleet_friction_scale(ltpl_fleet* fleet, const double* scale);
/* OTH.py:633-666. Batched lookup on the device: out [n_pts][2] = [ax, ay] of map `map` at (x[i], y[i]) times `scale`. A pure lookup: `scale`
 * is any finite factor (zero and negative values included), unlike the planners' grip factors above, which the velocity stage divides by
 * and which therefore must be positive. */
int ltpl_fleet_friction_rows(ltpl_fleet* fleet, int32_t map, const double* x, const double* y, int32_t n_pts, double scale, double* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- RACE TELEMETRY accumulated on the device: what happened in a simulated race, without the trace. Every planner
 * has a record of LTPL_FLEET_SIM_TELE_DOUBLES doubles, updated by ltpl_fleet_sim_run in every tick in which the planner is live (no error
 * word, an action found), after its tracker and after its mates were appended (csrc/fleet_sim.hpp: k_fleet_sim_tele, one wave64 per
 * planner; k_fleet_sim_rank for races with more than one planner). The reference logs the first of these numbers per tick itself:
 * s_coord = get_s_coord(raceline, pos_est, s_raceline, closed=True) (Graph_LTPL.py:436-440).
 *   L       = s_raceline[last] + sqrt(dx * dx + dy * dy), dx, dy = raceline[0] - raceline[last]: the closed length of the lattice's race line
 *   s(x, y) = what ltpl_raceline_s returns (the wave-wide projection of the device code; a lattice whose s_raceline[0] exceeds 0.05 --
 *             get_s_coord.py:67-68 shifts such an array -- is refused with LTPL_ERR_UNSUPPORTED)
 * The update reads the tracked pose, vel_est, the selected action and t_now of the tick, and the on-track objects the planner is handed
 * this tick (own position and radius; the predictions are not used). Fields, "before the first tick" value in brackets:
 *   [0]  ticks         live ticks accumulated [0]
 *   [1]  s             s(pos) of the last live tick [NaN]
 *   [2]  dist          sum of d = s_k - s_(k-1) (first live tick: 0); d < -L/2: d += L and a forward crossing; d > L/2: d -= L and a
 *                      backward crossing [0]
 *   [3]  laps          forward minus backward crossings [0]
 *   [4]  t_cross       time of the last forward crossing: t_now - dt * (s_k / d) with the wrapped d; t_now if !(d > 0) [NaN]
 *   [5]  lap_last      t_cross minus the previous t_cross [NaN until there are two]
 *   [6]  lap_best      smallest lap_last [NaN]
 *   [7]  vel_sum       sum of vel_est over the live ticks [0]         [8] vel_max  their maximum [-inf]
 *   [9 .. 13] act[5]   live ticks with the selected action LTPL_ACT_STRAIGHT / FOLLOW / LEFT / RIGHT / EMERGENCY [0]
 *   [14] clear_min     smallest sqrt(dx * dx + dy * dy) - radius of the object over all live ticks and all objects of the tick [+inf]
 *   [15] clear_tick    fleet tick index (ticks of ltpl_fleet_sim_run since the telemetry was set) and
 *   [16] clear_slot    list position at which clear_min was set: replaced only on a strictly smaller value, within a tick the first
 *                      smallest counts [-1]
 *   [17] contact_ticks live ticks in which the tick's smallest clearance is < radius[p] [0]
 *   [18] rank          1 + the number of planners q of p's race that are ahead: prog[q] > prog[p], or equal and q < p, with
 *                      prog = grid_s + dist. A mate that has not lived a tick is behind everybody; a failed mate stays where it stopped
 *                      [0; a planner alone in its race: 1 from its first live tick on]
 *   [19] passes        sum of the rank's decreases and  [20] passed  of its increases from one live tick to the next [0]
 *   [21] gap_ahead     prog[q] - prog[p] of the nearest q ahead [NaN; NaN for the leader]
 * Everything is fp64, + - * / and sqrt only, in the order written here (host mirror: sim.Telemetry). Ranks are per race; a race never
 * crosses a shard. A fleet without telemetry launches exactly the kernels it launches without this feature.
 * ------------------------------------------------------------------------------------------------------------------ */
#define LTPL_FLEET_SIM_TELE_DOUBLES 22
typedef struct {
    const double* radius;   /* [n] contact radius of planner p, finite >= 0 */
    const double* grid_s;   /* [n] or NULL: s of the first live tick        */
} ltpl_fleet_sim_tele_in;

/* (re)starts the telemetry with every record at its "before the first tick" values; in == NULL switches it off. After ltpl_fleet_sim_setup
 * (which switches it off) at any time between runs, also after ltpl_fleet_sim_race. Every argument is checked before the first HIP call
 * (no simulation, NaN / infinite / negative radius, non-finite grid_s: LTPL_ERR_INVALID_ARG); everything new is allocated before anything
 * old is freed: a failing call keeps the previous telemetry. */
int ltpl_fleet_sim_telemetry(ltpl_fleet* fleet, const ltpl_fleet_sim_tele_in* in);
/* synchronises the handle's stream and copies the records out: out [n][doubles_per_planner] with doubles_per_planner ==
 * LTPL_FLEET_SIM_TELE_DOUBLES; track_length (may be NULL): L. Accumulation goes on undisturbed. No simulation, a wrong record size or
 * telemetry off: LTPL_ERR_INVALID_ARG. */
int ltpl_fleet_sim_telemetry_read(ltpl_fleet* fleet, double* out, int32_t doubles_per_planner, double* track_length /* may be NULL */);

/* ------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- FLIGHT RECORDER: for a chosen subset of planners the device keeps a full record of every tick of
 * ltpl_fleet_sim_run in a ring of `depth` ticks, taken at the two points of the tick where the reference itself looks
 * (csrc/fleet_sim.hpp, one wave64 per RECORDED planner: the grid is the subset, not the fleet):
 *   capture P  k_fleet_sim_rec_paths, behind paths_post and in front of the velocity stage: what ltpl_fleet_get_paths would return at
 *              that moment -- start node, const_rows, closest_obj_index, per path key its id, n_rows, n_nodes, red_len and (layer, node)
 *              list -- and x, y of rows [0, const_rows) of the first key's path_param, the constant path segment as the reference logs it
 *              (Graph_LTPL.py:336-340, :445-447; the velocity stage trims the planner's memory to the cut layer afterwards, OTH.py:714-731);
 *   capture V  k_fleet_sim_rec_vel, behind the last kernel of the velocity stage: the head below, the objects the planner was handed this
 *              tick (its slice of the tick's object arrays, list order, <= 96: opponents and statics, then mates) and what
 *              ltpl_fleet_get_trajectories would return -- cut_index_pos, cut_layer, vel_plan, acc_plan, the id pairs, per trajectory key
 *              its id, trajectory id, UNTRIMMED row count and rows [0, min(rows, n_export)) -- without vel_course.
 * Record of (tick, recorded planner m) on the device: `stride` doubles at ring[(tick % depth) M + m], integers as exact doubles --
 *   head [64]: [0] tick [1] planner [2] error word [3] selected action [4] t_now [5] [6] pose x, y [7] vel_est [8] heading [9] objects
 *              [10] cut_index_pos [11] cut_layer [12] vel_plan [13] acc_plan [14] trajectory keys [15] id pairs
 *              [16 + 3 k ..] trajectory key k: key id, trajectory id, rows   [28 + 2 k ..] id pair k: key id, value
 *              [36] [37] start node [38] const_rows [39] closest_obj_index [40] path keys [41 + 4 k ..] path key k: id, n_rows, n_nodes, red_len
 *   objects [6][96] column-major (radius, velocity, x, y, predicted x, predicted y) | const [2][cap_rows] (x | y)
 *   | trajectories [K][7][n_export] column-major per key | nodes [K][cap_nodes][2] int32,   K = LTPL_PLANNER_MAX_KEYS
 *   stride = 64 + 576 + 2 cap_rows + 7 K n_export + K cap_nodes, rounded up to a multiple of 32 (cap_*: ltpl_planner_caps).
 * A live planner's head equals fields [0] .. [5] of its trace record. A planner whose error word is set gets a record in every tick as
 * well: its head with the simulation's last state of it (clock, action, pose, speed, heading), and zero counts (objects, keys, ids, path
 * keys; start node, const_rows and closest_obj_index -1). The recorder needs the state between paths_post and stage A, so a fleet with a
 * recorder takes the unfused launch sequence (LTPL_FLEET_NO_FUSE) whatever the environment says; results are bit-identical. A fleet
 * without a recorder launches exactly the kernels it launches without this feature. Indices are per fleet: a recorder never crosses a shard.
 * ------------------------------------------------------------------------------------------------------------------ */
#define LTPL_FLEET_SIM_RECORD_OBJECTS 96
typedef struct {
    int32_t tick;                   /* fleet tick: ticks of ltpl_fleet_sim_run since the recorder was set              */
    int32_t planner;
    int32_t error;                  /* error word of the planner (0: none), as field [0] of ltpl_fleet_digest            */
    int32_t sel_action;             /* LTPL_ACT_*, as trace field [0]                                                    */
    double  t_now;
    double  pos_x, pos_y;           /* tracked pose                                                                      */
    double  vel_est;
    double  heading;
    int32_t n_objects;              /* rows of `objects`, as trace field [5]                                             */
    int32_t reserved0;
} ltpl_fleet_sim_record_head;

/* sets or restarts the recorder for the planners[0 .. n_planners) (distinct, any order) with a ring of `depth` >= 1 ticks; planners == NULL
 * or n_planners == 0 switches it off. After ltpl_fleet_sim_setup (which switches it off) at any time between runs, before or after
 * ltpl_fleet_sim_race and ltpl_fleet_sim_telemetry. Every argument is checked before the first HIP call (no simulation, an index outside
 * 0 .. n - 1, an index given twice, depth < 1: LTPL_ERR_INVALID_ARG); everything new is allocated before anything old is freed: a failing
 * call keeps the previous recorder, its ring and its tick count. */
int ltpl_fleet_sim_record(ltpl_fleet* fleet, const int32_t* planners, int32_t n_planners, int32_t depth);
/* the ring holds the fleet ticks first_tick .. first_tick + n_ticks - 1 (every pointer may be NULL). Tick indices count the ticks of
 * ltpl_fleet_sim_run since the recorder was set and go on across several runs. Recorder off: n_planners = depth = n_ticks = 0. */
int ltpl_fleet_sim_record_info(ltpl_fleet* fleet, int32_t* n_planners, int32_t* depth, int32_t* first_tick, int32_t* n_ticks);
/* the record of fleet tick `tick` and recorded planner `slot` (position in the list given to ltpl_fleet_sim_record). Synchronises the
 * handle's stream; the first call after a run copies the ring to the host once, later calls are served from that copy until the next run
 * or a new recorder. Every pointer may be NULL. The view structs are filled the way ltpl_fleet_get_paths / _get_trajectories fill them:
 * counts always, arrays where the caller's pointer is non-NULL -- `nodes` of the paths view, `traj` of the trajectory view (rows
 * [0, min(n_rows, n_export)); n_rows is the untrimmed count). path_param, coeff, node_idx and vel_course are NOT recorded: those buffers
 * are left untouched, n_vel_course is 0. objects: rows [radius, velocity, x, y, predicted x, predicted y], n_objects of them.
 * const_xy: rows [x, y], min(const_rows, n_rows[0]) of them (none without a path key or with const_rows <= 0).
 * A tick the ring does not hold, a slot outside 0 .. M - 1, a recorder that is off: LTPL_ERR_INVALID_ARG. */
int ltpl_fleet_sim_record_get(ltpl_fleet* fleet, int32_t tick, int32_t slot, ltpl_fleet_sim_record_head* head,
                              double* objects /* [96][6] or NULL */, ltpl_planner_paths_view* paths,
                              double* const_xy /* [cap_rows][2] or NULL */, ltpl_planner_traj_view* traj);

/* ------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- SNAPSHOT AND BRANCH: the state of chosen planners of the simulation is copied on the device into one of
 * LTPL_FLEET_SIM_SNAPSHOTS slots of the fleet (ltpl_fleet_sim_snapshot) and from a slot, or from other planners of the live fleet, into
 * planners of the live fleet (ltpl_fleet_sim_branch): go back to the tick before a contact, run one situation with many parameter sets,
 * revive a planner whose error word is set. One kernel (csrc/fleet_branch.hpp: k_fleet_sim_branch, grid = chunks of a planner image x
 * pairs, 16 bytes per lane) serves all directions; no planner block passes through the host.
 * THE RULE: what the tick kernels write travels with the state, what the caller set stays the destination's own --
 *   copied (state)                                                     | stays (configuration)
 *   the planner block (its memory of ltpl_fleet_*, its error word)     | the race line, the opponents' vel_scale / length
 *   its window of friction rows, when windows exist on both sides      | statics, zones, preference list, dt, n_export
 *   now, sel, started, pos_x, pos_y, vel, theta, live                  | the velocity arguments (ltpl_fleet_sim_vel)
 *   opp_s / opp_tic of its opponents                                   | friction map index and scale
 *   with telemetry on: its record, grid_s and progress                 | race membership and length as a mate, contact radius
 *                                                                      | the recorder's ring and indices
 * - src and dst of a pair carry the same NUMBER of opponents (their offsets may differ; statics may differ): otherwise
 *   LTPL_ERR_INVALID_ARG, the message names the pair. The entries of dst are distinct. With the live fleet as source no planner is both a
 *   source and a destination, except a pair src == dst, which is skipped: the copy has no read-after-write hazard and needs no staging.
 * - The error word is copied: a healthy source revives a failed destination, a failed source fails the destination.
 * - Host counters are never rewound: the tick counts of the telemetry and the recorder go on counting executed ticks; a copied record
 *   keeps the source's clear_tick. The recorder is untouched: a recorded destination continues its ring.
 * - A snapshot has a telemetry part only if telemetry was on when it was taken. ltpl_fleet_sim_telemetry starts every record anew and so
 *   invalidates the telemetry part of the snapshots held; a branch copies the part only when both sides have one.
 * - Row windows are allocated by the first call that needs them and never freed. A snapshot taken before they existed holds no block
 *   that refers to rows; a branch from it leaves the destination's window alone.
 * - ltpl_fleet_sim_setup drops every snapshot (arrays and opponent counts change); ltpl_fleet_sim_race, _telemetry, _record, _vel and
 *   ltpl_fleet_friction* do not.
 * - All four calls need ltpl_fleet_sim_setup first, may come before or after runs, check every argument before the first HIP call,
 *   synchronise the handle's stream on entry and return after the copy has finished. A failing allocation returns LTPL_ERR_HIP and
 *   changes nothing. With models set (a selector, a safety monitor, reactive opponents) a branch is still one allocation, in front of
 *   up to four launches. After a branch a per-call ltpl_fleet_calc_vel_profile needs its own ltpl_fleet_calc_paths first, as after a run;
 *   ltpl_fleet_get_paths / _get_trajectories read the device at every call and so return the branched state.
 * ------------------------------------------------------------------------------------------------------------------ */
#define LTPL_FLEET_SIM_SNAPSHOTS 8   /* snapshot slots of a fleet */

/* copies the state of the chosen planners (planners == NULL: all n; else n_planners >= 1 distinct indices) into slot `slot`, replacing what
 * the slot held; everything new is allocated before anything old is freed: a failing call keeps the old snapshot */
int ltpl_fleet_sim_snapshot(ltpl_fleet* fleet, int32_t slot, const int32_t* planners, int32_t n_planners);
/* n_planners: planners of the slot (0: empty); planners (may be NULL): their indices in the order given, cap >= that many entries;
 * bytes (may be NULL): device memory of the slot */
int ltpl_fleet_sim_snapshot_info(ltpl_fleet* fleet, int32_t slot, int32_t* n_planners, int32_t* planners, int32_t cap, uint64_t* bytes);
/* frees the slot (an empty slot: nothing to do) */
int ltpl_fleet_sim_snapshot_drop(ltpl_fleet* fleet, int32_t slot);
/* for k < n_pairs: planner dst[k] of the LIVE fleet takes the state of planner src[k] of the source: slot == -1 the live fleet, else that
 * snapshot (an empty slot, or a src[k] that is not one of its planners: LTPL_ERR_INVALID_ARG). n_pairs == 0: nothing to do.
 * ms (may be NULL): device time of the copy. */
int ltpl_fleet_sim_branch(ltpl_fleet* fleet, int32_t slot, const int32_t* src, const int32_t* dst, int32_t n_pairs, float* ms);

/* ------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- SCRIPTED EVENTS: a per-planner event list, set once (ltpl_fleet_sim_events) and executed on the device inside
 * ltpl_fleet_sim_run at the head of every tick, in front of k_fleet_sim_step (csrc/fleet_events.hpp: k_fleet_sim_events_timed,
 * k_fleet_sim_triggers). An event is a condition (`when`) and ONE write into the planner's configuration (`set`). Every event fires at
 * most once; the tick in which it fired is kept on the device (ltpl_fleet_sim_events_read).
 * SCHEDULE TICK: the ticks ltpl_fleet_sim_run has executed since the events were set; 0 for the next tick to run. It goes on across
 * calls and is never rewound, like the tick counts of the telemetry and the recorder.
 * CONDITIONS are evaluated before tick k on the state as tick k - 1 left it (before the first tick: the state of ltpl_fleet_sim_setup).
 * A planner whose error word is set fires nothing: an event whose tick passes meanwhile never fires.
 *   LTPL_SIM_WHEN_TICK        fires at schedule tick when_index (>= 0); when_value is ignored
 *   LTPL_SIM_WHEN_OPP_WITHIN  when_index: an opponent of the planner (0 .. count - 1). Fires at the first tick with
 *                             dx dx + dy dy <= d d, d = when_value (finite, >= 0), dx / dy from the planner's tracked pose to the
 *                             opponent's position: np.interp of the race line's x / y columns at the opponent's stored arc length
 *                             (the x / y its last step produced, bit for bit). No sqrt; fp64, no contraction
 *   LTPL_SIM_WHEN_VEL_BELOW / _VEL_ABOVE   fires at the first tick with vel_est < when_value / vel_est > when_value (strict; finite)
 *   LTPL_SIM_WHEN_AFTER       when_index: an EARLIER event of the same planner (its place in the planner's list) whose kind is one of the
 *                             three state conditions or LTPL_SIM_WHEN_AFTER. Fires at fired_tick[that] + when_value, when_value integral
 *                             and >= 1. A reference to a LTPL_SIM_WHEN_TICK event is LTPL_ERR_INVALID_ARG (use LTPL_SIM_WHEN_TICK)
 * WRITES (set_index is local to the planner):
 *   LTPL_SIM_SET_OPP_VEL_SCALE / _OPP_LENGTH                  opponent set_index; finite; scale >= 0, length > 0
 *   LTPL_SIM_SET_STATIC_X / _Y / _THETA / _V / _LENGTH         static object set_index; finite; length > 0. (No kind lets a static
 *                                                             "appear": set it up off the track, where ingestion drops it, and move it)
 *   LTPL_SIM_SET_PREF                                         entry set_index of the preference list (its length stays); an LTPL_ACT_*
 *   LTPL_SIM_SET_VEL_MAX / _GG_SCALE / _GG_AX / _GG_AY / _SAFETY_D   the planner's element of ltpl_fleet_sim_vel's arrays (set_index 0);
 *                                                             finite; > 0, safety_d >= 0
 *   LTPL_SIM_SET_INCL_EMERG                                   incl_emerg_traj of the planner (0 / 1). ONLY with LTPL_SIM_WHEN_TICK (else
 *                                                             LTPL_ERR_UNSUPPORTED): the host derives the launches of the emergency
 *                                                             stage from these flags, so it follows them in a shadow of its own, and
 *                                                             tick k launches exactly what a run split at k launches. The flag itself
 *                                                             is written whatever the error word (the shadow stays exact); the event of
 *                                                             a failed planner is still not marked fired
 *   LTPL_SIM_SET_FRICTION_SCALE                               the planner's grip factor on its friction map (set_index 0); finite > 0.
 *                                                             A run with such an event and no maps set is refused before its first launch
 * ORDER: the timed events of tick k are applied first, then the state-conditioned and LTPL_SIM_WHEN_AFTER events ("triggers") that fire
 * in tick k, per planner in list order: of two triggers that write the same target in the same tick the later one of the list wins. Two
 * LTPL_SIM_WHEN_TICK events with the same tick, kind, planner and index are refused. Conditions read state only, never configuration: a
 * write cannot change a condition of the same tick. At most LTPL_FLEET_SIM_MAX_TRIGGERS triggers per planner (LTPL_ERR_CAPACITY); timed
 * events are unlimited in number.
 * THE CALL follows the rules of ltpl_fleet_sim_telemetry: after ltpl_fleet_sim_setup at any time, between runs; every argument is checked
 * before the first HIP call, the message names the planner and the event; everything new is allocated before anything old is freed; a
 * failing call keeps the previous list, its tick and its fired ticks; a successful call replaces the list, sets the tick to 0 and every
 * fired tick to -1. in == NULL or n_events == 0 switches the events off, and so does ltpl_fleet_sim_setup.
 * INTERPLAY: the list, its tick and the fired ticks are the live fleet's own, like the recorder: ltpl_fleet_sim_snapshot / _branch copy
 * none of it, and what events wrote is configuration, which stays the destination's own. A later ltpl_fleet_sim_vel, ltpl_fleet_friction
 * or ltpl_fleet_friction_scale sets its arrays anew: events that fired earlier are not applied again. (Those calls may re-allocate their
 * buffers; the event kernels are handed the target pointers at every launch.) A fleet without events launches per tick exactly the
 * kernels it launched before, with unchanged arguments; with events a tick has one more launch where a timed event falls on it and one
 * more while the list holds triggers.
 * ------------------------------------------------------------------------------------------------------------------ */
#define LTPL_FLEET_SIM_MAX_TRIGGERS 16   /* events of a planner that are not LTPL_SIM_WHEN_TICK */
#define LTPL_SIM_WHEN_TICK        0
#define LTPL_SIM_WHEN_OPP_WITHIN  1
#define LTPL_SIM_WHEN_VEL_BELOW   2
#define LTPL_SIM_WHEN_VEL_ABOVE   3
#define LTPL_SIM_WHEN_AFTER       4
#define LTPL_SIM_SET_OPP_VEL_SCALE   0
#define LTPL_SIM_SET_OPP_LENGTH      1
#define LTPL_SIM_SET_STATIC_X        2
#define LTPL_SIM_SET_STATIC_Y        3
#define LTPL_SIM_SET_STATIC_THETA    4
#define LTPL_SIM_SET_STATIC_V        5
#define LTPL_SIM_SET_STATIC_LENGTH   6
#define LTPL_SIM_SET_PREF            7
#define LTPL_SIM_SET_VEL_MAX         8
#define LTPL_SIM_SET_GG_SCALE        9
#define LTPL_SIM_SET_GG_AX          10
#define LTPL_SIM_SET_GG_AY          11
#define LTPL_SIM_SET_SAFETY_D       12
#define LTPL_SIM_SET_INCL_EMERG     13
#define LTPL_SIM_SET_FRICTION_SCALE 14

typedef struct {
    int32_t n_events;              /* 0 (or in == NULL): switches the events off */
    const int32_t* ev_off;         /* [n + 1] events of planner p, in list order */
    const int32_t* when_kind;      /* [n_events] LTPL_SIM_WHEN_*                 */
    const int32_t* when_index;     /* [n_events]                                 */
    const double*  when_value;     /* [n_events]                                 */
    const int32_t* set_kind;       /* [n_events] LTPL_SIM_SET_*                  */
    const int32_t* set_index;      /* [n_events]                                 */
    const double*  set_value;      /* [n_events]                                 */
} ltpl_fleet_sim_events_in;
int ltpl_fleet_sim_events(ltpl_fleet* fleet, const ltpl_fleet_sim_events_in* in);
/* fired_tick (may be NULL): [n_events] schedule tick in which event e fired, -1: not yet; n_events (may be NULL): events of the list (0: events
 * are off); tick (may be NULL): the schedule tick. No simulation: LTPL_ERR_INVALID_ARG. */
int ltpl_fleet_sim_events_read(ltpl_fleet* fleet, int32_t* fired_tick, int32_t* n_events, int32_t* tick);

/* ------------------------------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- SEEDED SENSOR NOISE: localisation and perception errors of every planner of the closed-loop simulation, drawn on
 * the device inside ltpl_fleet_sim_run (csrc/fleet_sim.hpp: k_fleet_sim_step_noise, k_fleet_sim_mates_noise; the generator:
 * csrc/fleet_noise.hpp). Without it every planner sees its tracked pose and every object exactly.
 * THE SAMPLE g(seed, tick, obj, comp): Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten
 * rounds) under the key (seed low word, seed high word) on the three counters (tick, obj, 3 comp + b, 0), b = 0, 1, 2; K = the sum of the
 * 12 output words as uint64; g = ((double)K + 6.0) 2^-32 - 6.0: the sum of twelve uniforms minus six, mean 0, variance 1 - 2^-64, |g| < 6.
 * Every step is exact in fp64: host (sim.noise_gauss) and device agree to the last bit.
 *   obj   0xFFFFFFFF: the ego estimate | k: entry k of the planner's own object list, opponents first, then statics (the index BEFORE the
 *         on-track compaction) | 0x80000000 | (q - first planner of the race): mate q of a race
 *   comp  ego: 0 x, 1 y, 2 v; object: 0 x, 1 y, 2 theta, 3 v
 *   tick  tick0 + the fleet ticks ltpl_fleet_sim_run has executed since the noise was set; it advances every tick, live planner or not
 * A draw depends on the planner's seed, never on its index: a planner computes the same in any fleet and on any shard.
 * WHAT IS PERTURBED, one multiply and one add each (value + sigma g); a sigma of 0 draws nothing and hands the value through untouched:
 *   ego      est_x = pos_x + sigma_pos g(.., 0), est_y likewise with comp 1, est_v = max(0, vel + sigma_vel g(.., 2)), written behind the
 *            tracker. The fleet's tick (get_ref_idx, the velocity stage) reads them as pos_est / vel_est. The TRUE pose stays what the
 *            tracker starts from, what the mates see of one another, and what ltpl_fleet_sim_state, the trace ([2] .. [4]), telemetry,
 *            the events' conditions and the flight recorder's head hold.
 *   objects  x, y (sigma_obj_pos), theta (sigma_obj_theta) and v (sigma_obj_vel, clamped at 0) of every opponent, static object and mate
 *            in front of the ingestion. The PERCEIVED values are what the planner is handed, what decides "on the track", and what trace
 *            fields [6] [7] and the recorder's objects hold.
 * TELEMETRY measures clearance and contacts against the TRUE positions of the objects the planner was handed. Limit: an object perceived
 * off the track is dropped by the ingestion and so is not measured, even where it truly is on the track.
 * A planner whose sigmas are all 0 computes bit for bit what a fleet without noise computes. Snapshot and branch copy state, not
 * configuration: seeds and sigmas stay the destination's own.
 * THE CALL: after ltpl_fleet_sim_setup (which switches the noise off) at any time between runs; in == NULL switches it off. Every argument
 * is checked before the first HIP call: no simulation, a sigma that is negative or not finite, a missing seed array or a negative tick0 are
 * LTPL_ERR_INVALID_ARG with a message. Everything new is allocated before anything old is freed: a failing call keeps the previous noise and
 * its tick count.
 * ------------------------------------------------------------------------------------------------------------------------------------------ */
typedef struct {
    const uint64_t* seed;            /* [n]                                            */
    const double* sigma_pos;         /* [n] m;   NULL: all zero (every sigma array)     */
    const double* sigma_vel;         /* [n] m/s                                        */
    const double* sigma_obj_pos;     /* [n] m                                          */
    const double* sigma_obj_theta;   /* [n] rad                                        */
    const double* sigma_obj_vel;     /* [n] m/s                                        */
    int32_t tick0;                   /* >= 0: the noise tick of the next tick to run   */
} ltpl_fleet_sim_noise_in;
int ltpl_fleet_sim_noise(ltpl_fleet* fleet, const ltpl_fleet_sim_noise_in* in);
/* the planners' pos_est / vel_est of the last tick (each may be NULL); the true state while the noise is off and until the first noisy tick */
int ltpl_fleet_sim_estimate(ltpl_fleet* fleet, double* x, double* y, double* v);
/* the test hook of the generator (k_fleet_noise_draws, one lane per tuple): g[i] = g(seed[i], tick[i], obj[i], comp[i]); words (may be
 * NULL): [n][12] the output words of the three blocks. Needs a fleet, no simulation. */
int ltpl_fleet_sim_noise_draws(ltpl_fleet* fleet, const uint64_t* seed, const uint32_t* tick, const uint32_t* obj, const uint32_t* comp, int32_t n,
                               double* g, uint32_t* words);

/* ------------------------------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- VEHICLE MODEL: a car between the planned trajectory and the pose of the next tick, integrated on the device inside
 * ltpl_fleet_sim_run (csrc/fleet_sim.hpp: k_fleet_sim_step_veh, k_fleet_sim_step_noise_veh; the model: csrc/fleet_vehicle.hpp). Without it
 * step 5 of a tick is the ideal tracker: the car is put ONTO its previous trajectory at exactly the planned speed. A planner with model 1
 * drives a kinematic single-track car with actuator lags, a friction circle of its TRUE grip and a pure-pursuit / speed controller over the
 * same trimmed rows of the previous trajectory of the selected action (columns s, x, y, vx and ax). Before the first trajectory nothing
 * moves, as with the ideal tracker.
 * ARITHMETIC: fp64, + - * / sqrt only, one fixed order (the library is built with -ffp-contract=off): the host mirror sim.VehicleModel and
 * the device agree to the last bit. The heading is carried as a unit vector (c, s), never as an angle: the direction of travel. The
 * library's headings (heading0, the psi column, ltpl_fleet_sim_heading) are measured from the y axis -- the direction of travel of a
 * heading theta is (-sin theta, cos theta) -- so c = -sin theta, s = cos theta and theta = atan2(-c, s).
 * STATE per planner: x, y, c, s, v, a, kappa.  A TICK: t = 0; k = 0; while (t < dt) { if (k % ctl_steps == 0) control; plant; t += 0.001; ++k; }
 * CONTROL at the pose p = (x, y):
 *   1 projection  every segment i = 0 .. n - 2 of the rows with l2 = dx dx + dy dy > 0: u = ((px - x_i) dx + (py - y_i) dy) / l2 clamped to
 *                 [0, 1], foot f = (x_i + u dx, y_i + u dy), d2 = |p - f|^2. The smallest d2 wins, ties to the lower i. On the winner
 *                 e = (dx (py - y_i) - dy (px - x_i)) / sqrt(l2) (positive: left of the trajectory), sf = s_i + u (s_{i+1} - s_i)
 *   2 references  vref, aff = np.interp of vx, ax at sf
 *   3 look-ahead  Ld = max(ld_min, t_look v), st = sf + Ld, target = np.interp of x, y at st (clamped at the last row); where
 *                 st > s_{n-1}: target += (st - s_{n-1}) (dx / sqrt(l2), dy / sqrt(l2)) of the last segment with l2 > 0
 *   4 curvature   r = target - p, yl = -s r_x + c r_y, L2 = r_x r_x + r_y r_y; kappa_cmd = L2 > 0 ? (2 yl) / L2 : 0, clamped to +-kappa_max
 *   5 friction    ay_lim = ay_max grip, ax_lim = ax_max grip, v2 = v v. |kappa_cmd| v2 > ay_lim: kappa_cmd = copysign(ay_lim / v2, kappa_cmd)
 *                 and sat_lat counts. q = (kappa_cmd v2) / ay_lim, rem = ax_lim sqrt(max(0, 1 - q q)); a_cmd = aff + k_v (vref - v),
 *                 clamped to +-rem; sat_lon counts where it was clamped
 *   6 statistics  e, e_max = max |e|, e2_sum += e e, dv_max = max |vref - v|, ctl += 1
 *   no usable trajectory (n <= 2, or no segment with l2 > 0): kappa_cmd = kappa (the steering is held), a_cmd = -ax_lim, and no statistic
 *   of 5 and 6 changes: ctl counts the control steps that had a trajectory
 * PLANT, h = 0.001: a += (a_cmd - a) (h / tau_a); kappa += (kappa_cmd - kappa) (h / tau_kappa); v += a h, a negative v becomes 0; ds = v h;
 *   t = 0.5 kappa ds; c' = ((1 - t t) c - (2 t) s) / (1 + t t); s' = ((1 - t t) s + (2 t) c) / (1 + t t); x += ds (0.5 (c + c'));
 *   y += ds (0.5 (s + s')); (c, s) = (c', s'). With kappa and v constant the car stays on the circle of radius 1 / kappa up to rounding.
 * END OF TICK: (c, s) divided by sqrt(c c + s s); pos = (x, y), vel = v, and the heading from the library's device atan2 of (-c, s)
 * (an output only: it never feeds the state; within 1e-12 of atan2). Everything downstream reads these unchanged: the mates, the noise
 * estimates (noise is added to the model's true pose), telemetry, the events' conditions, the recorder's head and the trace.
 * off_track_ticks counts the ticks in which the model ran and the pose at the end fails the track test of the object ingestion.
 * SNAPSHOT / BRANCH: state and statistics are written by the tick and travel with the planner; model and parameters stay the
 * destination's own. A destination on the ideal tracker takes no vehicle record (its own stays NaN); a destination with model 1 needs a
 * source that had model 1 when it was copied -- otherwise LTPL_ERR_INVALID_ARG.
 * THE CALL: after ltpl_fleet_sim_setup (which switches the model off; after ltpl_fleet_sim_race where heading0 matters) at any time between
 * runs; in == NULL switches it off: the tick then launches the kernels it launched before. Every argument is checked before the first HIP
 * call; the message names the planner and the field: model 0 or 1; for a planner with model 1 every parameter finite and positive, tau_a
 * and tau_kappa at least 0.001 s (the parameters of a planner with model 0 are not read); ctl_steps >= 1; no unknown flag. Everything new
 * is allocated before anything old is freed: a failing call keeps what was set. On success the state of every planner with model 1 is
 * its current true pose, speed and heading ((c, s) = host -sin / cos of the heading), a = kappa = 0, statistics cleared. With
 * LTPL_SIM_VEH_KEEP_STATE the planners that already had model 1 keep state and statistics and only the parameters change ("the grip
 * drops at tick 300" is two runs with such a call between them).
 * ------------------------------------------------------------------------------------------------------------------------------------------ */
#define LTPL_FLEET_SIM_VEH_DOUBLES 15   /* x, y, c, s, v, a, kappa, e (last), e_max, e2_sum, dv_max, ctl, sat_lat, sat_lon, off_track_ticks */
#define LTPL_SIM_VEH_KEEP_STATE 1u
typedef struct {
    const int32_t* model;            /* [n] 0: the ideal tracker, 1: the vehicle model */
    const double* ax_max;            /* [n] m/s^2 (every array is needed)              */
    const double* ay_max;            /* [n] m/s^2                                      */
    const double* grip;              /* [n] true grip factor on both limits            */
    const double* kappa_max;         /* [n] 1/m                                        */
    const double* tau_a;             /* [n] s, >= 0.001                                */
    const double* tau_kappa;         /* [n] s, >= 0.001                                */
    const double* k_v;               /* [n] 1/s                                        */
    const double* t_look;            /* [n] s                                          */
    const double* ld_min;            /* [n] m                                          */
    int32_t ctl_steps;               /* >= 1: control period in 1 ms plant steps       */
    uint32_t flags;                  /* LTPL_SIM_VEH_KEEP_STATE                         */
} ltpl_fleet_sim_vehicle_in;
int ltpl_fleet_sim_vehicle(ltpl_fleet* fleet, const ltpl_fleet_sim_vehicle_in* in);
/* out: [n][LTPL_FLEET_SIM_VEH_DOUBLES]; every double of a planner on the ideal tracker is NaN. No simulation, the model off or a wrong
 * record size: LTPL_ERR_INVALID_ARG. */
int ltpl_fleet_sim_vehicle_read(ltpl_fleet* fleet, double* out, int32_t doubles_per_planner);
/* the test hook of the model (k_fleet_sim_vehicle_step, one wave per case, the tick's own device function): case q has the state
 * state[q][7], the parameters params[q][9] (the order of the struct above), the rows rows[row_off[q] .. row_off[q + 1])[5] = s, x, y, vx,
 * ax (0 .. 256 of them), dt[q] in (0, 1] and ctl_steps[q] >= 1. out[q]: the state after the tick, the tick's statistics from zero, and
 * 1.0 as off_track_ticks where the pose fails the track test on the fleet's lattice; theta[q]: the heading. Needs a fleet, no simulation. */
int ltpl_fleet_sim_vehicle_step(ltpl_fleet* fleet, int32_t n_cases, const double* state, const double* params, const int32_t* row_off,
                                const double* rows, const double* dt, const int32_t* ctl_steps, double* out, int32_t doubles_per_case,
                                double* theta);

/* ------------------------------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- SENSOR MODEL: which of the tick's on-track objects a planner is shown, decided on the device inside
 * ltpl_fleet_sim_run (csrc/fleet_sim.hpp: k_fleet_sim_sense; the rule: csrc/fleet_sensor.hpp). Without it every planner is handed every
 * on-track object of the tick, every tick. The sensor is a pure function of the tick's TRUE state with no memory from tick to tick: it
 * is configuration, not state.
 * ARITHMETIC: fp64, + - * sqrt and comparisons only, one fixed order (the library is built with -ffp-contract=off): the host mirror
 * sim.SensorModel and the device agree to the last bit, given the same forward vector.
 * PER PLANNER p AND TICK: the true pose (px, py), the forward unit vector f = (-sin theta, cos theta) of its heading (the library's heading
 * is measured from the y axis; sin / cos are the device's), and the staged objects k = 0 .. cnt - 1 of the tick: opponents, statics and
 * mates behind the on-track ingestion, at their TRUE positions (the positions before ltpl_fleet_sim_noise moved them) with their radii r.
 *   dx = x - px;  dy = y - py;  L2 = dx dx + dy dy
 * An object is tested in this order; the first test that fails is its cause of loss:
 *   | # | cause     | lost when                                                                                   | off       |
 *   | 1 | range     | L2 > range range                                                                            | +inf      |
 *   | 2 | (near)    | L2 <= r_near r_near: tests 3 and 4 are skipped (all-round short-range sensing)              | 0         |
 *   | 3 | fov       | fov_cos > -1 and fx dx + fy dy < fov_cos sqrt(L2); fov_cos = cosine of the HALF opening     | -1 (not   |
 *   |   |           | angle                                                                                        | evaluated)|
 *   | 4 | occlusion | occl > 0 and some j != k among ALL staged objects of the tick has L2_j < L2_k and            | 0         |
 *   |   |           | dx_j dx_k + dy_j dy_k > 0 and cross cross <= ((occl r_j) (occl r_j)) L2_k, cross =           |           |
 *   |   |           | dx_j dy_k - dy_j dx_k. occl scales the occluder's radius. A lost object still occludes;      |           |
 *   |   |           | objects at equal distance never hide one another                                             |           |
 *   | 5 | dropout   | p_drop > 0 and u < p_drop; u = ((double)w0 + 0.5) 2^-32, w0 the first output word of ONE    | 0 (draws  |
 *   |   |           | Philox4x32-10 block, key = the sensor's seed of the planner, counter (tick, k, 0, 1)         | nothing)  |
 * k is the object's slot in the tick's on-track list before the sensor; tick = tick0 + the fleet ticks run since the sensor was set (it
 * advances whether or not a planner is live). Every block of ltpl_fleet_sim_noise has 0 in counter word 3: one seed may serve both.
 * The seen objects keep their order (a stable compaction of the staged list, perceived values included). The "open" sensor (range +inf,
 * fov_cos -1, occl 0, p_drop 0) keeps every object: bit-identical to a fleet without the call.
 * STATISTICS per planner, LTPL_FLEET_SIM_SENSOR_DOUBLES doubles, updated in every tick in which the planner is live:
 *   [0] ticks  [1] n_obj: sum of on-track counts  [2] n_seen  [3] n_range  [4] n_fov  [5] n_occl  [6] n_drop: objects lost to each cause
 *   [7] blind_ticks: ticks with at least one lost object  [8] blind_clear_min: smallest sqrt(L2) - r over the lost objects (telemetry's
 *   clearance, on truth; +inf at the start)  [9] blind_clear_tick: the sensor tick of that minimum (-1 at the start; the first smallest
 *   wins, within a tick the lower slot)
 * IN THE TICK: behind k_fleet_sim_tele / _rank, in front of k_fleet_sim_offsets. Telemetry (clearance, contacts), LTPL_SIM_WHEN_OPP_WITHIN
 * and the mates' view of one another keep acting on truth; offsets, compaction, the planner and the flight recorder see what the sensor
 * kept: the recorder's objects are the seen ones, and trace fields [5] .. [7] describe the list handed on. A planner that is not live is
 * skipped. SNAPSHOT / BRANCH copy neither the configuration nor the statistics: both stay the destination's own. No event kind sets it.
 * LIMITS: no memory between ticks -- detection latency and track persistence come from the tracker behind it (OBJECT TRACKER below); no
 * burst dropouts; an object the ingestion drops as off the track neither is seen nor occludes.
 * THE CALL: after ltpl_fleet_sim_setup (which switches the sensor off) at any time between runs; in == NULL switches it off: the tick then
 * launches the kernels it launched before. Every argument is checked before the first HIP call, the message names the argument: every
 * array present; range not NaN and not negative (+inf allowed); r_near in [0, range]; fov_cos in [-1, 1]; occl finite and >= 0; p_drop
 * in [0, 1); tick0 >= 0. Everything new is allocated before anything old is freed: a failing call keeps the previous sensor, its tick
 * count and its statistics. A successful call starts the statistics anew.
 * ------------------------------------------------------------------------------------------------------------------------------------------ */
#define LTPL_FLEET_SIM_SENSOR_DOUBLES 10
typedef struct {
    const double* range;             /* [n] m, >= 0 or +inf (every array is needed)      */
    const double* r_near;            /* [n] m, 0 .. range                               */
    const double* fov_cos;           /* [n] cosine of the half opening angle, -1 .. 1   */
    const double* occl;              /* [n] factor on the occluder's radius, 0: off     */
    const double* p_drop;            /* [n] dropout probability per object and tick, [0, 1) */
    const uint64_t* seed;            /* [n] key of the dropout draws                    */
    int32_t tick0;                   /* >= 0: the sensor tick of the next fleet tick    */
} ltpl_fleet_sim_sensor_in;
int ltpl_fleet_sim_sensor(ltpl_fleet* fleet, const ltpl_fleet_sim_sensor_in* in);
/* out: [n][LTPL_FLEET_SIM_SENSOR_DOUBLES]. No simulation, the sensor off or a wrong record size: LTPL_ERR_INVALID_ARG. */
int ltpl_fleet_sim_sensor_read(ltpl_fleet* fleet, double* out, int32_t doubles_per_planner);
/* the test hook of the rule (k_fleet_sim_sensor_eval, one wave per case, the tick's own device functions): case q has the pose and the
 * forward vector pose_f[q][4] = px, py, fx, fy (f as given: no trigonometry), params[q][5] = range, r_near, fov_cos, occl, p_drop,
 * seed[q], tick[q] and the objects objs[obj_off[q] .. obj_off[q + 1])[3] = x, y, r (0 .. 96 of them). cause[i]: 0 seen, 1 .. 4 the cause of
 * loss in the order of the table; u[i]: the dropout draw where one was made, NaN otherwise. Needs a fleet, no simulation. */
int ltpl_fleet_sim_sensor_eval(ltpl_fleet* fleet, int32_t n_cases, const double* pose_f, const double* params, const uint64_t* seed,
                               const uint32_t* tick, const int32_t* obj_off, const double* objs, int32_t* cause, double* u);

/* ------------------------------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- OBJECT TRACKER: a per-planner multi-object tracker with memory from tick to tick, run on the device inside
 * ltpl_fleet_sim_run (csrc/fleet_sim.hpp: k_fleet_sim_track; the rule: csrc/fleet_track.hpp). It closes the perception chain
 * truth -> noise -> sensor -> tracker -> planner: a new object is reported after n_confirm detections, a tracked object that is lost for
 * up to n_coast ticks is coasted on, the reported position and speed are filtered. Off by default.
 * ARITHMETIC: fp64, + - * and comparisons only, one fixed order (the library is built with -ffp-contract=off): the host mirror
 * sim.TrackerModel and the device agree to the last bit. The one division, adv = dt / 0.2 (dt of ltpl_fleet_sim_setup over the prediction
 * horizon of the object ingestion), is formed once per call.
 * PER PLANNER p AND TICK: the detections k = 0 .. K - 1 are the staged on-track list as it stands behind the sensor model (or behind the
 * ingestion and the mates): x, y (perceived), e = (px - x, py - y) the ingestion's displacement over 0.2 s, r, v. The planner's table holds
 * T <= C_p = min(96, 2 S_p) tracks of LTPL_FLEET_SIM_TRACK_DOUBLES doubles, S_p the planner's staging slots (opponents + statics + mates):
 *   [0] x  [1] y  [2] ex  [3] ey  [4] r  [5] v  [6] id  [7] hits  [8] miss  [9] born_tick
 *   | # | step      | rule                                                                                                          |
 *   | 1 | predict   | xp = x + adv ex, yp = y + adv ey (the product first, then the sum)                                            |
 *   | 2 | associate | d2(t, k) = dx dx + dy dy, dx = x_k - xp_t, dy = y_k - yp_t; candidates d2 <= gate gate, taken in ascending     |
 *   |   |           | (d2, t, k); accepted when neither its track nor its detection was accepted before (greedy nearest neighbour) |
 *   | 3 | update    | matched: x = x_k + w_pos (xp - x_k), y likewise; ex = e_kx + w_vel (ex - e_kx), ey and v likewise; r = r_k;    |
 *   |   |           | hits += 1; miss = 0. w = 0: the track is exactly the detection                                                 |
 *   | 4 | miss      | unmatched: hits < n_confirm: deleted (a tentative track does not survive a miss); else miss += 1;             |
 *   |   |           | miss > n_coast: deleted; else x = xp, y = yp, the rest kept (coasting)                                         |
 *   | 5 | births    | unmatched detections in ascending k, while the table holds fewer than C_p tracks: the detection's values,      |
 *   |   |           | id = next_id++ (per planner, from 0; never reused), hits = 1, miss = 0, born_tick = the tracker tick;          |
 *   |   |           | otherwise counted as overflow                                                                                  |
 *   | 6 | order     | the surviving old tracks in their previous order, then the births in detection order                          |
 *   | 7 | hand on   | the confirmed tracks (hits >= n_confirm) matched or born this tick in table order, then the confirmed         |
 *   |   |           | coasting tracks in table order until S_p objects are handed on (the rest: withheld). matched + born <= K      |
 *   |   |           | <= S_p: a live detection is never withheld. Object: x, y, x + ex, y + ey, r, v                                 |
 * The tracker tick = tick0 + the fleet ticks run since the call (it advances whether or not a planner is live). A planner that is not live
 * is skipped: its table is untouched.
 * STATISTICS per planner, LTPL_FLEET_SIM_TRACKER_DOUBLES doubles, updated in every tick in which the planner is live:
 *   [0] ticks  [1] n_det  [2] n_matched  [3] n_born  [4] n_confirmed: tracks reaching n_confirm  [5] n_del_tentative  [6] n_del_coast
 *   [7] n_out: objects handed on  [8] n_out_coast: coasting ones among them  [9] n_withheld  [10] n_overflow  [11] tracks_max
 * IN THE TICK: behind k_fleet_sim_sense (or telemetry / the mates), in front of k_fleet_sim_offsets, only while a tracker is set. Telemetry,
 * LTPL_SIM_WHEN_OPP_WITHIN and the mates keep acting on truth; offsets, compaction, the planner and the flight recorder see what the
 * tracker hands on: the count of the tick and trace fields [5] .. [7] describe that list (NaN for an empty one).
 *   | call                          | tracker                                                                                      |
 *   | ltpl_fleet_sim_setup          | switched off                                                                                 |
 *   | ltpl_fleet_sim_race           | (before the first run only) configuration kept, tables allocated for the new slot counts,    |
 *   |                               | empty                                                                                        |
 *   | ltpl_fleet_sim_snapshot       | table, track count and next_id are STATE: taken while a tracker is set; with the tracker off |
 *   |                               | the snapshot is what it was before                                                           |
 *   | ltpl_fleet_sim_branch         | a destination with a tracker takes table and next_id of a source that held tracker state (a  |
 *   |                               | live planner while the tracker is set, a snapshot entry taken with one); a source without    |
 *   |                               | empties the destination's table and sets next_id 0 (the start state); more tracks than the   |
 *   |                               | destination's C_p: refused. Configuration and statistics stay the destination's own          |
 *   | ltpl_fleet_sim_events         | no event kind sets it                                                                        |
 *   | ltpl_fleet_sim_record / trace | the objects and fields [5] .. [7] are the list handed on                                     |
 * LIMITS: coasting is straight-line along the last filtered displacement; a coasted position is not tested against the track bounds;
 * velocity and displacement come from the object list, not from position differences; no track merging or splitting.
 * THE CALL: after ltpl_fleet_sim_setup at any time between runs; in == NULL switches it off: the tick then launches the kernels it launched
 * before. Every argument is checked before the first HIP call, the message names the argument: every array present; gate finite and
 * > 0; w_pos, w_vel in [0, 1); n_confirm in 1 .. 255; n_coast in 0 .. 255; tick0 >= 0. Everything new is allocated before anything old
 * is freed: a failing call keeps the previous tracker with its tables. A successful call starts with empty tables, next_id 0 and fresh
 * statistics.
 * ------------------------------------------------------------------------------------------------------------------------------------------ */
#define LTPL_FLEET_SIM_TRACK_DOUBLES 10
#define LTPL_FLEET_SIM_TRACKER_DOUBLES 12
typedef struct {
    const double* gate;              /* [n] m, finite, > 0 (every array is needed)                  */
    const double* w_pos;             /* [n] weight of the prediction in the position update, [0, 1) */
    const double* w_vel;             /* [n] the same for displacement and speed, [0, 1)             */
    const int32_t* n_confirm;        /* [n] detections until a track is handed on, 1 .. 255          */
    const int32_t* n_coast;          /* [n] ticks a confirmed track is coasted on, 0 .. 255          */
    int32_t tick0;                   /* >= 0: the tracker tick of the next fleet tick               */
} ltpl_fleet_sim_tracker_in;
int ltpl_fleet_sim_tracker(ltpl_fleet* fleet, const ltpl_fleet_sim_tracker_in* in);
/* rec_out: [n][LTPL_FLEET_SIM_TRACKER_DOUBLES], all planners. n_sel > 0: the tables of the planners sel_planners[n_sel] into
 * tracks_out[n_sel][96][LTPL_FLEET_SIM_TRACK_DOUBLES] (unused rows NaN) and their track counts into n_tracks_out[n_sel]. No simulation, the
 * tracker off, a wrong record size or a planner index out of range: LTPL_ERR_INVALID_ARG. */
int ltpl_fleet_sim_tracker_read(ltpl_fleet* fleet, double* rec_out, int32_t doubles_per_planner, int32_t n_sel, const int32_t* sel_planners,
                                double* tracks_out, int32_t* n_tracks_out);
/* the test hook of the rule (k_fleet_sim_tracker_eval, one wave per case, the tick's own device functions): case q has params[q][5] = gate,
 * w_pos, w_vel, n_confirm, n_coast (checked as above), adv[q], tick[q], cap_slots[q][2] = C, S (0 .. 96 each), the table
 * tracks[trk_off[q] .. trk_off[q + 1])[10] (0 .. C rows), next_id[q] and the detections dets[det_off[q] .. det_off[q + 1])[6] = x, y, px, py,
 * r, v (0 .. S of them). Out: tracks_out[q][96][10] (unused rows NaN), n_tracks_out[q], next_id_out[q], the list handed on out[q][96][6]
 * (n_out[q] rows; the rest 0), assign[i] per detection: the id of the matched track, -1 unmatched (a track was born from it), -2 overflow;
 * rec[q][12]: the counters of this one step. Needs a fleet, no simulation. */
int ltpl_fleet_sim_tracker_eval(ltpl_fleet* fleet, int32_t n_cases, const double* params, const double* adv, const uint32_t* tick,
                                const int32_t* cap_slots, const int32_t* trk_off, const double* tracks, const double* next_id,
                                const int32_t* det_off, const double* dets, double* tracks_out, int32_t* n_tracks_out, double* next_id_out,
                                double* out, int32_t* n_out, int32_t* assign, double* rec);

/* ------------------------------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- PREDICTION MODEL: a per-planner multi-point prediction of the objects a planner is handed, run on the device inside
 * ltpl_fleet_sim_run (csrc/fleet_sim.hpp: k_fleet_sim_predict; the rule: csrc/fleet_predict.hpp). The simulation's ingestion gives every
 * object two positions, its own and one constant-velocity point 0.2 s ahead ("(at least) ... for delay comp.", ObjectListInterface.py:121-127);
 * the reference expects a real prediction in object_el['prediction'], the path kernel blocks lattice edges against every position of a
 * vehicle and takes the closest object from its LAST one. With the model set every object is handed on with 1 + K positions: its own and K
 * predicted points over `horizon` seconds. It is the last link of truth -> noise -> sensor -> tracker -> prediction -> planner. Off by default.
 * ARITHMETIC: fp64, + - * / sqrt and comparisons only, one fixed order (the library is built with -ffp-contract=off): the host mirror
 * sim.PredictorModel and the device agree to the last bit.
 * PER OBJECT: x, y, the ingestion's point px, py and the speed v as staged for the planner this tick (behind sensor and tracker). PER
 * PLANNER: mode, horizon T [s], relax, d_max [m]. FLEET-WIDE: K = n_points and the simulation's race-line table S = s_rl, X, Y (n rows).
 * Point j = 1 .. K belongs to the time t_j = (T j) / K.
 *   | mode | points                                                                                                                  |
 *   | 0    | as ingested: every point is (px, py). The planner computes what it computes without the model: the mask sees the same   |
 *   |      | positions and the last position is the same point                                                                       |
 *   | 1    | straight line: c_j = t_j / 0.2; (x + (px - x) c_j, y + (py - y) c_j)                                                    |
 *   | 2    | along the track: (1) i* = the first table row with the smallest (X_i - x)^2 + (Y_i - y)^2; (2) of the segments           |
 *   |      | (i* - 1, i*) and (i*, i* + 1) -- no wrap at the table's ends, a segment of length 0 is skipped -- the one whose foot point |
 *   |      | (t clamped to [0, 1]) is nearer, ties to the lower: s0 = S_a + t (S_b - S_a), signed offset d = (ex (y - Y_a) - ey (x - X_a)) |
 *   |      | / sqrt(ex ex + ey ey); (3) s_j = s0 + v t_j, minus S[n - 1] once if s_j >= S[n - 1] (a wrap, as the opponents wrap);     |
 *   |      | X(s_j), Y(s_j) = np.interp on the segment of s_j, clamped at both ends as the opponents' evaluation is; (ux, uy) the     |
 *   |      | unit direction of that segment (the first below S[0], the last at or above the end); d_j = d (1 - relax (j / K)); the    |
 *   |      | point is (X(s_j) - d_j uy, Y(s_j) + d_j ux) (without the offset on a segment of length 0); (4) mode 1 instead when there |
 *   |      | is no candidate segment, when |d| > d_max (equality stays), or when (px - x) ex + (py - y) ey < 0 on the chosen segment  |
 *   |      | (the object moves against the track), tested in this order                                                              |
 * In modes 1 and 2 an object with !(v > 0) gets K copies of (px, py). The full definition: the comment of csrc/fleet_predict.hpp.
 * STATISTICS per planner, LTPL_FLEET_SIM_PREDICTOR_DOUBLES doubles, updated in every tick in which the planner is live:
 *   [0] ticks  [1] n_obj: objects predicted  [2] n_ingested (mode 0)  [3] n_still  [4] n_straight_mode (mode 1)  [5] n_straight_dmax
 *   [6] n_straight_dir  [7] n_straight_noseg  [8] n_track: along the track  [9] d_abs_max: the largest |d| used along the track
 *   [10] n_wrap: points that wrapped
 * IN THE TICK: k_fleet_sim_predict is launched INSTEAD of k_fleet_sim_compact, behind k_fleet_sim_offsets, only while a predictor is set:
 * a fleet that never calls this entry point launches the kernels it launched before. The tick's object arrays then hold 1 + K positions
 * per object (pos_off[v] = (1 + K) v).
 *   | call                          | predictor                                                                                    |
 *   | ltpl_fleet_sim_setup          | switched off                                                                                 |
 *   | ltpl_fleet_sim_race           | configuration and records kept; the staging is allocated for the new slot counts at 1 + K     |
 *   |                               | positions; refused with LTPL_ERR_CAPACITY, everything left as it was, when the new slot counts |
 *   |                               | break the bound below                                                                        |
 *   | snapshot / branch / events    | untouched: the predictor is configuration plus statistics, not state; no event kind sets it  |
 *   | telemetry                     | keeps measuring on truth                                                                     |
 *   | ltpl_fleet_sim_record         | the record's objects show own position and point 1; the record format is unchanged           |
 * CAPACITY: the path kernel's per-position arrays hold 192 entries and the simulation hands its objects on without the per-call check, so
 * the call is refused with LTPL_ERR_CAPACITY unless slots_p (1 + K) <= 192 for every planner, slots_p = opponents + statics + mates.
 * KNOWN CONSEQUENCE: the planner's closest object is decided at the LAST position of every vehicle (the reference's rule for any supplied
 * prediction), so with a long horizon it is decided at the far end of the prediction: which car a `follow` job follows may change.
 * THE CALL: after ltpl_fleet_sim_setup at any time between runs; in == NULL switches it off and restores the two-position layout. Every
 * argument is checked before the first HIP call, the message names the argument: n_points in 1 .. 8; every array present; mode 0, 1 or 2;
 * horizon finite and > 0; relax in [0, 1]; d_max >= 0 (+inf allowed); the capacity bound. Everything new is allocated before anything old is
 * freed: a refused or failing call keeps the previous predictor and its records. A successful call starts fresh records.
 * ------------------------------------------------------------------------------------------------------------------------------------------ */
#define LTPL_FLEET_SIM_PREDICTOR_DOUBLES 11
#define LTPL_FLEET_SIM_PREDICTOR_MAX_POINTS 8
typedef struct {
    int32_t n_points;                /* K, 1 .. 8: predicted points per object, fleet-wide            */
    const int32_t* mode;             /* [n] 0 as ingested, 1 straight line, 2 along the track         */
    const double* horizon;           /* [n] s, finite, > 0                                            */
    const double* relax;             /* [n] share of the lateral offset given up by the last point, [0, 1] */
    const double* d_max;             /* [n] m, >= 0, +inf allowed: beyond it an object is predicted straight */
} ltpl_fleet_sim_predictor_in;
int ltpl_fleet_sim_predictor(ltpl_fleet* fleet, const ltpl_fleet_sim_predictor_in* in);
/* out: [n][LTPL_FLEET_SIM_PREDICTOR_DOUBLES]. No simulation, the predictor off or a wrong record size: LTPL_ERR_INVALID_ARG. */
int ltpl_fleet_sim_predictor_read(ltpl_fleet* fleet, double* out, int32_t doubles_per_planner);
/* the test hook of the rule (k_fleet_sim_predictor_eval, one wave per case, the tick's own device functions, the fleet's race-line table: needs
 * ltpl_fleet_sim_setup, no predictor): case q has params[q][4] = mode, horizon, relax, d_max (checked as above) and the objects
 * objs[obj_off[q] .. obj_off[q + 1])[5] = x, y, px, py, v (0 .. 96 of them); n_points as above, the same for every case. Out:
 * points[i][1 + n_points][2] per object in case order -- own position, then the K points, the tick's layout --, outcome[i] per object: 0 as
 * ingested, 1 still, 2 straight by mode, 3 by d_max, 4 by direction, 5 without segment, 6 along the track; rec[q][11]: the counters of
 * this one evaluation. */
int ltpl_fleet_sim_predictor_eval(ltpl_fleet* fleet, int32_t n_cases, int32_t n_points, const double* params, const int32_t* obj_off,
                                  const double* objs, double* points, int32_t* outcome, double* rec);

/* ------------------------------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- BEHAVIOUR SELECTOR: a per-planner rule that scores the trajectories of the previous tick's exported set against the
 * objects the planner was handed in that tick and writes an ORDERED preference list, which the step kernel walks exactly as it walks the
 * user's list (csrc/fleet_sim.hpp: k_fleet_sim_select; the rule: csrc/fleet_select.hpp). Without it the simulation takes "the first
 * preferred key of the previous exported set" (main_std_example.py), whatever the trajectories and the objects look like. Off by default.
 * ARITHMETIC: fp64, + - * / sqrt and comparisons only, one fixed order (the library is built with -ffp-contract=off): the host mirror
 * sim.SelectorModel and the device agree to the last bit.
 * INPUTS, all of them the previous tick's: the user's preference list as the events last wrote it (the allowed set plus the tie order;
 * the rule never adds an action and never writes the list), sel_action, the exported set (rows 0 .. n - 1, n = min(rows, n_export), columns
 * s, x, y, vx), the staged object list (x, y, the ingestion's 0.2 s point, radius: what the planner perceived behind noise, sensor and
 * tracker), and PER PLANNER horizon T [s], r_ego [m], c_hard [m], c_soft [m], w_clear [1/s], w_switch [m/s].
 * An action is SCORED when it is straight, follow, left or right, stands in the user's list, is exported and has n >= 2 rows:
 *   times      t_0 = 0, t_i = t_{i-1} + (2 (s_i - s_{i-1})) / (v_i + v_{i-1}); the first row with !(v_i + v_{i-1} > 0) and every later one
 *              is unreachable (the car stands); the window: reachable rows with t_i <= T, `last` its highest
 *   pace       vbar = (s_T - s_0) / T with s_T interpolated between rows last and last + 1; (s_last - s_0) / T where the car stands;
 *              (s_last - s_0) / t_last where the trajectory ends inside the horizon (v_0 when t_last == 0)
 *   clearance  over window rows i and objects o, the object moved at constant velocity through its 0.2 s point: c = t_i / 0.2,
 *              d = sqrt((x_i - (x_o + (px_o - x_o) c))^2 + (y_i - (y_o + (py_o - y_o) c))^2) - r_o - r_ego; clear = min d (+inf
 *              without objects), ties to the lower (object, row), a NaN never wins
 *   score      J = vbar - w_clear max(0, c_soft - clear) - (action != sel_action ? w_switch : 0); UNSAFE when clear < c_hard (equality is
 *              safe) or J is NaN (then ranked with clearance -inf)
 *   order      safe actions by J descending; emergency, if listed; unsafe actions by clearance descending; every other entry (not
 *              exported, n < 2) in the user's order. Ties keep the user's order; the output is a permutation of the user's list.
 * A car with no safe option takes the emergency trajectory if its list holds it, the least bad action otherwise; c_hard = -inf switches
 * that off. Copied unchanged, record untouched: a planner with on == 0, one that has not started or has its error word set (the step
 * kernel's "straight before the first tick" rule and its E_SIM_ACTION stay), a one-entry list. The full definition: csrc/fleet_select.hpp.
 * STATISTICS per planner, LTPL_FLEET_SIM_SELECTOR_DOUBLES doubles, updated in every evaluation ("taken": the first ordered entry that is in
 * the exported set -- what the step kernel will choose):
 *   [0] ticks  [1] n_scored: actions scored  [2] n_switch: taken != sel_action  [3] n_override: taken differs from what the user's list
 *   alone gives  [4] n_unsafe: no safe action  [5] n_emergency: emergency taken  [6] .. [9] chosen_straight / _follow / _left / _right
 *   [10] clear_min: the smallest clearance of a taken scored action (+inf at the start)  [11] j_last: J of the latest taken scored action
 * IN THE TICK: k_fleet_sim_select (one wave64 per planner) runs at the head of the tick, behind the events kernels and in front of the step
 * kernel, only while a selector is set; the step and mates kernels then get the ordered lists (a buffer of the selector's own, indexed by
 * the same pref_off) in the user's place. A fleet that never calls this entry point launches the kernels it launched before.
 *   | call                          | selector                                                                                     |
 *   | ltpl_fleet_sim_setup          | switched off                                                                                 |
 *   | ltpl_fleet_sim_events         | `pref` events keep writing the USER's list; the selector runs behind them, so from that tick on|
 *   | noise / sensor / tracker      | the rule scores the staged list, i.e. what they handed on                                     |
 *   | predictor                     | not read: the rule uses the staged 0.2 s point whether or not a predictor is set             |
 *   | snapshot / branch             | parameters, ordered lists and records stay with the destination (configuration and statistics); |
 *   |                               | sel_action travels as before, and so does the staged list (count and x, y, px, py, r of its    |
 *   |                               | entries), which the selector made state: a snapshot taken and restored with the selector set   |
 *   |                               | reproduces the run. A source without a list (taken without a selector) leaves an empty one; a  |
 *   |                               | list longer than the destination's staging slots is cut to them                                |
 *   | ltpl_fleet_sim_race / _predictor | kept; they allocate the staging again, which then holds no list: the next run starts from  |
 *   |                               | empty lists (its first tick scores without objects)                                          |
 * THE CALL: after ltpl_fleet_sim_setup at any time between runs; in == NULL switches it off. Every argument is checked before the first
 * HIP call: every array present; horizon > 0; r_ego, w_clear, w_switch >= 0; no NaN anywhere (c_hard and c_soft may be infinite).
 * Everything new is allocated before anything old is freed. A successful call starts fresh records.
 * ------------------------------------------------------------------------------------------------------------------------------------------ */
#define LTPL_FLEET_SIM_SELECTOR_DOUBLES 12
typedef struct {
    const int32_t* on;               /* [n] 0: the planner keeps its list as it is                     */
    const double* horizon;           /* [n] s, > 0                                                     */
    const double* r_ego;             /* [n] m, >= 0                                                    */
    const double* c_hard;            /* [n] m: below it an action is unsafe (-inf: never)              */
    const double* c_soft;            /* [n] m: below it clearance costs w_clear per metre              */
    const double* w_clear;           /* [n] 1/s, >= 0                                                  */
    const double* w_switch;          /* [n] m/s, >= 0: what leaving the previous action costs          */
} ltpl_fleet_sim_selector_in;
int ltpl_fleet_sim_selector(ltpl_fleet* fleet, const ltpl_fleet_sim_selector_in* in);
/* out: [n][LTPL_FLEET_SIM_SELECTOR_DOUBLES]; ordered (or NULL): the current ordered lists, n_ordered = pref_off[n] entries laid out as the
 * user's preference lists are. No simulation, the selector off, a wrong record size or a wrong n_ordered: LTPL_ERR_INVALID_ARG. */
int ltpl_fleet_sim_selector_read(ltpl_fleet* fleet, double* out, int32_t doubles_per_planner, int32_t* ordered, int32_t n_ordered);
/* the test hook of the rule (k_fleet_sim_selector_eval, one wave per case, the tick's own device functions; needs no simulation): case q
 * has params[q][6] = horizon, r_ego, c_hard, c_soft, w_clear, w_switch (checked as above), lists[q][8] = n_pref (1 .. 5), sel_action,
 * emergency exported (0 / 1) and the user's entries (LTPL_ACT_* 0 .. 4), n_rows[q][4] per action straight .. right (-1: not exported,
 * else 0 .. 256), rows[q][4][4][256] = per action the columns s, x, y, vx, and the objects objs[obj_off[q] .. obj_off[q + 1])[5] = x, y,
 * px, py, r (0 .. 96). Out: ordered[q][5] (the first n_pref entries), act_d[q][4][3] = vbar, clear, J, act_i[q][4][2] = clear_obj (-1:
 * none), flags (1 scored, 2 unsafe, 4 NaN score, 8 exported); rec[q][12]: IN the record before, OUT the record after this evaluation
 * (unlike the tick, the hook evaluates a one-entry list too). */
int ltpl_fleet_sim_selector_eval(ltpl_fleet* fleet, int32_t n_cases, const double* params, const int32_t* lists, const int32_t* n_rows,
                                 const double* rows, const int32_t* obj_off, const double* objs, int32_t* ordered, double* act_d, int32_t* act_i,
                                 double* rec);

/* ------------------------------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- SAFETY MONITOR: surrogate safety measures per planner and tick -- time to collision, time exposed below a TTC
 * threshold, required deceleration, time headway, impact speed -- accumulated into a record, plus a log of the near misses (csrc/fleet_sim.hpp:
 * k_fleet_sim_safety; the rule: csrc/fleet_safety.hpp). Telemetry's clear_min and contact_ticks are distances and blind to time; this says
 * how fast the gap was closing and WHEN, so that the flight recorder and a snapshot can be pointed at the tick. MEASUREMENT ONLY: no kernel
 * of the tick reads what it writes. Off by default.
 * ARITHMETIC: fp64, + - * / sqrt and comparisons only, one fixed order (the library is built with -ffp-contract=off), no trigonometry: the
 * host mirror sim.SafetyModel and the device agree to the last bit.
 * INPUTS of planner p in a tick in which it is live: the TRUE pose P = (px, py) behind the step and mates kernels; dt; the monitor's tick
 * index (tick0 + fleet ticks since the call: like the noise's it advances whether or not the planner is live); the staged on-track list --
 * what telemetry reads, in FRONT of sensor and tracker: an object the sensor hides is still measured -- per object position X (the noise's
 * TRUE position while noise is on), the ingestion's 0.2 s point Q, radius r_o; PER PLANNER on (0 / 1), r_ego >= 0 [m], ttc_thr > 0 [s],
 * drac_thr >= 0 [m/s^2], thw_thr >= 0 [s], margin >= 0 [m], all finite.
 *   | step        | rule                                                                                                              |
 *   | ego velocity| W = ((px - prev_x) / dt, (py - prev_y) / dt) from the pose of the previous live tick (the record keeps it): the      |
 *   |             | displacement the car really made, whatever drives it. A live tick WITHOUT a valid previous pose (the first after    |
 *   |             | the call, the first after a branch from a source without a record) counts in ticks, moves the gap fields and        |
 *   |             | overlap_ticks with W = (0, 0) and stores the pose; nothing else moves. Every other live tick is EVALUATED           |
 *   | 1           | ux = (qx - ox) / 0.2, uy = (qy - oy) / 0.2                                                                          |
 *   | 2           | rx = ox - px, ry = oy - py; vx = ux - wx, vy = uy - wy                                                              |
 *   | 3           | rr = rx rx + ry ry; dist = sqrt(rr)                                                                                 |
 *   | 4           | gap = (dist - r_o) - r_ego  (gap_min == telemetry's clear_min - r_ego bit for bit)                                  |
 *   | 5           | rho = r_o + r_ego; c = rr - rho rho; b = rx vx + ry vy; a = vx vx + vy vy                                           |
 *   | 6           | rr, a, b or r_o not finite: the object is SKIPPED -- counted, takes part in nothing                                 |
 *   | 7           | overlap = !(gap > 0)                                                                                                |
 *   | 8           | closing = b < 0 ? (-b) / dist : 0; with dist == 0: sqrt(a)                                                          |
 *   | 9  TTC      | 0 when overlap or !(c > 0); else on a COLLISION COURSE (b < 0 and disc = b b - a c >= 0): c / (sqrt(disc) - b);      |
 *   |             | else +inf  (two discs at constant velocity)                                                                         |
 *   | 10 DRAC     | (closing closing) / (2 gap) when not overlapping and on a collision course, else 0                                  |
 *   | 11 headway  | w2 = wx wx + wy wy, wn = sqrt(w2); with wn > 0: lon = (rx wx + ry wy) / wn, lat = (rx wy - ry wx) / wn; IN THE       |
 *   |             | CORRIDOR when lon > 0 and |lat| <= rho + margin: thw = (lon - rho) / wn, 0 when !(lon - rho > 0); otherwise, and      |
 *   |             | with wn == 0, +inf                                                                                                  |
 *   | per tick    | gap_t, ttc_t: minima on the key (value, slot), ties to the lower slot, a NaN never wins, slot -1 without an object;  |
 *   |             | drac_t a maximum (from 0); thw_t a minimum; overlap_t any overlap; impact_t the largest closing over the overlapping |
 *   |             | objects, closing_t over all (from 0); skipped_t a count                                                             |
 * THE RECORD, LTPL_FLEET_SIM_SAFETY_DOUBLES doubles: [0] ticks (live ticks seen) [1] ticks_eval [2] prev_x [3] prev_y [4] prev_valid
 *   [5] gap_min [6] gap_tick [7] gap_slot (strictly smaller replaces) [8] ttc_min [9] ttc_tick [10] ttc_slot (strictly smaller replaces)
 *   [11] tet += dt on a tick with ttc_t < ttc_thr [12] tit += (ttc_thr - ttc_t) dt on the same ticks [13] drac_max [14] drac_tick (strictly
 *   larger replaces) [15] drac_ticks: ticks with drac_t > drac_thr [16] thw_min [17] thw_ticks: ticks with thw_t < thw_thr [18] overlap_ticks
 *   [19] impact_max [20] n_skipped [21] n_incidents [22] inc_open [23] .. [30] hist: an evaluated tick goes into the first bin j in 0 .. 6
 *   with ttc_t < (ttc_thr (j + 1)) / 7, else bin 7 (+inf: bin 7). The gap fields and overlap_ticks move on every live tick, everything else
 *   on evaluated ticks only. Start state: zeros, gap_min = ttc_min = thw_min = +inf.
 * THE INCIDENT LOG: a ring of LTPL_FLEET_SIM_SAFETY_INCIDENTS entries of LTPL_FLEET_SIM_SAFETY_INCIDENT_DOUBLES doubles per planner:
 *   tick_first, tick_last, ttc_min, slot, gap_min, closing_max; unwritten entries are NaN. An incident OPENS on an evaluated tick with
 *   ttc_t < ttc_thr while inc_open == 0: n_incidents += 1 and entry (n_incidents - 1) mod 8 is set from this tick. While it is open and
 *   ttc_t < ttc_thr: tick_last moves, a strictly smaller ttc_t replaces ttc_min and slot, gap_min takes the minimum, closing_max the
 *   maximum. The first evaluated tick with !(ttc_t < ttc_thr) closes it. An overlap has TTC 0: every contact is an incident.
 * IN THE TICK: k_fleet_sim_safety (one wave64 per planner, registers only) runs behind k_fleet_sim_tele / k_fleet_sim_rank and in front of
 * k_fleet_sim_sense, only while a monitor is set; a planner that is not live or has on == 0 returns at once. A fleet that never calls this
 * entry point launches the kernels it launched before, with the same arguments.
 *   | with                          | what happens                                                                                 |
 *   | ltpl_fleet_sim_setup          | switched off                                                                                 |
 *   | noise                         | positions are the TRUE ones; the 0.2 s displacement Q - (staged x, y) is the PERCEIVED one (the |
 *   |                               | staging holds no true heading: a limit): the rule is handed Q = X_true + (Q_staged - X_staged), |
 *   |                               | so the position error itself never enters the object's velocity                              |
 *   | sensor / tracker / predictor / selector | not read: the monitor measures the staged list in front of them                    |
 *   | races                         | mates are staged behind the own objects and measured like them                               |
 *   | telemetry                     | independent: either can be on alone                                                          |
 *   | snapshot / branch             | record and ring are what the tick writes: they TRAVEL (k_fleet_sim_branch_safety behind        |
 *   |                               | k_fleet_sim_branch); parameters stay the destination's. A snapshot taken with the monitor on   |
 *   |                               | holds them; a source without a record (a snapshot taken with the monitor off) leaves the       |
 *   |                               | destination the start state with prev_valid = 0. Snapshot, run, restore,                       |
 *   |                               | ltpl_fleet_sim_safety(KEEP_STATE, tick0 = the snapshot's tick), run reproduces record and ring |
 *   | events                        | no new kind                                                                                  |
 *   | ltpl_fleet_sim_race / _predictor | kept: the kernel reads the staging through the pointers of the launch                      |
 *   | a failed planner              | skipped; its record stays                                                                    |
 * THE CALL: after ltpl_fleet_sim_setup at any time between runs; in == NULL clears the monitor. Every argument is checked before the first
 * HIP call: every array present, on 0 or 1, the parameters as above, tick0 >= 0, no unknown flag. Everything new is allocated before
 * anything old is freed; a failed call keeps the previous monitor. A successful call starts fresh records and rings -- with
 * LTPL_SIM_SAFETY_KEEP_STATE (and a monitor set) parameters, mask and tick0 change and records and rings stay.
 * ------------------------------------------------------------------------------------------------------------------------------------------ */
#define LTPL_FLEET_SIM_SAFETY_DOUBLES 31
#define LTPL_FLEET_SIM_SAFETY_INCIDENTS 8
#define LTPL_FLEET_SIM_SAFETY_INCIDENT_DOUBLES 6
#define LTPL_SIM_SAFETY_KEEP_STATE 1u
typedef struct {
    const int32_t* on;               /* [n] 0: the planner is not monitored, 1: it is                  */
    const double* r_ego;             /* [n] m, >= 0                                                    */
    const double* ttc_thr;           /* [n] s, > 0                                                     */
    const double* drac_thr;          /* [n] m/s^2, >= 0                                                */
    const double* thw_thr;           /* [n] s, >= 0                                                    */
    const double* margin;            /* [n] m, >= 0: widens the headway corridor                       */
    int32_t tick0;                   /* >= 0: the monitor's tick of the next fleet tick                */
    uint32_t flags;                  /* LTPL_SIM_SAFETY_KEEP_STATE                                     */
} ltpl_fleet_sim_safety_in;
int ltpl_fleet_sim_safety(ltpl_fleet* fleet, const ltpl_fleet_sim_safety_in* in);
/* out: [n][LTPL_FLEET_SIM_SAFETY_DOUBLES]; incidents (or NULL): [n][LTPL_FLEET_SIM_SAFETY_INCIDENTS][LTPL_FLEET_SIM_SAFETY_INCIDENT_DOUBLES].
 * No simulation, the monitor off, a wrong record or incident size: LTPL_ERR_INVALID_ARG. */
int ltpl_fleet_sim_safety_read(ltpl_fleet* fleet, double* out, int32_t doubles_per_planner, double* incidents, int32_t doubles_per_incident);
/* the test hook of the rule (k_fleet_sim_safety_eval, one wave per case, the tick's own device function; needs a fleet and no simulation):
 * case q is one live tick at pose[q][2] with dt[q] > 0, tick[q] >= 0, params[q][5] = r_ego, ttc_thr, drac_thr, thw_thr, margin (checked as
 * above) and the objects objs[obj_off[q] .. obj_off[q + 1])[5] = x, y, px, py, r (0 .. 96). rec[q][31] and inc[q][8][6]: IN the record and
 * ring before (prev_x, prev_y, prev_valid decide whether the tick is evaluated), OUT after. per_obj[..][6] = ttc, drac, thw, gap, closing,
 * flags (1 skipped, 2 overlap, 4 collision course, 8 in corridor); per_tick[q][8] = gap_t, gap_slot, ttc_t, ttc_slot, drac_t, thw_t,
 * impact_t, closing_t. */
int ltpl_fleet_sim_safety_eval(ltpl_fleet* fleet, int32_t n_cases, const double* pose, const double* dt, const int32_t* tick, const double* params,
                               const int32_t* obj_off, const double* objs, double* rec, double* inc, double* per_obj, double* per_tick);

/* ------------------------------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- REACTIVE OPPONENTS: a car-following rule for the race-line opponents of the simulation (csrc/fleet_sim.hpp:
 * k_fleet_sim_react; the rule: csrc/fleet_react.hpp). Without it every opponent integrates vel_rl(s) * vel_scale and sees nothing: a faster
 * one drives through a slower one and through the ego from behind, contacts no planner could have avoided. With it every opponent keeps
 * an EFFECTIVE scale e_q in [0, c_q] under its configured vel_scale c_q, decided at the head of every tick from the car ahead of it on the
 * race line -- another opponent or the ego -- and the step kernels integrate vel_rl(s) * e_q. Off by default.
 * ARITHMETIC: fp64, + - * / sqrt and comparisons only, one fixed order (the library is built with -ffp-contract=off), no pow, no
 * trigonometry: the host mirror sim.ReactModel / sim.react_tick and the device agree to the last bit.
 * INPUTS of planner p at the head of a tick: the TRUE pose pos_x / pos_y and speed vel the previous tick left (never the noise's estimate);
 * dt; the model's tick index (tick0 + fleet ticks since the call: it advances whether or not the planner is live); the race table S, X, Y,
 * V (columns 0, 1, 2, 4 of ltpl_fleet_sim_in::race), lap length L = S[n - 1]; per opponent s_q (opp_s), c_q (vel_scale as the events left
 * it), e_q, l_q (length). PER PLANNER, all finite unless noted: on (0 / 1), a_max > 0, b_comf > 0, b_max > 0 [m/s^2], headway >= 0 [s],
 * gap0 >= 0 [m], look > 0 [m] (+inf allowed), lat_gate >= 0 [m], ego_len >= 0 [m].
 *   | step      | rule                                                                                                                |
 *   | 0 ego     | the ego on the race line by steps 1 and 2 of the prediction model (nearest row, the better of its two segments):      |
 *   |           | (s_e, d_e), or nothing without a candidate segment. A possible leader iff a projection exists and |d_e| <= lat_gate   |
 *   |           | (equality inside, a NaN outside)                                                                                      |
 *   | first     | Vq = np.interp of V at s_q. !(c_q > 0) or !(Vq > 0): PASSIVE -- e' = c_q, counted, steps 1 .. 5 skipped; as a leader  |
 *   |           | of others its speed is c_q Vq                                                                                         |
 *   | 1         | v_q = e_q Vq                                                                                                          |
 *   | 2 leader  | candidates in the order ego, opponents r = 0 .. no - 1 (r != q): D = s_j - s_q, D < 0: D = D + L; against an opponent   |
 *   |           | with D == 0: r < q is ahead at 0, r > q a lap ahead (D = L). Only a strictly smaller D replaces (the ego wins ties,   |
 *   |           | then the lower index; a NaN never wins). No leader unless D <= look. Leader's speed u and length l_j: the ego's       |
 *   |           | (vel, ego_len), opponent r's (e_r V(s_r), l_r) with e_r of the START of the tick                                      |
 *   | 3         | gap = (D - 0.5 l_j) - 0.5 l_q                                                                                         |
 *   | 4 acc     | r = e_q / c_q; free = 1 - (r r)(r r). No leader: a_max free. Leader and !(gap > 0): -b_max (an OVERLAP). Otherwise    |
 *   |           | dv = v_q - u; z = v_q headway + (v_q dv) / (2 sqrt(a_max b_comf)), !(z > 0): 0; k = (gap0 + z) / gap;                 |
 *   |           | acc = a_max (free - k k). Then acc < -b_max: -b_max (CLAMPED, counted); acc > a_max: a_max                            |
 *   | 5         | e' = e_q + (acc dt) / Vq; !(e' > 0): 0; e' > c_q: c_q                                                                 |
 * Every opponent reads the values of the start of the tick: the result does not depend on the order of evaluation. An opponent with no
 * leader and e == c keeps e exactly (r = 1, free = 0, acc = 0, e + 0 / Vq = e): a fleet whose opponents never find a leader drives the run
 * without a model bit for bit.
 * THE RECORD, LTPL_FLEET_SIM_REACT_DOUBLES doubles: [0] ticks [1] opp_ticks (opponents x ticks) [2] follow_ticks: opponent-ticks with a
 *   leader [3] ego_lead_ticks: those whose leader is the ego [4] clamped [5] overlaps [6] passive (opponent-ticks each) [7] gap_min
 *   [8] gap_tick [9] gap_slot: the smallest gap of an opponent with a leader, its tick and the FOLLOWER's index [10] acc_min [11] acc_tick
 *   [12] acc_slot: the smallest acc of an opponent that is not passive [13] ego_gap_min [14] ego_gap_tick: the smallest gap behind the ego
 *   [15] ego_outside: ticks with a projection outside the gate. Minima replace when strictly smaller, ties go to the lower slot, a NaN
 *   never wins. Start state: zeros, +inf in the minima, -1 in their ticks and slots.
 * IN THE TICK: k_fleet_sim_react (one wave64 per planner, 2.3 KB of LDS) runs behind the events kernels and k_fleet_sim_select and in
 * front of the step kernel, only while a model is set; the step kernels then read the effective scales where they read vel_scale. A
 * planner whose error word is set returns at once (scales and record stay); one with on == 0 hands on its configured scales and does
 * nothing else. A fleet that never calls this entry point launches the kernels it launched before, with the same arguments.
 *   | with                          | what happens                                                                                 |
 *   | ltpl_fleet_sim_setup          | switched off                                                                                 |
 *   | events                        | LTPL_SIM_SET_OPP_VEL_SCALE writes c; e follows by the rule from that tick on (down at once by  |
 *   |                               | the clamp e <= c, up at a_max). No new event kind                                             |
 *   | noise / vehicle model         | the opponents react to the TRUE pose and speed                                               |
 *   | sensor / tracker / predictor / selector / telemetry / safety / recorder | untouched: they read the staging              |
 *   | snapshot / branch             | effective scales and record are what the tick writes: they TRAVEL (k_fleet_sim_branch_react    |
 *   |                               | behind k_fleet_sim_branch); parameters and tick0 stay the destination's. A destination fleet   |
 *   |                               | without a model takes nothing; a source without state (a snapshot taken with the model off)    |
 *   |                               | leaves the destination the start state, e = its own c. Snapshot, run, restore,                 |
 *   |                               | ltpl_fleet_sim_react(KEEP_STATE, tick0 = the snapshot's tick), run reproduces scales, records, |
 *   |                               | trace and state bit for bit                                                                  |
 *   | ltpl_fleet_sim_race / _predictor | kept                                                                                      |
 *   | a failed planner              | skipped; scales and record stay                                                              |
 * LIMITS: statics and race mates are no leaders; no lateral moves, no blue flags; parameters per planner, not per opponent; no event
 * writes the model's parameters; the opponents see the truth, never a noisy view.
 * THE CALL: after ltpl_fleet_sim_setup at any time between runs; in == NULL or on == 0 for every planner switches the model off. Every
 * argument is checked before the first HIP call: every array present, on 0 or 1, the parameters as above, tick0 >= 0, no unknown flag.
 * Everything new is allocated before anything old is freed; a failed call keeps the previous model. A successful call starts from e = c
 * and fresh records -- with LTPL_SIM_REACT_KEEP_STATE (and a model set) parameters and tick0 change and scales and records stay.
 * ------------------------------------------------------------------------------------------------------------------------------------------ */
#define LTPL_FLEET_SIM_REACT_PARAMS 9
#define LTPL_FLEET_SIM_REACT_DOUBLES 16
#define LTPL_SIM_REACT_KEEP_STATE 1u
typedef struct {
    const int32_t* on;               /* [n] 0: the planner's opponents drive their configured scale, 1: they react */
    const double* a_max;             /* [n] m/s^2, > 0: acceleration back to the configured speed      */
    const double* b_comf;            /* [n] m/s^2, > 0: comfortable deceleration                       */
    const double* b_max;             /* [n] m/s^2, > 0: hardest deceleration                           */
    const double* headway;           /* [n] s, >= 0                                                    */
    const double* gap0;              /* [n] m, >= 0: gap at standstill                                 */
    const double* look;              /* [n] m, > 0, +inf allowed: how far ahead a leader is looked for */
    const double* lat_gate;          /* [n] m, >= 0: the ego leads only within this distance of the race line */
    const double* ego_len;           /* [n] m, >= 0                                                    */
    int32_t tick0;                   /* >= 0: the model's tick of the next fleet tick                  */
    uint32_t flags;                  /* LTPL_SIM_REACT_KEEP_STATE                                      */
} ltpl_fleet_sim_react_in;
int ltpl_fleet_sim_react(ltpl_fleet* fleet, const ltpl_fleet_sim_react_in* in);
/* out: [n][LTPL_FLEET_SIM_REACT_DOUBLES]; eff_scale (or NULL): the effective scales in the order of ltpl_fleet_sim_state's opp_s.
 * No simulation, the model off, a wrong record size: LTPL_ERR_INVALID_ARG. */
int ltpl_fleet_sim_react_read(ltpl_fleet* fleet, double* out, int32_t doubles_per_planner, double* eff_scale);
/* the test hook of the rule (k_fleet_sim_react_eval, one wave per case, the tick's own device function; needs a simulation, for the race
 * table): case q is one tick with params[q][9] = on, a_max, b_comf, b_max, headway, gap0, look, lat_gate, ego_len (checked as above; on is
 * not read), the ego ego[q][3] = x, y, v (any value, NaN included), dt[q] > 0, tick[q] >= 0 and the opponents
 * opp[opp_off[q] .. opp_off[q + 1])[4] = s, c, e, length (0 .. 96, finite). rec[q][16]: IN the record before, OUT after. e_out[..]: the new
 * scales; per_opp[..][4] = leader (-2 none, -1 the ego, else the index), D, gap, acc (D and gap +inf without a leader, acc 0 for a
 * passive opponent); ego_out[q][3] = s_e, d_e, has. */
int ltpl_fleet_sim_react_eval(ltpl_fleet* fleet, int32_t n_cases, const double* params, const double* ego, const double* dt, const int32_t* tick,
                              const int32_t* opp_off, const double* opp, double* rec, double* e_out, double* per_opp, double* ego_out);

/* ------------------------------------------------------------------------------------------------------------------------------------------
 * Additive to ABI v9 -- CAMPAIGN STATISTICS: chosen fields of the planners' records reduced on the device per group of planners
 * (csrc/fleet_sim.hpp: k_fleet_sim_stats_chunk / k_fleet_sim_stats_merge; the rule: csrc/fleet_stats.hpp). A fleet is one situation fanned
 * out into thousands of planners; judging it took eight _read calls (129 doubles per planner, eight stream synchronisations) and a host
 * pass. A PLAN names groups of planners and measures; ltpl_fleet_sim_stats_reduce reduces now, and with a period ltpl_fleet_sim_run reduces
 * at the tail of every period-th tick into a ring, with no host round trip. Measurement only: no kernel of the tick reads what the
 * statistics write, and the run is bit-identical with and without a plan. Off by default.
 * ARITHMETIC: fp64, + - * / and comparisons only, one fixed order (the library is built with -ffp-contract=off), no floating-point
 * atomics: the host mirror sim.stats_reduce / sim.StatsModel and the device agree to the last bit, for every launch geometry.
 * THE PLAN: n_groups G (1 .. 4096); group[p] in -1 .. G - 1 per planner (-1: in no group); the host turns it into group offsets and a
 * member list, planners ascending inside a group, uploaded once. n_measures M (1 .. 64), each a family (LTPL_SIM_STATS_*: the eight record
 * families, whose module must be on, and LTPL_SIM_STATS_STATE with its one column 0, `failed`: 1.0 when the planner's error word is set --
 * the word that makes the planner skip its ticks -- else 0.0), a column of the family's record, lo < hi (finite), bins (1 .. 16) and
 * top_dir (-1: the smallest, +1: the largest, 0: no list). top_k (0 .. 8) entries per list. period (0: no series), depth (rows of the
 * ring), tick0 (the plan's tick of the next fleet tick).
 * ONE VALUE v of member i (its position in the group) and planner p:
 *   | NaN (v != v) | counted in n_nan; takes part in nothing else                                                                   |
 *   | +-inf        | counted in n_inf; takes part in min / max / top-K and in under / over; not in n, sum, sumsq or the cells         |
 *   | finite       | n += 1, sum, sumsq (v * v), min / max, one histogram cell                                                       |
 * MINIMUM on the key (value, planner), MAXIMUM on (-value, planner): a strict compare of the values decides, ties go to the lower planner;
 * a -0.0 that ties with a +0.0 keeps the bits of the lower planner's value. An empty group: min = +inf, argmin = -1, max = -inf, argmax = -1.
 * HISTOGRAM: edges e_j = lo + ((hi - lo) * j) / bins for j = 0 .. bins, in exactly this order; under counts v < e_0, cell j counts
 * e_j <= v < e_(j+1), over counts v >= e_bins.
 * TOP-K: the K smallest (top_dir -1) or largest (+1) keys of the group, in order; a NaN never enters, an infinity may; unused entries are
 * (NaN, -1).
 * SUM ORDER of sum and sumsq: members are cut into chunks of 1024 consecutive positions; inside a chunk lane l = i mod 64 adds its
 * values serially in ascending i from +0.0 (a skipped value adds nothing); the 64 lane sums are folded by the tree t[l] = t[l] + t[l + s]
 * for l < s, s = 32, 16, 8, 4, 2, 1; the chunk sums are added serially in ascending chunk order from +0.0.
 * THE ROW, LTPL_FLEET_SIM_STATS_DOUBLES doubles: [0] n [1] n_nan [2] n_inf [3] min [4] argmin [5] max [6] argmax [7] sum [8] sumsq [9] under
 * [10] over [11 .. 26] hist (unused cells 0).
 * THE SERIES: with period > 0 ltpl_fleet_sim_run launches the two kernels at the tail of every tick whose index satisfies
 * (index + 1) % period == 0, behind every other kernel of the tick; index = tick0 + the fleet's ticks since the plan was set (it advances
 * in every tick). The rows [G][M][27] go into slot (rows written) mod depth of a ring, with the tick; no lists. A run that would reduce a
 * family that is off is refused before its first tick.
 *   | with                          | what happens                                                                                 |
 *   | ltpl_fleet_sim_setup          | the plan is cleared                                                                          |
 *   | a module set again            | the records' addresses are taken at every launch: the plan follows                           |
 *   | a module switched off         | ltpl_fleet_sim_stats_reduce and a run with a period refuse, naming the family, until the plan |
 *   |                               | is cleared or replaced or the module is back                                                 |
 *   | snapshot / branch / restore   | the plan holds no per-planner state: nothing travels, plan and series stay                   |
 *   | ltpl_fleet_sim_race / _predictor | kept                                                                                      |
 *   | events                        | no new kind                                                                                  |
 *   | a failed planner              | its records stay and are reduced like any other; STATE / failed counts or excludes them      |
 *   | a planner whose module has on == 0 | contributes its start-state record; groups are the caller's tool to leave it out       |
 * LIMITS: no quantiles beyond the histogram; one device (the rows of disjoint groups of several fleets concatenate); no event is
 * triggered by a statistic; the incident rings and the tracker's tables are not reduced.
 * THE CALL: after ltpl_fleet_sim_setup at any time between runs; in == NULL clears the plan. Every argument is checked before the first
 * HIP call, each with a message that names it; a series above 256 MiB is LTPL_ERR_CAPACITY. Everything new is allocated before anything
 * old is freed; a failed call keeps the previous plan and series. With LTPL_SIM_STATS_KEEP_SERIES (and a plan with a series set) the ring,
 * its ticks and its count stay; n_groups, n_measures and depth must then be the plan's and period > 0 (else LTPL_ERR_INVALID_ARG).
 * ------------------------------------------------------------------------------------------------------------------------------------------ */
#define LTPL_FLEET_SIM_STATS_DOUBLES 27
#define LTPL_FLEET_SIM_STATS_MAX_BINS 16
#define LTPL_FLEET_SIM_STATS_MAX_TOP 8
#define LTPL_SIM_STATS_TELEMETRY 0
#define LTPL_SIM_STATS_VEHICLE   1
#define LTPL_SIM_STATS_SENSOR    2
#define LTPL_SIM_STATS_TRACKER   3
#define LTPL_SIM_STATS_PREDICTOR 4
#define LTPL_SIM_STATS_SELECTOR  5
#define LTPL_SIM_STATS_SAFETY    6
#define LTPL_SIM_STATS_REACT     7
#define LTPL_SIM_STATS_STATE     8
#define LTPL_SIM_STATS_KEEP_SERIES 1u
typedef struct {
    int32_t n_groups;                /* G: 1 .. 4096                                                   */
    const int32_t* group;            /* [n] -1 .. G - 1                                                */
    int32_t n_measures;              /* M: 1 .. 64                                                     */
    const int32_t* family;           /* [M] LTPL_SIM_STATS_*                                           */
    const int32_t* column;           /* [M] a column of the family's record                            */
    const double* lo;                /* [M] finite, lo < hi                                            */
    const double* hi;                /* [M]                                                            */
    const int32_t* bins;             /* [M] 1 .. 16                                                    */
    const int32_t* top_dir;          /* [M] -1 / 0 / +1                                                */
    int32_t top_k;                   /* 0 .. 8                                                         */
    int32_t period;                  /* >= 0; 0: no series                                             */
    int32_t depth;                   /* >= 1 with a period                                             */
    int32_t tick0;                   /* >= 0: the plan's tick of the next fleet tick                   */
    uint32_t flags;                  /* LTPL_SIM_STATS_KEEP_SERIES                                     */
} ltpl_fleet_sim_stats_in;
int ltpl_fleet_sim_stats(ltpl_fleet* fleet, const ltpl_fleet_sim_stats_in* in);
/* reduces now: rows_out [G][M][LTPL_FLEET_SIM_STATS_DOUBLES]; top_out (or NULL) [G][M][top_k][2] = value, planner, top_k the plan's.
 * Synchronises the handle's stream. No simulation, no plan, a wrong row size or top_k, a referenced family that is off (the message
 * names it): LTPL_ERR_INVALID_ARG. */
int ltpl_fleet_sim_stats_reduce(ltpl_fleet* fleet, double* rows_out, int32_t doubles_per_row, double* top_out, int32_t top_k);
/* the ring, oldest first: ticks_out [depth], rows_out [depth][G][M][27] (both may be NULL: the counts only); *n_rows_out: the rows held,
 * *n_total_out: the rows ever written. No simulation, no plan with a period, a wrong row size: LTPL_ERR_INVALID_ARG. */
int ltpl_fleet_sim_stats_series(ltpl_fleet* fleet, int32_t* ticks_out, double* rows_out, int32_t doubles_per_row, int32_t* n_rows_out,
                                int64_t* n_total_out);
/* the test hook of the rule (k_fleet_sim_stats_eval in k_fleet_sim_stats_chunk's place: the same device functions on raw values, then
 * k_fleet_sim_stats_merge; needs a fleet and no simulation): case q (at most 4096) reduces values[val_off[q] .. val_off[q + 1]) as one
 * group and one measure with spec[q][5] = lo, hi, bins, top_dir, top_k (checked as above); planner_idx (or NULL: the position in the case)
 * gives every value its planner, 0 .. 2^31 - 2, distinct inside a case. rows_out [n_cases][27]; top_out [n_cases][8][2], entries from
 * top_k on (NaN, -1). */
int ltpl_fleet_sim_stats_eval(ltpl_fleet* fleet, int32_t n_cases, const int32_t* val_off, const double* values, const int32_t* planner_idx,
                              const double* spec, double* rows_out, double* top_out);

#ifdef __cplusplus
}
#endif
#endif /* LTPL_HIP_H */
