// ltpl_hip.hip -- MI355X (gfx950 / CDNA4) backend of the graph_ltpl online hot path. C ABI: include/ltpl_hip.h.
//
// Seam (1) lives in paths_team.hpp: a team of NW wave64s plans one scenario (NW = 1 for batches, NW = 4 for single
// ticks). Seam (2) (velocity profiles): vel_wave.hpp (one wave per profile), vel_lanes.hpp (one lane per profile); the fused tick's kernels
// live in this file, the host side of the tick in tick_host.hpp.
// The lattice (< 15 MB for Monteblanco) is uploaded once and is L2 / Infinity-Cache resident afterwards.
// Everything is IEEE fp64 and compiled with -ffp-contract=off so that masks, arg-mins and path costs are
// bit-identical to the NumPy arithmetic of the reference.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ltpl_hip.h"
#include "planner_host.hpp"
#include "fleet_api.hpp"
#include "capsule.hpp"
#include "layer_grid.hpp"
#include "assembly_records.hpp"
#include "vel_layout.hpp"

#define WG_THREADS 256
#define PIPELINE_MIN_SCEN 64   // seam (1) alone: batches from this size on use one-wave teams (nw1_min_scen). The fused tick against the batch
                               // pipeline has its own, device-dependent threshold since round 6: ltpl_handle::pipeline_min_scen
#define NUM_WAVES 4
#define MAX_POS 192      // obstacle positions (own + predicted) per scenario
#define MAX_VEH 96       // vehicles per scenario
#define NFILT 4
#define F_PR 0
#define F_DEF 1
#define F_LEFT 2
#define F_RIGHT 3
#define D_PI 3.14159265358979323846

// ---------------------------------------------------------------------------------------------------------------------
// device-side views
// ---------------------------------------------------------------------------------------------------------------------
#define LTPL_SW_PAD 512      // sentinel entries behind the sweep-order edge tables (DevLat::sw_cost / sw_meta)
struct DevLat {
    int L, V, E, S, G;
    int mode;
    int closed;                       // GraphBase.closed; open tracks: the planning range is clamped to the last layer
    double min_plan_horizon, veh_width, sampled_resolution, lat_offset, vel_decrease_lat, veh_length;
    const int* layer_off; const int* rl_idx;
    const double* s_rl; const double* ref_x; const double* ref_y; const double* vel_rl;
    const double* node_x; const double* node_y; const double* vgoal;
    const int* in_ptr; const int* edge_src; const double* edge_cost; const double* edge_len; const int* samp_ptr;
    const double* sx; const double* sy; const double* spsi; const double* slen;
    const double* ssc;                // [S][2] (sin, cos) of spsi, tabulated at ltpl_create: the spline end slopes of a path need no sincos per path
    const double* glob_rl;
    const double* grx; const double* gry;   // x / y columns of glob_rl as contiguous arrays (coalesced scans)
    // derived at ltpl_create
    const int* rng_end;               // [L]     end layer of the planning range that starts in layer l
    const int* layer_ebase;           // [L + 1] first edge INTO layer l (= in_ptr[layer_off[l]]); [L] = E
    const unsigned char* edge_src8;   // [E]     edge_src as bytes (<= 255 nodes per layer)
    const unsigned char* edge_dst8;   // [E]     destination node index inside its layer
    const unsigned char* edge_rank8;  // [E]     rank of the edge among the in-edges of its destination
    const int* layer_degmax;          // [L]     largest in-degree of a node of layer l
    // SWEEP ORDER. Inside every layer transition the sweep, the obstacle mask and the LDS edge bitmap address the edges in a second order:
    // sorted by (in-edge rank, destination node) instead of CSC (destination, source). The lanes of a wave then hold edges into DIFFERENT
    // nodes, so the LDS atomics of the sweep (ds_min_u64 on the destination's frontier slot) meet at most two lanes per address; in CSC
    // order the ~5 (up to 21) in-edges of a node sit in consecutive lanes and every atomic serialises that many times. A transition's
    // edges occupy the same index range [layer_ebase[l], layer_ebase[l + 1]) in both orders.
    const double* sw_cost;            // [E + 1 + LTPL_SW_PAD] edge cost in sweep order; [E] = +inf (sentinel for the lanes beyond a transition)
    const unsigned* sw_meta;          // [same] in-edge rank | source node << 8 | destination node << 16, sweep order; [E] = 0 (the low half
                                      //         is the election key among equal candidates: the reference settles them by source node)
    const int* sw2csc;                // [E]     CSC edge id of sweep position p
    const int* csc2sw;                // [E]     sweep position of CSC edge e
    // track bounds per layer: bound1 = refline + normvec w_right, bound2 = refline - normvec w_left, centre = (b1 + b2) / 2
    const double* b1x; const double* b1y; const double* b2x; const double* b2y; const double* ctx; const double* cty;
    const float4* edge_cap;           // [2 E] IN SWEEP ORDER: capsule of the edge's samples in fp32: (Ax, Ay, ABx, ABy), (1 / |AB|^2, dev, hg2, first sample |
                                      //     #samples << 24 as bit pattern; #samples = 0: look samp_ptr up): chord between the first and the last
                                      //     sample, largest sample distance from it, squared half of the largest gap between consecutive sample
                                      //     projections -- two-sided conservative cull of the obstacle mask, the exact test is fp64
    float cull_slack;                 // bound on the fp32 rounding of the cull's distance (positions, chord, arithmetic)
    // closest-layer grid (layer_grid.hpp): per cell the <= 2 intervals of reference-line layers that can be closest to a point of the cell
    // (first layer, length, first layer, length; length -1 = scan all layers); null: phase 1 scans all layers (LTPL_NO_LAYER_GRID=1)
    const int4* lgrid; double lg_x0, lg_y0, lg_inv; int lg_nx, lg_ny;
    // PATH ASSEMBLY RECORDS (round 5): what the assembly of a path gathers per node / per edge, as ONE record each, so that the chain of
    // dependent global round trips behind the backtrack is node record -> edge record (it was layer_off -> in_ptr -> edge_src8 ->
    // samp_ptr -> sx / sy / ssc: five round trips of ~600 cycles per path on a wave that has nothing else to do meanwhile)
    const int4* node_rec;             // [V] first in-edge (CSC id), then the source nodes of the node's first 12 in-edges as bytes (0xff = none)
    const double* edge_rec;           // [E][LTPL_EDGE_REC] (first sample | #samples << 32 as bit pattern, edge length, x, y of the first sample,
                                      //     x, y of the last sample, sin, cos of the first sample's heading, sin, cos of the last sample's)
};

struct DevPathsIn {
    int n_scen, n_w_last;
    const double* w_last;
    const int* start_layer; const int* start_node; const int* flags; const int* last_action; const int* const_closest;
    const double* psi_s;
    const int* veh_off; const int* pos_off; const double* veh_radius; const double* pos_x; const double* pos_y;
    const int* zone_off; const int* zone_gid;
    const int* n_last; const int* last_layer; const int* last_node;
    // BLOCK -> SCENARIO ORDER (round 6; one-wave batches, null otherwise: block b plans scenario b): order[b] = the scenario of block b, the
    // scenarios sorted by start layer. Blocks are dispatched in index order, so at any time the whole chip works on one region of the track:
    // the waves of a moment share their lattice lines, and the velocity jobs -- numbered in the order their paths complete -- come in runs of
    // similar length, so that the 64 profiles of a lane-kernel wave end together (lane kernel alone 0.265 against 0.282 ms; +2 % ticks/s,
    // profiles/r06r_ab_order.txt). Tried first and NOT kept: the sorted sequence dealt out in eighths, one per XCD (block b runs on XCD b % 8,
    // each XCD with its own 4 MiB L2 and an eighth of the 6 MB lattice to itself) -- 37.8 against 40.1 M ticks/s: the eighths of a track are
    // not equal work (planning ranges of 11 to 29 layers), and the lattice was not missing in L2 to begin with (path kernel alone: unchanged by
    // the order that won). Outputs are indexed by scenario: results do not depend on the order.
    const int* order;
};

// completion signal of the latency path: the LAST block of a launch writes a sequence number into page-locked host memory after
// every block has pushed its (zero-copy) outputs out with a system-scope fence; the host polls that word instead of synchronising
// the stream (launch + poll: 11 us, launch + hipStreamSynchronize: 15 us on the round-2 box, tools/ubench/launch). All null: no signal.
struct DoneSignal { unsigned* host_flag; unsigned* dev_count; unsigned seq; };

// called by ALL threads of every block as the last thing the kernel does
__device__ __forceinline__ void signal_done(const DoneSignal& d)
{
    if (!d.host_flag) return;
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned prev = atomicAdd(d.dev_count, 1u);
        if (prev == gridDim.x - 1) {
            *d.dev_count = 0u;                                   // the next launch on the stream starts from zero
            __hip_atomic_store(d.host_flag, d.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// Operand records of the batch velocity stage (|kappa|, element length per path row): an fp64 PAIR, one 16-byte load per row and lane,
// 1 / |kappa| in fp64 -- the reference is IEEE fp64 throughout (VpForwardBackward.py:194-227) and so is every operand, state and output
// of this stage (element-wise vx error against the oracle ~1e-13). -DLTPL_VEL_F32_OPERANDS builds the rounds-3..5 form (fp32 pair,
// v_rcp_f32: +6.5 % ticks/s, element-wise vx error up to 1e-5 -- profiles/r04f_vel_precision.txt); not shipped, not tested.
#ifndef LTPL_VEL_F32_OPERANDS
typedef double ke_scalar;
typedef double ke_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ ke_t make_ke(double k, double e) { ke_t v; v.x = k; v.y = e; return v; }
// 1 / |kappa|: hardware reciprocal + ONE Newton step. Measured on gfx950 over 4 M values of |kappa| between 1e-12 and 4e3 1/m
// (tools/ubench/rcp/rcp_f64.hip, profiles/r06c_rcp_f64.txt): v_rcp_f64 alone 4.6e-8 relative, one step 2.2e-15 (20 ulp), two steps correctly
// rounded. The limit speed ay / |kappa| is a row of the result wherever no sweep lowers it: tests/test_gpu_vel_ref.py holds those rows to the
// long-double reference at 5e-10 (exponent 1; vel_cases.BOUNDS, class "regular"), which one step meets (20 ulp = 2e-15 in v^2) and the bare
// v_rcp_f64 does not (4.6e-8 in v^2 = 2.3e-8 in v: passes the oracle comparisons at 1e-5, fails there);
// the second step was two dependent fma on the lane kernels' serial chain: +1.7 % ticks/s without it (same-box A/B, profiles/r06b_ab_bench.txt).
__device__ __forceinline__ double ke_rcp(const ke_t& r)        // (0 -> NaN: treated as +inf by the callers' fmin)
{
    double q = __builtin_amdgcn_rcp(r.x);
    q = fma(fma(-r.x, q, 1.0), q, q);
    return r.x == 0.0 ? (double)INFINITY : q;
}
#else
typedef float ke_scalar;
typedef float2 ke_t;
__device__ __forceinline__ ke_t make_ke(double k, double e) { return make_float2((float)k, (float)e); }
__device__ __forceinline__ double ke_rcp(const ke_t& r) { return (double)__builtin_amdgcn_rcpf(r.x); }     // 1 ulp in fp32, inf on straights
#endif

struct DevPathsOut {
    int cap_nodes, cap_pts;
    int* end_layer; int* closest_obj_index; int* closest_obj_node; int* n_actions;
    int* action_id; int* valid; int* reduced; int* goal_layer; int* n_nodes; int* n_pts; int* n_ties;
    int* nodes; int* node_idx; double* coeff; double* path_param;
    ke_t* vke;                       // optional tiled plane (|kappa|, element length) as fp64 pairs for the batch velocity stage
    double* vxy;                     // optional tiled plane (x, y) of the FOLLOW jobs' path points (tile = follow job index): k_follow_prep
    // job compaction of the batch velocity stage (all nullptr outside the pipeline): every valid path takes a job index
    // from a counter of its class (0 = generic forward-backward profile, 1 = follow); its planes are tiled by JOB, so
    // the lanes of a velocity wave (64 consecutive jobs of one class) are all busy and equally long
    int* job_cnt;                    // [0] generic jobs, [1] follow jobs, [2] largest n_pts of the launch (row chunks beyond it exit at once)
    int2* job_slot;                  // [n_slots_pad] generic jobs -> (slot, n_pts), then [n_scen_pad] follow jobs: one load gives a velocity
                                     // wave slot AND length of its job (two dependent round trips less per block)
    int n_slots_pad;                 // tile index of follow job j = n_slots_pad + j (rows of the blocked planes: cap_pts rounded up to 8)
    DoneSignal done;                 // latency path only (k_paths / k_tick launched for a few scenarios)
};


// Timing / fault-injection switches (LTPL_ABLATE, LTPL_EXP_SKIP, LTPL_LDS_POISON, LTPL_SCRATCH_POISON, LTPL_DEBUG_TIMING, LTPL_DEBUG_OCC)
// only exist in the EXPERIMENT build (-DLTPL_EXPERIMENT -> libltpl_hip_exp.so, tools/ and the stale-LDS test): the release library has
// no code path that skips work, alters memory or instruments kernels on an environment variable's say-so.
#define DBG_SLOTS 64
#ifdef LTPL_EXPERIMENT
__device__ __forceinline__ void dbg_stamp(long long* dbg, int k)
{
    if (dbg && (threadIdx.x & 63) == 0 && blockIdx.x < 256) dbg[(size_t)blockIdx.x * DBG_SLOTS + (threadIdx.x >> 6) * 16 + k] = clock64();
}
#else
__device__ __forceinline__ void dbg_stamp(long long*, int) {}
#endif

// LTPL_DEBUG_TIMING for the lane kernel: `row` selects one of 256 sample rows (generic / follow / unconstrained blocks)
#ifdef LTPL_EXPERIMENT
__device__ __forceinline__ void vl_stamp(long long* dbg, int row, int k)
{
    if (dbg && (threadIdx.x & 63) == 0 && row >= 0 && row < 256) dbg[(size_t)row * DBG_SLOTS + k] = clock64();
}
#else
__device__ __forceinline__ void vl_stamp(long long*, int, int) {}
#endif

#include "wave_ops.hpp"

// ---------------------------------------------------------------------------------------------------------------------
// the path kernel (seam 1)
// ---------------------------------------------------------------------------------------------------------------------
// Result of the path stage for the calling wave (waves 0..2 own one action slot each).
struct WavePath { int valid; int n_pts; int n_nodes; int name; int reduced; int goal_layer; int end_node; };

#include "paths_team.hpp"

// Waves per SIMD of the one-wave batch kernel: the register budget must hold the kernel WITHOUT register spills (builds of
// this kernel that spilled VGPRs to scratch produced wrong parents on gfx950; __graft_entry__.build() rejects such builds).
// Runtime plan (any lattice): 2 waves per SIMD = 256 VGPRs. Compile-time plan (three register chunks of edges): 4 waves per
// SIMD = 128 VGPRs.
#ifndef LTPL_RT_WAVES
#define LTPL_RT_WAVES 2              // -DLTPL_RT_WAVES=4 builds the spilling variant studied in tools/ubench/spill_study
#endif
template <int NW, class P>
__global__ __launch_bounds__(64 * NW, (NW == 1 ? (P::fixed ? 4 : LTPL_RT_WAVES) : 1)) void k_paths(DevLat lat, DevPathsIn in, DevPathsOut out, TeamLds lp)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ TeamShared ts;
    if constexpr (P::fixed) {
        // compile-time plan classes: the argument structs are read from the kernarg segment phase by phase (karg_reload, paths_team.hpp)
        // instead of being held in scalar registers -- and spilled into vector-register lanes -- from entry to last use; the by-value
        // parameters only define the kernarg layout
        const PathsKArgs* ka = paths_kargs();
        (void)team_paths_body<NW, P, 1>(ka->lat, ka->in, ka->out, ka->lp, smem, ts, nullptr, nullptr, nullptr, nullptr);
        if constexpr (NW != 1) signal_done(ka->out.done);
        return;
    }
    (void)team_paths_body<NW, P>(lat, in, out, lp, smem, ts, nullptr, nullptr, nullptr, nullptr);
    if constexpr (NW != 1) signal_done(out.done);          // (only the four-wave latency form is launched with a completion word)
}
typedef PlanFx<32, 32, 1> PlanA;      // <= 32 nodes per layer, <= 31 layers of planning range (Monteblanco, stock parameters)
typedef PlanFx<32, 40, 1> PlanB;      // <= 32 nodes per layer, <= 39 layers (synthetic C3 oval; zalazone, lvms, modena of the reference's tracks)
typedef PlanFx<48, 32, 1> PlanC;      // <= 48 nodes per layer, <= 31 layers (berlin: 40 nodes per layer -- round 3 ran it on the 204-register PlanRt kernel)
typedef PlanFx<32, 32, NUM_WAVES> PlanA4;   // class A for the four-wave latency kernels (k_paths<4>, k_tick)


#include "vel_wave.hpp"

// the arguments of k_tick as they lie in the kernarg segment
struct TickKArgs { PathsKArgs pk; DevVelParams p; DevTickVelIn vin; DevTickVelOut vout; int vel_off, vel_stride, vel_cap; };
static_assert(sizeof(DevVelParams) % 8 == 0 && sizeof(DevTickVelIn) % 8 == 0 && sizeof(DevTickVelOut) % 8 == 0 && alignof(DevVelParams) == 8 &&
              alignof(DevTickVelIn) == 8 && alignof(DevTickVelOut) == 8, "TickKArgs must mirror the kernarg layout of k_tick");
static constexpr size_t KOFF_TP = offsetof(TickKArgs, p), KOFF_TVIN = offsetof(TickKArgs, vin), KOFF_TVOUT = offsetof(TickKArgs, vout);

// body of k_tick. RL = true: every argument struct is a reference INTO THE KERNARG SEGMENT, re-read per stage (karg_reload, paths_team.hpp)
template <int EM, bool AXM1, class P, int RL>
__device__ __forceinline__ void tick_body(const DevLat& lat_, const DevPathsIn& in_, const DevPathsOut& out_, const TeamLds& lp_,
                                          const DevVelParams& p_, const DevTickVelIn& vin_, const DevTickVelOut& vout_,
                                          int vel_off, int vel_stride, int vel_cap, unsigned char* smem, TeamShared& ts, int& sh_follow_n)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    VelScratch vs; double* px = nullptr; double* py = nullptr;
    if (wave < LTPL_MAX_ACTIONS) vs = carve_vel_scratch(smem + vel_off + (size_t)wave * vel_stride, vel_cap, false, true, &px, &py);
    WavePath wp = team_paths_body<NUM_WAVES, P, RL>(lat_, in_, out_, lp_, smem, ts, wave < LTPL_MAX_ACTIONS ? vs.kabs : nullptr,
                                                 wave < LTPL_MAX_ACTIONS ? vs.el : nullptr, px, py);
    // (re-derived from the kernarg segment pointer, not carried across the path search: karg_at, paths_team.hpp)
    const DevLat& lat = *LTPL_KARG_LAT(&lat_); const DevPathsIn& in = *LTPL_KARG_IN(&in_); const DevPathsOut& out = *LTPL_KARG_OUT(&out_);
    const TeamLds& lp = *LTPL_KARG_LP(&lp_);
    // (the small parameter structs of the velocity stage by value: its recurrences must not depend on argument loads)
    const DevVelParams p = *karg_at<RL, DevVelParams, KOFF_TP>(&p_);
    const DevTickVelIn vin = *karg_at<RL, DevTickVelIn, KOFF_TVIN>(&vin_); const DevTickVelOut vout = *karg_at<RL, DevTickVelOut, KOFF_TVOUT>(&vout_);
    const int s = blockIdx.x;
    // The fourth wave has no primitive of its own: it computes the unconstrained profile of the 'follow' slot
    // (calc_vel_profile_follow.py:297-307, independent of the controlled part) while wave 0 runs the brake / segment part.
    if (wave < LTPL_MAX_ACTIONS) {
        for (int i = lane; i < 2 * p.n_axm; i += 64) vs.axm[i] = p.axm[i];
        if (wp.valid) for (int i = lane; i < wp.n_pts; i += 64) vs.kabs[i] = fabs(vs.kabs[i]);
        if (wave == 0 && lane == 0) sh_follow_n = (wp.valid && wp.name == LTPL_ACT_FOLLOW) ? wp.n_pts : 0;
    }
    __syncthreads();
    const int follow_n = sh_follow_n;
    if (wave < LTPL_MAX_ACTIONS) {
        const int slot = s * LTPL_MAX_ACTIONS + wave;
        vs.dbg = lp.dbg;
        if (wp.valid) tick_vel_stage<EM, AXM1>(lat, in, out, wp, vs, px, py, p, vin, vout, s, slot, lane, wave == 0 && follow_n > 0);
        else if (lane == 0) { vout.vel_bound[slot] = 0; vout.too_close[slot] = 0; }
        dbg_stamp(lp.dbg, 11);
        if (!(wave == 0 && follow_n > 0)) __syncthreads();     // wave 0 with a follow slot joins inside follow_profile
    } else {
        if (follow_n > 0) {
            double* dpx; double* dpy;
            VelScratch v0 = carve_vel_scratch(smem + vel_off, vel_cap, false, true, &dpx, &dpy);   // wave 0's arrays
            v0.start = smem + fused_tick_flags_off(vel_off, vel_stride);                           // own run-start flags
            v0.dbg = nullptr;
            fb_profile<EM, AXM1, false>(follow_n, v0, vin.gg_ax, vin.gg_ay, p, p.v_max, vin.vel_plan[s], false, 0.0, lane);
        }
        __syncthreads();
    }
    signal_done(LTPL_KARG_OUT(&out)->done);
}


template <int EM, bool AXM1, class P>
__global__ __launch_bounds__(WG_THREADS) void k_tick(DevLat lat, DevPathsIn in, DevPathsOut out, TeamLds lp,
                                                     DevVelParams p, DevTickVelIn vin, DevTickVelOut vout,
                                                     int vel_off, int vel_stride, int vel_cap)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ TeamShared ts;
    __shared__ int sh_follow_n;
    if constexpr (P::fixed) {
        // (the by-value parameters only define the kernarg layout: see k_paths)
        const TickKArgs* tk = (const TickKArgs*)(const TickKArgs LTPL_AS4*)__builtin_amdgcn_kernarg_segment_ptr();
        tick_body<EM, AXM1, P, 1>(tk->pk.lat, tk->pk.in, tk->pk.out, tk->pk.lp, tk->p, tk->vin, tk->vout, tk->vel_off, tk->vel_stride, tk->vel_cap,
                                     smem, ts, sh_follow_n);
        return;
    }
    tick_body<EM, AXM1, P, 0>(lat, in, out, lp, p, vin, vout, vel_off, vel_stride, vel_cap, smem, ts, sh_follow_n);
}

// ---------------------------------------------------------------------------------------------------------------------
// PERSISTENT SINGLE TICK (round 6): k_tick as a RESIDENT kernel behind a mailbox in page-locked memory
// ---------------------------------------------------------------------------------------------------------------------
// One car, one tick at a time (the only use the reference has: OnlineTrajectoryHandler.py:353-366 spends a 0.1 s budget per tick) is a
// LATENCY problem, and the round-5 counters say where a launched tick loses it (profiles/r05D_icache_tick.txt): every launch starts with
// a cold instruction cache (the kernel's ~70 KB come back through L2: 1.1 k line fetches per tick), pays the dispatch of a grid on an
// idle chip and two runtime calls (H2D copy + launch) on the host. This kernel is launched ONCE per handle -- one workgroup of four waves,
// the team of k_tick -- and then serves ticks until it is told to leave or has idled for `idle_limit`:
//   host:   pack the inputs into the page-locked staging buffer (as for k_tick), write the tick's argument block into the mailbox,
//           store-release the next sequence number, spin on the completion word (the DoneSignal the fused tick already carries);
//   kernel: thread 0 polls the sequence word (system-scope acquire loads: they bypass the caches), the others sleep at the barrier;
//           all threads copy the argument block and the packed inputs into device memory (two coalesced passes over PCIe instead of
//           dependent zero-copy reads inside the phases), fence, invalidate the scalar cache (the arguments are read with scalar loads)
//           and run tick_body<.., RL = 2> -- the SAME body as k_tick, its argument block addressed through the kernel's first argument.
// Outputs go straight into page-locked memory as for every call with <= 8 scenarios (LTPL_ZC_OUT). No hipMemcpyAsync, no launch, no
// stream synchronisation on the tick's path. Results are bit-identical to k_tick's (same code, same order of operations).
// A RESIDENT kernel never completes: device-wide synchronisations of the process (hipDeviceSynchronize, hipFree) would wait for it. That
// is why the mode is opt-in (ltpl_create_ex / LTPL_PERSISTENT_TICK), why every other entry point of the handle stops the kernel first
// (persist_stop) and why the kernel leaves BY ITSELF after `idle_limit` (default 250 ms) without a tick; the host notices (`exited`)
// and starts it again with the next tick. Only for lattices whose four-wave kernel has a compile-time LDS plan (PlanA4).
#define PT_CMD_TICK 0u
#define PT_CMD_EXIT 1u
struct TickMailbox {
    // host -> kernel
    unsigned seq;                  // number of the posted tick; written LAST, with release semantics
    unsigned cmd;                  // PT_CMD_*
    unsigned in_bytes;             // packed inputs of the tick: bytes to copy from the staging buffer to its device twin (multiple of 16)
    unsigned pad0;
    // kernel -> host
    unsigned exited;               // 0 while the kernel is resident; its last store: 1
    unsigned n_done;               // ticks served by this residency
    unsigned long long busy_clk;   // wall_clock64 ticks (100 MHz) between "sequence number seen" and "tick done", summed over n_done ticks
    unsigned long long last_clk;   // ... of the last tick
    unsigned long long pad1;
    alignas(16) unsigned char args[2048];      // TickKArgs of the posted tick
};
static_assert(sizeof(TickKArgs) <= 2048 && sizeof(TickKArgs) % 8 == 0, "mailbox argument block");

template <int EM, bool AXM1, class P>
__global__ __launch_bounds__(WG_THREADS) void k_tick_persistent(const TickKArgs* d_args, TickMailbox* mb, const unsigned char* h_in, unsigned char* d_in,
                                                                unsigned start_seq, unsigned long long idle_limit)
{
    static_assert(P::fixed, "the persistent tick reads its arguments like the compile-time plan classes do");
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ TeamShared ts;
    __shared__ int sh_follow_n;
    __shared__ unsigned sh_seq, sh_cmd, sh_in_bytes;
    unsigned last = start_seq, n_done = 0;
    unsigned long long busy = 0;
    for (;;) {
        unsigned long long t_seen = 0;
        if (threadIdx.x == 0) {
            const unsigned long long t0 = wall_clock64();
            unsigned sq, cmd = PT_CMD_TICK;
            for (;;) {
                sq = __hip_atomic_load(&mb->seq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
                if (sq != last) { cmd = __hip_atomic_load(&mb->cmd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
                if (wall_clock64() - t0 > idle_limit) { cmd = PT_CMD_EXIT; break; }
                __builtin_amdgcn_s_sleep(4);
            }
            t_seen = wall_clock64();
            sh_seq = sq; sh_cmd = cmd;
            sh_in_bytes = __hip_atomic_load(&mb->in_bytes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __syncthreads();
        if (sh_cmd != PT_CMD_TICK) break;
        last = sh_seq;
        // argument block and packed inputs: page-locked memory -> device memory, 16 bytes per thread and pass. Page-locked memory is not
        // cached on the device (fine-grained: every read crosses PCIe), so ALL loads are issued before the first store -- one PCIe round
        // trip for the block and the first 8 KB of inputs (a C2 tick packs ~2 KB) -- and nothing has to be invalidated for them.
        {
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            constexpr unsigned NA = (unsigned)(sizeof(TickKArgs) + 15) / 16;
            static_assert(NA <= WG_THREADS, "one pass over the argument block");
            const u32x4* sa = reinterpret_cast<const u32x4*>(mb->args);
            u32x4* da = reinterpret_cast<u32x4*>(const_cast<TickKArgs*>(d_args));
            const u32x4* si = reinterpret_cast<const u32x4*>(h_in);
            u32x4* di = reinterpret_cast<u32x4*>(d_in);
            const unsigned nq = sh_in_bytes >> 4, t = threadIdx.x;
            const u32x4 zero = {0u, 0u, 0u, 0u};
            const u32x4 a = t < NA ? sa[t] : zero;
            const u32x4 b0 = t < nq ? si[t] : zero, b1 = t + WG_THREADS < nq ? si[t + WG_THREADS] : zero;
            if (t < NA) da[t] = a;
            if (t < nq) di[t] = b0;
            if (t + WG_THREADS < nq) di[t + WG_THREADS] = b1;
            for (unsigned i = t + 2 * WG_THREADS; i < nq; i += WG_THREADS) di[i] = si[i];
            // the copies are consumed by THIS workgroup: stores retired (they write through to L2), then no stale line of the two buffers in
            // the CU's vector cache and no argument of the previous tick in the scalar cache -- no system-scope fence, no L2 write-back
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_s_waitcnt(0);
            __syncthreads();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __builtin_amdgcn_s_dcache_inv();
        }
        tick_body<EM, AXM1, P, 2>(d_args->pk.lat, d_args->pk.in, d_args->pk.out, d_args->pk.lp, d_args->p, d_args->vin, d_args->vout,
                                  *karg_at<2, int, offsetof(TickKArgs, vel_off)>((const int*)nullptr), *karg_at<2, int, offsetof(TickKArgs, vel_stride)>((const int*)nullptr),
                                  *karg_at<2, int, offsetof(TickKArgs, vel_cap)>((const int*)nullptr), smem, ts, sh_follow_n);
        // (tick_body ends with signal_done: outputs fenced out, completion word stored -- the host may already be packing the next tick)
        if (threadIdx.x == 0) {
            const unsigned long long dt = wall_clock64() - t_seen;
            busy += dt; ++n_done;
            __hip_atomic_store(&mb->last_clk, dt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&mb->busy_clk, busy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&mb->n_done, n_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __syncthreads();                                             // (sh_seq / sh_cmd are rewritten by thread 0 in the next round)
    }
    if (threadIdx.x == 0) __hip_atomic_store(&mb->exited, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

#include "vel_lanes.hpp"

// ---------------------------------------------------------------------------------------------------------------------
// object ingestion: ObjectListInterface.process_object_list (ObjectListInterface.py:75-153)
// ---------------------------------------------------------------------------------------------------------------------
// One lane per object: closest centre-line point (first minimum), the neighbour with the larger opening angle
// (get_s_coord.py:34-47,93-96 with closed = True), closest of the 50 np.linspace points between the two bracketing
// points, comparison of the squared distances to the interpolated bounds with the squared track width
// (check_inside_bounds.py:26-56); constant-velocity prediction and radius (ObjectListInterface.py:117-133).
// The per-object body is shared with the fleet's closed-loop simulation (fleet_sim.hpp, k_fleet_sim_step).
struct ObjIngest { int on_track; double pred_x, pred_y, radius; };
__device__ __forceinline__ ObjIngest process_object_dev(const DevLat& lat, double dt, double px, double py, double th, double v, double len)
{
    const int L = lat.L;
    int nb = 0; double best = INFINITY;
    for (int l = 0; l < L; ++l) {
        const double dx = lat.ctx[l] - px, dy = lat.cty[l] - py;
        const double d2 = dx * dx + dy * dy;
        if (d2 < best) { best = d2; nb = l; }
    }
    int i1 = nb - 1; if (i1 < 0) i1 += L;
    int i2 = nb + 1; if (i2 > L - 1) i2 = 0;
    const double ang1 = fabs(angle3pt_dev(lat.ctx[nb], lat.cty[nb], px, py, lat.ctx[i1], lat.cty[i1]));
    const double ang2 = fabs(angle3pt_dev(lat.ctx[nb], lat.cty[nb], px, py, lat.ctx[i2], lat.cty[i2]));
    const int a = ang1 >= ang2 ? i1 : nb, b = ang1 >= ang2 ? nb : i2;
    const double cax = lat.ctx[a], cay = lat.cty[a], cbx = lat.ctx[b], cby = lat.cty[b];
    // np.linspace(start, stop, 50): y_i = i * ((stop - start) / 49) + start, y_49 = stop
    const double sx = (cbx - cax) / 49.0, sy = (cby - cay) / 49.0;
    int bi = 0; double bd = INFINITY;
    for (int i = 0; i < 50; ++i) {
        const double qx = i == 49 ? cbx : (double)i * sx + cax, qy = i == 49 ? cby : (double)i * sy + cay;
        const double dx = qx - px, dy = qy - py;
        const double d2 = dx * dx + dy * dy;
        if (d2 < bd) { bd = d2; bi = i; }
    }
    auto lin = [&](double A, double B) { return bi == 49 ? B : (double)bi * ((B - A) / 49.0) + A; };
    const double l1x = lin(lat.b1x[a], lat.b1x[b]), l1y = lin(lat.b1y[a], lat.b1y[b]);
    const double l2x = lin(lat.b2x[a], lat.b2x[b]), l2y = lin(lat.b2y[a], lat.b2y[b]);
    const double d_track_2 = (l1x - l2x) * (l1x - l2x) + (l1y - l2y) * (l1y - l2y);
    const double d_b1_2 = (l1x - px) * (l1x - px) + (l1y - py) * (l1y - py);
    const double d_b2_2 = (l2x - px) * (l2x - px) + (l2y - py) * (l2y - py);
    ObjIngest r;
    r.on_track = !(d_b1_2 > d_track_2 || d_b2_2 > d_track_2) ? 1 : 0;
    r.pred_x = px - sin(th) * v * dt;
    r.pred_y = py + cos(th) * v * dt;
    r.radius = len / 2.0;
    return r;
}

__global__ __launch_bounds__(64) void k_process_objects(DevLat lat, int n_obj, double dt, const double* ox, const double* oy,
                                                        const double* oth, const double* ov, const double* olen,
                                                        int* on_track, double* pred_x, double* pred_y, double* radius)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n_obj) return;
    const ObjIngest r = process_object_dev(lat, dt, ox[k], oy[k], oth[k], ov[k], olen[k]);
    on_track[k] = r.on_track; pred_x[k] = r.pred_x; pred_y[k] = r.pred_y; radius[k] = r.radius;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
static thread_local std::string g_create_error;
struct TickLayout;
static void free_resident(TickLayout* t);
static int self_test(struct ltpl_handle* h, const ltpl_lattice_desc* d);

struct ltpl_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    DevLat lat{};
    TeamLds lp1{}, lp4{};            // LDS plans of the path kernel: one wave / four waves per scenario
    int batch_nw = 1;                // waves per scenario used for batches (LTPL_BATCH_NW)
    int plan_class = 0;              // LDS plan of the one-wave batch kernel: 0 = runtime (PlanRt), 1 = PlanA, 2 = PlanB, 3 = PlanC
    int plan_class4 = 0;             // LDS plan of the four-wave kernels: 0 = runtime, 1 = PlanA4
    int long_horizon = 0;            // 1: parent tables in global memory (PlanRtG), velocity stage always through the lane kernels
    int fused_fits = 1;              // 0: the fused tick's LDS footprint (fused_tick_lds) is above the budget, or long_horizon: every tick runs the
                                     // pipeline (single ticks included: its path kernel then takes the four-wave team)
    int nw1_min_scen = PIPELINE_MIN_SCEN;   // calls with at least this many scenarios use one-wave teams
    // ltpl_tick_batch & co: calls with at least this many scenarios run the batch PIPELINE (one wave per scenario + the three velocity kernels),
    // smaller ones the FUSED tick kernel (one four-wave workgroup per scenario, one launch). Rounds 1-5: 64. Round 6, measured on the MI355X
    // with resident inputs (tools/c4_fused_ab.py, profiles/r06h_c4_fused_ab.txt; us per step, fused / pipeline): 128 scenarios 81 / 110,
    // 256: 81 / 109, 512: 92 / 111, 1024: 152 / 117 -- while every workgroup of the fused kernel finds a compute unit of its own (or shares
    // one with a single neighbour) a step costs ONE tick's latency, the pipeline pays four dependent launches. BASELINE config C4 shards
    // 1024 scenarios over 8 GPUs: 128 per GPU. Default: more than 2 workgroups per compute unit (fewer where the fused kernel's LDS
    // footprint lets fewer be resident) -> pipeline; LTPL_PIPELINE_MIN_SCEN=<n> overrides (the GPU test-suite pins 64: its batches of
    // 64 .. 256 scenarios are there to exercise the pipeline).
    int pipeline_min_scen = PIPELINE_MIN_SCEN;
    // pipeline launches with at least this many scenarios finish their follow jobs inside the lane kernel (k_vel_lanes, emit bit 1); smaller ones
    // keep the two halves of a follow job on two waves + k_vel_final: a shorter chain, which is what a small batch's step is made of.
    // LTPL_FOLLOW_EMIT_MIN_SCEN overrides (the GPU test-suite sets 256 so that its batches exercise the form the headline runs on).
    int follow_emit_min_scen = 8192;
    int scen_order = 1;              // batches of >= LTPL_SCEN_ORDER_MIN_SCEN scenarios are planned in the order of their start layers (DevPathsIn::order);
                                     // LTPL_NO_SCEN_ORDER=1: in the caller's order (identical results: tests, same-box A/B)
    void* d_par = nullptr; size_t d_par_cap = 0;         // parent-table slabs of the long-horizon mode
    ltpl_caps caps{};
    std::vector<void*> dev_allocs;
    // staging
    void* h_in = nullptr; size_t h_in_cap = 0;
    void* d_in = nullptr; size_t d_in_cap = 0;
    void* h_out = nullptr; size_t h_out_cap = 0;
    void* d_out = nullptr; size_t d_out_cap = 0;
    struct TickLayout* resident = nullptr;   // device-resident batch of ltpl_batch_upload
    long long* d_dbg = nullptr;              // LTPL_DEBUG_TIMING=1: cycle stamps
    void* d_planes = nullptr; size_t d_planes_cap = 0;   // tiled profile planes of the lane kernel
    // second buffer set + stream of the device-resident batch: the velocity kernels of step k overlap the path kernel of
    // step k + 1 (ltpl_batch_run)
    // Round 3: THREE buffer sets and TWO velocity streams. With two sets the path kernel of step r + 2 waited for the velocity kernels of
    // step r, and those take a whole step when they share the chip with a path kernel (its four waves per SIMD hold the register file: a
    // velocity wave only gets on a SIMD when a path wave retires) -- the velocity chain was the critical path (0.99 ms per step against
    // 0.89 ms of path kernel). Chains of consecutive steps now run next to each other on alternating streams and the path kernel only
    // waits for the chain three steps back: 0.947 ms per step (33.4 -> 34.4 M ticks/s).
#ifndef LTPL_PIPE_SETS
#define LTPL_PIPE_SETS 3               // (A/B on one box: 3, 4, 6 sets with two velocity streams all 34.3-34.4 M ticks/s; three or four streams: 33.4 M)
#endif
#ifndef LTPL_VEL_STREAMS
#define LTPL_VEL_STREAMS 2
#endif
    static constexpr int PIPE_SETS = LTPL_PIPE_SETS, VEL_STREAMS = LTPL_VEL_STREAMS;
    struct TickLayout* resident_x[PIPE_SETS - 1] = {};    // sets 1 .. (set 0 = `resident` on d_out / d_planes)
    void* d_out_x[PIPE_SETS - 1] = {}; size_t d_out_x_cap[PIPE_SETS - 1] = {};
    void* d_planes_x[PIPE_SETS - 1] = {}; size_t d_planes_x_cap[PIPE_SETS - 1] = {};
    hipStream_t vel_stream[VEL_STREAMS] = {};
    hipEvent_t ev_paths[PIPE_SETS] = {}, ev_vel[PIPE_SETS] = {};
    // second stream for the path kernels of odd steps (LTPL_PATH_STREAMS=2): the drain of one path kernel -- its longest scenarios on a
    // mostly idle chip -- overlaps the ramp of the next one
    hipStream_t path_stream2 = nullptr; hipEvent_t ev_begin = nullptr; int path_streams = 1;
    int last_set = 0;
    std::vector<hipEvent_t> ev_step;          // timing events around the path kernel of every step of the last timed run
    float last_paths_ms = 0.0f; int last_paths_n = 0;
    // host copy of the per-layer / per-node tables for the planner state machine (planner_core.hpp); empty when the
    // descriptor came without raceline / node_psi columns
    ltplp::HostLat hostlat; bool has_hostlat = false;
    int scratch_poison_on = 0; unsigned scratch_poison_word = 0;   // LTPL_SCRATCH_POISON (testing)
    int final_y = 8;                                                // row-chunk blocks per tile of k_vel_final (LTPL_FINAL_Y; A/B on one box: 2: 1.09, 4: 1.07, 8 / 22: 1.06 ms per step)
    int exp_skip = 0;                                               // LTPL_EXP_SKIP (timing experiments only): 1 prep, 2 lanes, 4 final kernel not launched
    int force_fused = 0, no_overlap = 0;                            // LTPL_FORCE_FUSED, LTPL_NO_OVERLAP (measurement switches)
    int poll_sync_every = 4096, poll_query = 0;
    int poll = 0;                    // LTPL_POLL=1: small zero-copy calls complete through a polled word in page-locked memory instead of a stream
                                     // synchronisation. Measured on the drop-in tick: p50 -4 us, but p99 +8 us with occasional 250 us outliers
                                     // (the runtime retires the launch concurrently with the next call) -- off by default, p99 is the metric
    unsigned* h_flag = nullptr; unsigned* d_done_cnt = nullptr; unsigned done_seq = 0; unsigned polled_calls = 0;
    int zc_in = 0;                   // small calls: kernels read their inputs straight from the page-locked staging buffer (no H2D copy)
    int zc_out = 0;                  // small calls: kernels write their outputs straight into the page-locked host buffer (no D2H copy)
    std::vector<int> rng_end_host;   // planning range end per start layer, -1 = no planning range (end of an open track)
    std::vector<int> sw2csc_host;    // CSC edge id of every sweep position (DevLat::sw2csc)
    int n_planners = 0;              // live ltpl_planner objects that compute through this handle (ltpl_destroy refuses while > 0)
    // LTPL_TICK_GRAPH=1 (round 5, measurement switch, off by default): the single fused tick -- H2D copy of the packed inputs -> k_tick
    // [-> D2H copy of the outputs] -- submitted as ONE hipGraph launch instead of two or three stream calls. The executable graph is
    // built at the first tick and re-parameterised per tick (the pointers into the staging buffers move with the tick's counts).
    int tick_graph = 0;
    // PERSISTENT SINGLE TICK (round 6, k_tick_persistent): opt-in by ltpl_create_ex(LTPL_CREATE_PERSISTENT_TICK) or LTPL_PERSISTENT_TICK=1
    struct PersistTick {
        int enabled = 0;                    // requested AND the lattice's four-wave kernel has a compile-time LDS plan
        int running = 0, variant = -1; size_t lds = 0;
        TickMailbox* mb = nullptr;          // page-locked
        TickKArgs* d_args = nullptr;        // device copy of the argument block (the resident kernel's "kernarg segment")
        hipStream_t stream = nullptr;
        const void* h_in = nullptr; void* d_in = nullptr;      // staging buffers the resident kernel was started on
        unsigned seq = 0;
        double idle_ms = 250.0;             // LTPL_PERSIST_IDLE_MS: the kernel leaves by itself after this long without a tick
        unsigned long long ticks = 0, launches = 0;            // served ticks, kernel starts (1 + restarts after idling out / other entry points)
        unsigned long long busy_clk = 0, busy_n = 0;           // device-side time of completed residencies (wall_clock64 ticks), their ticks
    } pt;
    hipGraph_t tg_graph = nullptr; hipGraphExec_t tg_exec = nullptr;
    hipGraphNode_t tg_n_in = nullptr, tg_n_k = nullptr, tg_n_out = nullptr;
    const void* tg_func = nullptr; int tg_has_out = 0;
};

#define HIP_TRY(h, call)                                                                                              \
    do {                                                                                                              \
        hipError_t e_ = (call);                                                                                       \
        if (e_ != hipSuccess) {                                                                                       \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                                             \
            return LTPL_ERR_HIP;                                                                                      \
        }                                                                                                             \
    } while (0)

static const void* paths_kernel_of(const ltpl_handle* h, int nw)
{
    if (nw == 1) {
        if (h->long_horizon) return reinterpret_cast<const void*>(k_paths<1, PlanRtG>);
        switch (h->plan_class) {
            case 1: return reinterpret_cast<const void*>(k_paths<1, PlanA>);
            case 2: return reinterpret_cast<const void*>(k_paths<1, PlanB>);
            case 3: return reinterpret_cast<const void*>(k_paths<1, PlanC>);
            default: return reinterpret_cast<const void*>(k_paths<1, PlanRt>);
        }
    }
    if (h->long_horizon) return reinterpret_cast<const void*>(k_paths<NUM_WAVES, PlanRtG>);
    return h->plan_class4 == 1 ? reinterpret_cast<const void*>(k_paths<NUM_WAVES, PlanA4>)
                               : reinterpret_cast<const void*>(k_paths<NUM_WAVES, PlanRt>);
}

// (mangled) symbol prefix of that kernel in the code object: what a profile is matched against (ltpl_paths_kernel_symbol)
static const char* paths_kernel_symbol_of(const ltpl_handle* h, int nw)
{
    if (nw == 1) {
        if (h->long_horizon) return "_Z7k_pathsILi1E7PlanRtGE";
        switch (h->plan_class) {
            case 1: return "_Z7k_pathsILi1E6PlanFxILi32ELi32ELi1EEE";
            case 2: return "_Z7k_pathsILi1E6PlanFxILi32ELi40ELi1EEE";
            case 3: return "_Z7k_pathsILi1E6PlanFxILi48ELi32ELi1EEE";
            default: return "_Z7k_pathsILi1E6PlanRtE";
        }
    }
    if (h->long_horizon) return "_Z7k_pathsILi4E7PlanRtGE";
    return h->plan_class4 == 1 ? "_Z7k_pathsILi4E6PlanFxILi32ELi32ELi4EEE" : "_Z7k_pathsILi4E6PlanRtE";
}
extern "C" const char* ltpl_paths_kernel_symbol(const ltpl_handle* h, int32_t team_waves)
{
    return h ? paths_kernel_symbol_of(h, team_waves == 4 ? NUM_WAVES : 1) : "";
}

// the path kernel with `nw` waves per scenario in the LDS plan class chosen for the lattice at ltpl_create
static int launch_paths(ltpl_handle* h, int nw, int n_scen, hipStream_t st, const DevPathsIn& di, const DevPathsOut& dout,
                        unsigned* mask_out = nullptr)
{
    TeamLds lp = nw == 1 ? h->lp1 : h->lp4;
    lp.mask_out = mask_out;
    if (h->long_horizon) {
        const size_t need = (size_t)lp.par_glob_stride * (size_t)n_scen;
        if (need > h->d_par_cap) {
            HIP_TRY(h, hipDeviceSynchronize());          // an earlier launch may still use the old slabs
            if (h->d_par) (void)hipFree(h->d_par);
            h->d_par = nullptr; h->d_par_cap = 0;
            HIP_TRY(h, hipMalloc(&h->d_par, need));
            h->d_par_cap = need;
        }
        lp.par_glob = static_cast<unsigned char*>(h->d_par);
    }
    const dim3 grid(n_scen), block(nw == 1 ? 64 : WG_THREADS);
    if (nw == 1) {
        if (h->long_horizon) hipLaunchKernelGGL((k_paths<1, PlanRtG>), grid, block, lp.total, st, h->lat, di, dout, lp);
        else switch (h->plan_class) {
            case 1: hipLaunchKernelGGL((k_paths<1, PlanA>), grid, block, lp.total, st, h->lat, di, dout, lp); break;
            case 2: hipLaunchKernelGGL((k_paths<1, PlanB>), grid, block, lp.total, st, h->lat, di, dout, lp); break;
            case 3: hipLaunchKernelGGL((k_paths<1, PlanC>), grid, block, lp.total, st, h->lat, di, dout, lp); break;
            default: hipLaunchKernelGGL((k_paths<1, PlanRt>), grid, block, lp.total, st, h->lat, di, dout, lp); break;
        }
    } else if (h->long_horizon) hipLaunchKernelGGL((k_paths<NUM_WAVES, PlanRtG>), grid, block, lp.total, st, h->lat, di, dout, lp);
    else if (h->plan_class4 == 1) hipLaunchKernelGGL((k_paths<NUM_WAVES, PlanA4>), grid, block, lp.total, st, h->lat, di, dout, lp);
    else hipLaunchKernelGGL((k_paths<NUM_WAVES, PlanRt>), grid, block, lp.total, st, h->lat, di, dout, lp);
    HIP_TRY(h, hipGetLastError());
    return LTPL_OK;
}

static void dbg_report(ltpl_handle* h, const char* what, int n_blocks)
{
    if (!h->d_dbg) return;
    std::vector<long long> v((size_t)256 * DBG_SLOTS);
    if (hipMemcpy(v.data(), h->d_dbg, v.size() * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return;
    int nb = n_blocks < 256 ? n_blocks : 256;
    fprintf(stderr, "[ltpl dbg] %s: mean cycles between stamps over %d blocks (wave: d01 d12 ...)\n", what, nb);
    for (int w = 0; w < 4; ++w) {
        fprintf(stderr, "[ltpl dbg]   wave %d:", w);
        for (int k = 0; k + 1 < 16; ++k) {
            double acc = 0; int cnt = 0;
            for (int b = 0; b < nb; ++b) {
                long long a = v[(size_t)b * DBG_SLOTS + w * 16 + k], c = v[(size_t)b * DBG_SLOTS + w * 16 + k + 1];
                if (a > 0 && c > a) { acc += (double)(c - a); ++cnt; }
            }
            fprintf(stderr, " %9.0f", cnt ? acc / cnt : 0.0);
        }
        fprintf(stderr, "\n");
    }
    (void)hipMemset(h->d_dbg, 0, v.size() * sizeof(long long));
}



static void dbg_report_lanes(ltpl_handle* h)
{
    if (!h->d_dbg) return;
    std::vector<long long> v((size_t)256 * DBG_SLOTS);
    if (hipMemcpy(v.data(), h->d_dbg, v.size() * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return;
    const char* names[3] = {"generic", "follow (controlled)", "follow (unconstrained)"};
    {
        double acc = 0; int cnt = 0;
        for (int r = 0; r < 64; ++r) { const long long* row = &v[(size_t)(128 + r) * DBG_SLOTS]; if (row[0] > 0 && row[8] > row[0]) { acc += (double)(row[8] - row[0]); ++cnt; } }
        fprintf(stderr, "[ltpl dbg] k_vel_lanes unconstrained profile: forward sweep %9.0f cycles (%d rows)\n", cnt ? acc / cnt : 0.0, cnt);
    }
    {
        fprintf(stderr, "[ltpl dbg] k_follow_prep mean cycles between stamps 0-1-2-3-4-5 (inputs | race line scan | path scan | foot points | sums):");
        for (int k = 0; k < 5; ++k) {
            double acc = 0; int cnt = 0;
            for (int r = 0; r < 64; ++r) { const long long* row = &v[(size_t)(192 + r) * DBG_SLOTS]; if (row[k] > 0 && row[k + 1] > row[k]) { acc += (double)(row[k + 1] - row[k]); ++cnt; } }
            fprintf(stderr, " %8.0f", cnt ? acc / cnt : 0.0);
        }
        fprintf(stderr, "\n");
    }
    for (int g = 0; g < 3; ++g) {
        fprintf(stderr, "[ltpl dbg] k_vel_lanes %-24s mean cycles between stamps 0-1-2-3-4-5-6, total:", names[g]);
        double tot = 0; int tc = 0;
        for (int k = 0; k < 6; ++k) {
            double acc = 0; int cnt = 0;
            for (int r = 0; r < 64; ++r) {
                const long long* row = &v[(size_t)(g * 64 + r) * DBG_SLOTS];
                int k2 = k + 1; while (k2 < 7 && row[k2] == 0) ++k2;
                if (row[k] > 0 && k2 < 7 && row[k2] > row[k] && (k2 == k + 1)) { acc += (double)(row[k2] - row[k]); ++cnt; }
            }
            fprintf(stderr, " %9.0f", cnt ? acc / cnt : 0.0);
        }
        for (int r = 0; r < 64; ++r) { const long long* row = &v[(size_t)(g * 64 + r) * DBG_SLOTS]; if (row[0] > 0 && row[6] > row[0]) { tot += (double)(row[6] - row[0]); ++tc; } }
        fprintf(stderr, " | %9.0f (%d rows)\n", tc ? tot / tc : 0.0, tc);
    }
    (void)hipMemset(h->d_dbg, 0, v.size() * sizeof(long long));
}

template <typename T>
static int upload(ltpl_handle* h, const T* src, size_t n, const T** dst)
{
    void* p = nullptr;
    size_t bytes = (n ? n : 1) * sizeof(T);
    HIP_TRY(h, hipMalloc(&p, bytes));
    h->dev_allocs.push_back(p);
    if (n) HIP_TRY(h, hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    *dst = static_cast<const T*>(p);
    return LTPL_OK;
}

// LDS of one workgroup of the fused tick kernel (k_tick, k_tick_persistent): fused_tick_lds (vel_layout.hpp), cap = max_path_pts rows. ltpl_create
// routes every tick of a lattice whose footprint is above this budget to the pipeline; tick_prepare launches the fused kernel with exactly that much.
static const size_t FUSED_TICK_LDS_BUDGET = 150 * 1024;

// planning-range statistics over all start layers (sizes the LDS plan and the output capacities)
static int horizon_stats(const ltpl_lattice_desc* d, int* hmax, int* ehmax, int* nhmax, int* ptsmax, int* kmax,
                         int* degmax, int* etmax, std::vector<int>* rng_end, std::string* why)
{
    const int L = d->num_layers;
    std::vector<int> edges_into(L, 0), maxsamp_into(L, 0);
    *kmax = 0; *degmax = 0;
    for (int l = 0; l < L; ++l) {
        int K = d->layer_node_off[l + 1] - d->layer_node_off[l];
        if (K > *kmax) *kmax = K;
        for (int v = d->layer_node_off[l]; v < d->layer_node_off[l + 1]; ++v) {
            int deg = d->in_ptr[v + 1] - d->in_ptr[v];
            if (deg > *degmax) *degmax = deg;
            edges_into[l] += deg;
            for (int e = d->in_ptr[v]; e < d->in_ptr[v + 1]; ++e) {
                if (!(d->edge_cost[e] >= 0.0)) { *why = "negative or NaN edge cost"; return LTPL_ERR_INVALID_ARG; }
                int ns = d->samp_ptr[e + 1] - d->samp_ptr[e];
                if (ns < 2) { *why = "edge with fewer than 2 samples"; return LTPL_ERR_INVALID_ARG; }
                if (ns > maxsamp_into[l]) maxsamp_into[l] = ns;
                int pl = (l + L - 1) % L;
                if (d->edge_src[e] < 0 || d->edge_src[e] >= d->layer_node_off[pl + 1] - d->layer_node_off[pl]) {
                    *why = "edge_src out of range"; return LTPL_ERR_INVALID_ARG;
                }
            }
        }
    }
    *hmax = *ehmax = *nhmax = *ptsmax = 0; *etmax = 0;
    for (int l = 0; l < L; ++l) if (edges_into[l] > *etmax) *etmax = edges_into[l];
    rng_end->assign((size_t)L, 0);
    for (int sl = 0; sl < L; ++sl) {
        int el;
        if (d->plan_horizon_mode == 0) {                             // gen_local_node_template.py:104-124
            double des = d->s_raceline[sl] + d->min_plan_horizon;
            if (des > d->s_raceline[L - 1]) { if (d->closed) des -= d->s_raceline[L - 1]; else des = d->s_raceline[L - 1]; }
            int lo = 0, hi = L;
            while (lo < hi) { int mid = (lo + hi) / 2; if (d->s_raceline[mid] < des) lo = mid + 1; else hi = mid; }
            el = lo;
        } else if (d->closed) el = (sl + (int)d->min_plan_horizon) % L;
        else el = std::max(sl + (int)d->min_plan_horizon, L - 1);    // :131-133 (sic: max)
        if (el >= L) {
            if (!d->closed) { (*rng_end)[(size_t)sl] = -1; continue; }   // the reference fails for this start layer (GraphBase.py:889)
            *why = "planning horizon runs past the last layer (track shorter than the horizon?)"; return LTPL_ERR_UNSUPPORTED;
        }
        (*rng_end)[(size_t)sl] = el;
        int H = el - sl; if (H < 0) H = L - sl + el;
        if (!d->closed) {
            if (H <= 0) { (*rng_end)[(size_t)sl] = -1; continue; }       // last layer of an open track: empty planning range
        } else if (H <= 0 || H >= L - 1) { *why = "planning range covers the whole track; not supported"; return LTPL_ERR_UNSUPPORTED; }
        int eh = 0, nh = d->layer_node_off[sl + 1] - d->layer_node_off[sl], pts = 1;
        for (int j = 1; j <= H; ++j) {
            int b = (sl + j) % L;
            eh += edges_into[b]; nh += d->layer_node_off[b + 1] - d->layer_node_off[b];
            pts += maxsamp_into[b] - 1;
        }
        if (H + 1 > *hmax) *hmax = H + 1;
        if (eh > *ehmax) *ehmax = eh;
        if (nh > *nhmax) *nhmax = nh;
        if (pts > *ptsmax) *ptsmax = pts;
    }
    return LTPL_OK;
}

// "No C++ exception crosses the ABI" (include/ltpl_hip.h): every entry point that allocates is a function-try-block; an exception
// (std::bad_alloc / std::length_error of a host container in practice) becomes LTPL_ERR_EXCEPTION with the message in the handle's
// (or the thread's create-time) error string.
static int abi_caught(std::string* err, const char* what) noexcept
{
    try { (err ? *err : g_create_error) = std::string("C++ exception caught at the ABI: ") + what; } catch (...) {}
    return LTPL_ERR_EXCEPTION;
}
static std::string* abi_err_of(const ltpl_handle* h) { return h ? const_cast<std::string*>(&h->err) : nullptr; }
static std::string* abi_err_of(const ltpl_planner* p) { return p ? const_cast<std::string*>(&p->P.err) : nullptr; }
#define LTPL_ABI_CATCH(errptr) \
    catch (const std::exception& e) { return abi_caught(errptr, e.what()); } \
    catch (...) { return abi_caught(errptr, "unknown exception"); }

extern "C" int ltpl_version(void) { return LTPL_ABI_VERSION; }

static void persist_stop(ltpl_handle* h);      // (the resident single-tick kernel leaves: defined next to ltpl_tick_batch)

extern "C" const char* ltpl_last_error(const ltpl_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

extern "C" int ltpl_destroy(ltpl_handle* h)
{
    if (!h) return LTPL_ERR_INVALID_ARG;
    if (h->n_planners > 0) { h->err = "ltpl_destroy: planners created on this handle are still alive (destroy them first)"; return LTPL_ERR_INVALID_ARG; }
    (void)hipSetDevice(h->device);
    persist_stop(h);
    if (h->pt.stream) (void)hipStreamDestroy(h->pt.stream);
    if (h->pt.mb) (void)hipHostFree(h->pt.mb);
    if (h->pt.d_args) (void)hipFree(h->pt.d_args);
    for (void* p : h->dev_allocs) (void)hipFree(p);
    if (h->d_in) (void)hipFree(h->d_in);
    if (h->d_out) (void)hipFree(h->d_out);
    if (h->d_dbg) (void)hipFree(h->d_dbg);
    if (h->d_planes) (void)hipFree(h->d_planes);
    if (h->d_par) (void)hipFree(h->d_par);
    for (int i = 0; i < ltpl_handle::PIPE_SETS - 1; ++i) {
        if (h->d_planes_x[i]) (void)hipFree(h->d_planes_x[i]);
        if (h->d_out_x[i]) (void)hipFree(h->d_out_x[i]);
        free_resident(h->resident_x[i]);
    }
    for (int i = 0; i < ltpl_handle::VEL_STREAMS; ++i) if (h->vel_stream[i]) (void)hipStreamDestroy(h->vel_stream[i]);
    if (h->path_stream2) (void)hipStreamDestroy(h->path_stream2);
    if (h->ev_begin) (void)hipEventDestroy(h->ev_begin);
    for (int i = 0; i < ltpl_handle::PIPE_SETS; ++i) { if (h->ev_paths[i]) (void)hipEventDestroy(h->ev_paths[i]); if (h->ev_vel[i]) (void)hipEventDestroy(h->ev_vel[i]); }
    for (hipEvent_t e : h->ev_step) (void)hipEventDestroy(e);
    if (h->h_in) (void)hipHostFree(h->h_in);
    if (h->h_out) (void)hipHostFree(h->h_out);
    if (h->h_flag) (void)hipHostFree(h->h_flag);
    if (h->d_done_cnt) (void)hipFree(h->d_done_cnt);
    if (h->tg_exec) (void)hipGraphExecDestroy(h->tg_exec);
    if (h->tg_graph) (void)hipGraphDestroy(h->tg_graph);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    free_resident(h->resident);
    delete h;
    return LTPL_OK;
}

extern "C" int ltpl_create(const ltpl_lattice_desc* d, int device, ltpl_handle** out_handle)
{
    return ltpl_create_ex(d, device, 0u, out_handle);
}

extern "C" int ltpl_create_ex(const ltpl_lattice_desc* d, int device, uint32_t flags, ltpl_handle** out_handle)
try {
    g_create_error.clear();
    if (flags & ~(uint32_t)LTPL_CREATE_PERSISTENT_TICK) { g_create_error = "ltpl_create_ex: unknown flag"; return LTPL_ERR_INVALID_ARG; }
    if (!d || !out_handle) { g_create_error = "null argument"; return LTPL_ERR_INVALID_ARG; }
    if (d->num_layers < 4 || d->num_nodes < 1 || d->num_edges < 1) { g_create_error = "empty lattice"; return LTPL_ERR_INVALID_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_create_error = "no HIP device visible"; return LTPL_ERR_NO_DEVICE; }
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    if (device >= ndev) { g_create_error = "device index out of range"; return LTPL_ERR_NO_DEVICE; }

    int hmax, ehmax, nhmax, ptsmax, kmax, degmax, etmax;
    std::vector<int> rng_end;
    int rc = horizon_stats(d, &hmax, &ehmax, &nhmax, &ptsmax, &kmax, &degmax, &etmax, &rng_end, &g_create_error);
    if (rc) return rc;
    if (hmax < 2) { g_create_error = "no start layer with a planning range"; return LTPL_ERR_INVALID_ARG; }
    if (etmax > 65535) { g_create_error = "more than 65535 edges in one layer transition"; return LTPL_ERR_CAPACITY; }
    if (kmax > 255 || degmax > 127) { g_create_error = "more than 255 nodes per layer or 127 in-edges per node"; return LTPL_ERR_CAPACITY; }

    ltpl_handle* h = new ltpl_handle();
    h->device = device;
    h->rng_end_host = rng_end;
    struct Guard { ltpl_handle* h; ~Guard() { if (h) ltpl_destroy(h); } } guard{h};     // error returns and exceptions release the handle
    auto fail = [&](int code) { g_create_error = h->err; return code; };
    if (hipSetDevice(device) != hipSuccess) { h->err = "hipSetDevice failed"; return fail(LTPL_ERR_HIP); }
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { h->err = "hipStreamCreate failed"; return fail(LTPL_ERR_HIP); }

    DevLat& L = h->lat;
    L.L = d->num_layers; L.V = d->num_nodes; L.E = d->num_edges; L.S = d->num_samples; L.G = d->num_glob_rl;
    L.mode = d->plan_horizon_mode; L.closed = d->closed ? 1 : 0; L.min_plan_horizon = d->min_plan_horizon; L.veh_width = d->veh_width;
    L.sampled_resolution = d->sampled_resolution; L.lat_offset = d->lat_offset;
    L.vel_decrease_lat = d->vel_decrease_lat; L.veh_length = d->veh_length;
#define UP(field, src, n) if ((rc = upload(h, src, (size_t)(n), &L.field)) != LTPL_OK) return fail(rc)
    UP(layer_off, d->layer_node_off, L.L + 1); UP(rl_idx, d->raceline_index, L.L);
    UP(s_rl, d->s_raceline, L.L); UP(ref_x, d->refline_x, L.L); UP(ref_y, d->refline_y, L.L);
    UP(vel_rl, d->vel_raceline, L.L);
    UP(node_x, d->node_x, L.V); UP(node_y, d->node_y, L.V); UP(vgoal, d->vgoal_cost, L.V);
    UP(in_ptr, d->in_ptr, L.V + 1); UP(edge_src, d->edge_src, L.E);
    UP(edge_cost, d->edge_cost, L.E);
    UP(edge_len, d->edge_len, L.E); UP(samp_ptr, d->samp_ptr, L.E + 1);
    UP(sx, d->samp_x, L.S); UP(sy, d->samp_y, L.S); UP(spsi, d->samp_psi, L.S); UP(slen, d->samp_len, L.S);
    UP(glob_rl, d->glob_rl, (size_t)L.G * 5);
    {
        std::vector<double> sc(2 * (size_t)L.S + 2, 0.0);
        for (int k = 0; k < L.S; ++k) { sc[2 * (size_t)k] = sin(d->samp_psi[k]); sc[2 * (size_t)k + 1] = cos(d->samp_psi[k]); }
        UP(ssc, sc.data(), 2 * (size_t)L.S + 2);
    }
    {
        std::vector<double> gx((size_t)L.G), gy((size_t)L.G);
        for (int k = 0; k < L.G; ++k) { gx[(size_t)k] = d->glob_rl[(size_t)k * 5 + 1]; gy[(size_t)k] = d->glob_rl[(size_t)k * 5 + 2]; }
        UP(grx, gx.data(), L.G); UP(gry, gy.data(), L.G);
    }
    {
        // derived tables: planning range per start layer, first edge into every layer, byte-wide edge sources
        std::vector<int> ebase((size_t)L.L + 1);
        for (int l = 0; l <= L.L; ++l) ebase[(size_t)l] = d->in_ptr[d->layer_node_off[l]];
        std::vector<unsigned char> src8((size_t)L.E + 16, (unsigned char)0xff);   // padded: path assembly reads 16 bytes at a time
        for (int e = 0; e < L.E; ++e) src8[(size_t)e] = (unsigned char)d->edge_src[e];
        std::vector<unsigned char> dst8((size_t)L.E);
        for (int l = 0; l < L.L; ++l)
            for (int v = d->layer_node_off[l]; v < d->layer_node_off[l + 1]; ++v)
                for (int e = d->in_ptr[v]; e < d->in_ptr[v + 1]; ++e) dst8[(size_t)e] = (unsigned char)(v - d->layer_node_off[l]);
        UP(rng_end, rng_end.data(), L.L); UP(layer_ebase, ebase.data(), L.L + 1); UP(edge_src8, src8.data(), L.E + 16);
        UP(edge_dst8, dst8.data(), L.E);
        std::vector<unsigned char> rank8((size_t)L.E);
        for (int v = 0; v < L.V; ++v)
            for (int e = d->in_ptr[v]; e < d->in_ptr[v + 1]; ++e) rank8[(size_t)e] = (unsigned char)(e - d->in_ptr[v]);
        UP(edge_rank8, rank8.data(), L.E);
        {
            // path assembly records (see DevLat; csrc/assembly_records.hpp)
            std::vector<int32_t> nrec; std::vector<double> erec;
            ltplrec::build(L.V, L.E, d->in_ptr, d->edge_src, d->edge_len, d->samp_ptr, d->samp_x, d->samp_y, d->samp_psi, nrec, erec);
            const int4* nr = nullptr;
            if ((rc = upload(h, reinterpret_cast<const int4*>(nrec.data()), (size_t)L.V, &nr)) != LTPL_OK) return fail(rc);
            L.node_rec = nr;
            UP(edge_rec, erec.data(), (size_t)L.E * LTPL_EDGE_REC);
        }
        std::vector<int> ldeg((size_t)L.L, 0);
        for (int l = 0; l < L.L; ++l)
            for (int v = d->layer_node_off[l]; v < d->layer_node_off[l + 1]; ++v)
                ldeg[(size_t)l] = std::max(ldeg[(size_t)l], d->in_ptr[v + 1] - d->in_ptr[v]);
        UP(layer_degmax, ldeg.data(), L.L);
        // sweep order (see DevLat): per transition sorted by (rank, destination); cost / meta with the sentinel at index E
        h->sw2csc_host.resize((size_t)L.E);
        std::vector<int> csc2sw((size_t)L.E);
        for (int l = 0; l < L.L; ++l) {
            const int e0 = ebase[(size_t)l], e1 = ebase[(size_t)l + 1];
            for (int e = e0; e < e1; ++e) h->sw2csc_host[(size_t)e] = e;
            std::stable_sort(h->sw2csc_host.begin() + e0, h->sw2csc_host.begin() + e1, [&](int a, int b) {
                if (rank8[(size_t)a] != rank8[(size_t)b]) return rank8[(size_t)a] < rank8[(size_t)b];
                return dst8[(size_t)a] < dst8[(size_t)b];
            });
        }
        // (LTPL_SW_PAD sentinel entries behind the last edge: the sweep's prefetch reads whole 64-edge chunks from a transition's first edge
        //  on and replaces what lies beyond the transition by the sentinel in registers -- behind the LAST transition it reads these)
        std::vector<double> swc((size_t)L.E + 1 + LTPL_SW_PAD, (double)INFINITY);
        std::vector<unsigned> swm((size_t)L.E + 1 + LTPL_SW_PAD, 0u);
        for (int p = 0; p < L.E; ++p) {
            const int e = h->sw2csc_host[(size_t)p];
            csc2sw[(size_t)e] = p; swc[(size_t)p] = d->edge_cost[e];
            swm[(size_t)p] = (unsigned)rank8[(size_t)e] | ((unsigned)src8[(size_t)e] << 8) | ((unsigned)dst8[(size_t)e] << 16);
        }
        swc[(size_t)L.E] = INFINITY;
        UP(sw_cost, swc.data(), L.E + 1 + LTPL_SW_PAD); UP(sw_meta, swm.data(), L.E + 1 + LTPL_SW_PAD);
        UP(sw2csc, h->sw2csc_host.data(), L.E); UP(csc2sw, csc2sw.data(), L.E);
        if (d->normvec_x && d->normvec_y && d->width_right && d->width_left) {
            // ObjectListInterface.py:71-72 and check_inside_bounds.py:27 (same operations, no contraction)
            std::vector<double> b1x((size_t)L.L), b1y((size_t)L.L), b2x((size_t)L.L), b2y((size_t)L.L), cx((size_t)L.L), cy((size_t)L.L);
            for (int l = 0; l < L.L; ++l) {
                b1x[(size_t)l] = d->refline_x[l] + d->normvec_x[l] * d->width_right[l]; b1y[(size_t)l] = d->refline_y[l] + d->normvec_y[l] * d->width_right[l];
                b2x[(size_t)l] = d->refline_x[l] - d->normvec_x[l] * d->width_left[l]; b2y[(size_t)l] = d->refline_y[l] - d->normvec_y[l] * d->width_left[l];
                cx[(size_t)l] = (b1x[(size_t)l] + b2x[(size_t)l]) / 2; cy[(size_t)l] = (b1y[(size_t)l] + b2y[(size_t)l]) / 2;
            }
            UP(b1x, b1x.data(), L.L); UP(b1y, b1y.data(), L.L); UP(b2x, b2x.data(), L.L); UP(b2y, b2y.data(), L.L);
            UP(ctx, cx.data(), L.L); UP(cty, cy.data(), L.L);
        }
        // capsule per edge (two-sided cull of the obstacle mask, paths_team.hpp phase 2; construction and its conservativeness
        // argument in capsule.hpp)
        std::vector<float4> cap((size_t)L.E * 2), cap_sw((size_t)L.E * 2);
        L.cull_slack = ltplcap::build(L.E, d->samp_ptr, d->samp_x, d->samp_y, L.S, reinterpret_cast<float*>(cap.data()));
        for (int p = 0; p < L.E; ++p) {                         // the mask phase walks a transition in sweep order
            const size_t e = (size_t)h->sw2csc_host[(size_t)p];
            cap_sw[2 * (size_t)p] = cap[2 * e]; cap_sw[2 * (size_t)p + 1] = cap[2 * e + 1];
        }
        UP(edge_cap, cap_sw.data(), (size_t)L.E * 2);
        // closest-layer grid of phase 1 (layer_grid.hpp: construction and conservativeness argument; tests/test_layer_grid.py)
        L.lgrid = nullptr; L.lg_x0 = L.lg_y0 = L.lg_inv = 0.0; L.lg_nx = L.lg_ny = 0;
        if (!getenv("LTPL_NO_LAYER_GRID")) {
            const ltplgrid::Grid g = ltplgrid::build(L.L, d->refline_x, d->refline_y);
            if (g.nx > 0 && g.ny > 0) {
                UP(lgrid, reinterpret_cast<const int4*>(g.cells.data()), (size_t)g.nx * g.ny);
                L.lg_x0 = g.x0; L.lg_y0 = g.y0; L.lg_inv = g.inv_cell; L.lg_nx = g.nx; L.lg_ny = g.ny;
            }
        }
    }
#undef UP

    auto make_plan = [&](int nw, TeamLds* lp, bool par_in_global) {
        lp->kpad = (int)align_up((size_t)kmax, 4);
        lp->hmax = hmax + 1;
        lp->etmax = etmax;
        lp->words_blocked = (ehmax + 31) / 32 + 1;
        lp->words_zone = (nhmax + 31) / 32 + 1;
        lp->n_path_bufs = nw < LTPL_MAX_ACTIONS ? nw : LTPL_MAX_ACTIONS;
        size_t off = 0;
        lp->off_dist = (int)off; off += sizeof(double) * NFILT * 2 * lp->kpad;
        lp->off_cnt = (int)off; off += sizeof(unsigned) * NFILT * lp->kpad;
        lp->off_widx = (int)off; off += sizeof(unsigned) * NFILT * lp->kpad; off = align_up(off, 16);
        lp->off_dumin = (int)off; off += sizeof(double) * NFILT * lp->kpad;
        lp->path_stride = (int)align_up(sizeof(double) * 7 * lp->hmax + sizeof(int) * 2 * (lp->hmax + 1), 16);
        if (lp->n_path_bufs == 1) {
            // one-wave teams: the path scratch aliases the sweep's frontier / election arrays (dead during path assembly)
            lp->off_path = lp->off_dist;
            if ((size_t)lp->path_stride > off - (size_t)lp->off_dist) off = (size_t)lp->off_dist + (size_t)lp->path_stride;
        } else {
            lp->off_path = (int)off; off += (size_t)lp->path_stride * lp->n_path_bufs;
        }
        lp->off_best = (int)off; off += sizeof(int) * NFILT * lp->hmax; off = align_up(off, 16);
        lp->off_blocked = (int)off; off += sizeof(unsigned) * lp->words_blocked; off = align_up(off, 16);
        lp->off_zone = (int)off; off += sizeof(unsigned) * lp->words_zone; off = align_up(off, 16);
        const size_t par_bytes = sizeof(uchar2) * NPAR * (size_t)lp->hmax * lp->kpad;
        lp->off_par = (int)off; if (!par_in_global) { off += par_bytes; off = align_up(off, 16); }
        lp->ref_lds = (!par_in_global && sizeof(double) * 2 * (size_t)d->num_layers <= par_bytes) ? 1 : 0;
        lp->par_glob = nullptr; lp->par_glob_stride = par_in_global ? (long long)align_up(par_bytes, 256) : 0;
        lp->off_lay = (int)off; off += sizeof(int) * 4 * (size_t)lp->hmax;
        lp->off_pos_layer = (int)off; off += sizeof(short) * MAX_POS; off = align_up(off, 16);
        lp->off_pos_veh = (int)off; off += MAX_POS; off = align_up(off, 16);
        // shell list of the obstacle mask (phase 2): 128 entries of 8 bytes per wave (runtime plans: own storage)
        lp->shell_cap = 128; lp->off_shell = (int)off; off += (size_t)8 * 128 * nw; off = align_up(off, 16);
        lp->total = (int)off;
        lp->mask_out = nullptr;
        lp->ablate = 0; lp->poison_on = 0; lp->poison = 0u; lp->dbg = nullptr;
#ifdef LTPL_EXPERIMENT
        lp->ablate = getenv("LTPL_ABLATE") ? atoi(getenv("LTPL_ABLATE")) : 0;
        lp->poison_on = getenv("LTPL_LDS_POISON") ? 1 : 0;
        lp->poison = lp->poison_on ? (unsigned)strtoul(getenv("LTPL_LDS_POISON"), nullptr, 0) : 0u;
#endif
    };
    make_plan(1, &h->lp1, false); make_plan(NUM_WAVES, &h->lp4, false);
    const int lds_limit = 150 * 1024;
    if (h->lp4.total > lds_limit || h->lp1.total > lds_limit || getenv("LTPL_FORCE_LONG_HORIZON")) {
        // long planning horizons: the parent tables move to global memory, the path scratch stays in LDS
        h->long_horizon = 1;
        make_plan(1, &h->lp1, true); make_plan(NUM_WAVES, &h->lp4, true);
    }
    // compile-time plan classes of the one-wave batch kernel: same arrays, hot offsets taken from the policy (PlanFx)
    auto make_fixed_plan = [&](auto plan_tag, TeamLds* lp) {       // *lp holds the runtime plan of the same team size
        typedef decltype(plan_tag) PL;
        lp->kpad = PL::c_kpad; lp->hmax = PL::c_hmax; lp->n_path_bufs = PL::c_n_path_bufs;
        lp->off_dist = PL::c_off_dist; lp->off_cnt = PL::c_off_cnt; lp->off_widx = PL::c_off_widx; lp->off_dumin = PL::c_off_dumin;
        lp->path_stride = PL::c_path_stride; lp->off_path = PL::c_off_path; lp->off_best = PL::c_off_best;
        lp->off_par = PL::c_off_par; lp->off_lay = PL::c_off_lay;
        // the shell list of phase 2 lives in the frontier / election arrays (not written before phase 4)
        lp->off_shell = PL::c_off_dist;
        lp->shell_cap = (PL::c_end_elect - PL::c_off_dist) / 8 / (PL::c_n_path_bufs == 1 ? 1 : NUM_WAVES);
        size_t off = (size_t)PL::c_fixed_end;
        lp->off_blocked = (int)off; off += sizeof(unsigned) * lp->words_blocked; off = align_up(off, 16);
        lp->off_zone = (int)off; off += sizeof(unsigned) * lp->words_zone; off = align_up(off, 16);
        lp->ref_lds = (sizeof(double) * 2 * (size_t)d->num_layers <= (size_t)PL::c_par_bytes) ? 1 : 0;
        // the per-position tables are dead once phase 3 is over, the parent table is not written before phase 4: they
        // share its storage (behind the staged reference line) when they fit
        const size_t ref_bytes = lp->ref_lds ? align_up(sizeof(double) * 2 * (size_t)d->num_layers, 16) : 0;
        const size_t pos_bytes = align_up(sizeof(short) * MAX_POS, 16) + align_up((size_t)MAX_POS, 16);
        if (ref_bytes + pos_bytes <= (size_t)PL::c_par_bytes) {
            lp->off_pos_layer = lp->off_par + (int)ref_bytes;
            lp->off_pos_veh = lp->off_pos_layer + (int)align_up(sizeof(short) * MAX_POS, 16);
        } else {
            lp->off_pos_layer = (int)off; off += sizeof(short) * MAX_POS; off = align_up(off, 16);
            lp->off_pos_veh = (int)off; off += MAX_POS; off = align_up(off, 16);
        }
        lp->total = (int)off;
    };
    if (!getenv("LTPL_NO_FIXED_PLAN") && !h->long_horizon) {
        if (kmax <= PlanA::c_kpad && hmax + 1 <= PlanA::c_hmax && d->num_layers >= PlanA::c_hmax) {
            h->plan_class = 1; make_fixed_plan(PlanA(), &h->lp1);
            h->plan_class4 = 1; make_fixed_plan(PlanA4(), &h->lp4);
        }
        else if (kmax <= PlanB::c_kpad && hmax + 1 <= PlanB::c_hmax && d->num_layers >= PlanB::c_hmax) { h->plan_class = 2; make_fixed_plan(PlanB(), &h->lp1); }
        else if (kmax <= PlanC::c_kpad && hmax + 1 <= PlanC::c_hmax && d->num_layers >= PlanC::c_hmax) { h->plan_class = 3; make_fixed_plan(PlanC(), &h->lp1); }
    }
    // between the two limits (the plan fits, plan + velocity scratch does not: C5 at 0.5 m spacing with a 120 .. 190 m horizon) the fused
    // tick cannot run: the pipeline serves every batch size there, as it does in the long-horizon mode
    h->fused_fits = (!h->long_horizon && fused_tick_lds(h->lp4.total, (int)align_up((size_t)ptsmax, 16)) <= FUSED_TICK_LDS_BUDGET) ? 1 : 0;
    if (const char* e = getenv("LTPL_BATCH_NW")) h->batch_nw = atoi(e) == 4 ? 4 : 1;
    h->zc_out = 1;
    if (const char* e = getenv("LTPL_ZC_OUT")) h->zc_out = atoi(e);
    if (const char* e = getenv("LTPL_ZC_IN")) h->zc_in = atoi(e);
    if (const char* e = getenv("LTPL_POLL")) h->poll = atoi(e);
    if (const char* e = getenv("LTPL_TICK_GRAPH")) h->tick_graph = atoi(e);
    if (const char* e = getenv("LTPL_POLL_SYNC_EVERY")) h->poll_sync_every = atoi(e);
    if (const char* e = getenv("LTPL_POLL_QUERY")) h->poll_query = atoi(e);
    // the persistent single tick: requested by flag or environment, engaged where the four-wave kernel has a compile-time LDS plan
    {
        const char* e = getenv("LTPL_PERSISTENT_TICK");
        const bool want = (flags & LTPL_CREATE_PERSISTENT_TICK) != 0u || (e && atoi(e) != 0);
        h->pt.enabled = (want && h->plan_class4 == 1 && h->fused_fits && h->zc_out) ? 1 : 0;
        if (const char* m = getenv("LTPL_PERSIST_IDLE_MS")) { const double v = atof(m); if (v > 0.0) h->pt.idle_ms = v; }
    }
    if (h->poll || h->pt.enabled) {
        if (hipHostMalloc(reinterpret_cast<void**>(&h->h_flag), 64, hipHostMallocDefault) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&h->d_done_cnt), 64) != hipSuccess ||
            hipMemset(h->d_done_cnt, 0, 64) != hipSuccess) { h->err = "cannot allocate the completion word"; return fail(LTPL_ERR_HIP); }
        *h->h_flag = 0u;
    }
    // environment switches are read ONCE here: getenv() in a per-tick entry point costs microseconds in a process with a large environment
#ifdef LTPL_EXPERIMENT
    if (const char* e = getenv("LTPL_SCRATCH_POISON")) { h->scratch_poison_on = 1; h->scratch_poison_word = (unsigned)strtoul(e, nullptr, 0); }
    if (const char* e = getenv("LTPL_EXP_SKIP")) h->exp_skip = atoi(e);
#endif
    h->force_fused = getenv("LTPL_FORCE_FUSED") ? 1 : 0;
    h->no_overlap = getenv("LTPL_NO_OVERLAP") ? 1 : 0;
    if (const char* e = getenv("LTPL_FINAL_Y")) h->final_y = atoi(e) > 0 ? atoi(e) : 8;
    if (const char* e = getenv("LTPL_NW1_MIN_SCEN")) h->nw1_min_scen = atoi(e) > 0 ? atoi(e) : PIPELINE_MIN_SCEN;
#ifdef LTPL_EXPERIMENT
    if (getenv("LTPL_DEBUG_TIMING")) {
        if (hipMalloc(reinterpret_cast<void**>(&h->d_dbg), sizeof(long long) * 256 * DBG_SLOTS) == hipSuccess) {
            (void)hipMemset(h->d_dbg, 0, sizeof(long long) * 256 * DBG_SLOTS);
            h->lp1.dbg = h->d_dbg; h->lp4.dbg = h->d_dbg;
        }
    }
#endif
    if (h->lp4.total > lds_limit || h->lp1.total > lds_limit) {
        h->err = "planning horizon too large: the path scratch of the sweep does not fit in LDS (" + std::to_string(h->lp4.total) + " B > 150 KiB)";
        return fail(LTPL_ERR_CAPACITY);
    }
    if (h->lp4.total > 48 * 1024 || h->lp1.total > 48 * 1024) {
        if (hipFuncSetAttribute(paths_kernel_of(h, 1), hipFuncAttributeMaxDynamicSharedMemorySize,
                                h->lp1.total) != hipSuccess ||
            hipFuncSetAttribute(paths_kernel_of(h, NUM_WAVES), hipFuncAttributeMaxDynamicSharedMemorySize,
                                h->lp4.total) != hipSuccess) { h->err = "cannot raise dynamic LDS limit"; return fail(LTPL_ERR_HIP); }
    }
#ifdef LTPL_EXPERIMENT
    if (getenv("LTPL_DEBUG_OCC"))
#else
    if (false)
#endif
    {
        int nb1 = -1, nb4 = -1;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb1, paths_kernel_of(h, 1), 64, (size_t)h->lp1.total);
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb4, paths_kernel_of(h, NUM_WAVES), WG_THREADS, (size_t)h->lp4.total);
        fprintf(stderr, "[ltpl occ] k_paths<1> (plan class %d): %d blocks/CU at %d B LDS; k_paths<4>: %d blocks/CU at %d B LDS\n", h->plan_class, nb1, h->lp1.total, nb4, h->lp4.total);
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { h->err = "hipGetDeviceProperties failed"; return fail(LTPL_ERR_HIP); }
    // capacity in rows rounded up to 16: a slot's row block of the fp64 outputs (vx, ax: 8 B per row; path_param: 40 B) then starts on a
    // 128-byte line, so the 128-byte chunks the final velocity kernel writes are whole sectors (measured write traffic was 1.8x the data)
    h->caps.max_path_nodes = hmax; h->caps.max_path_pts = (int)align_up((size_t)ptsmax, 16); h->caps.max_horizon_edges = ehmax;
    h->caps.device = device; h->caps.num_cus = prop.multiProcessorCount; h->caps.lds_bytes_paths = h->lp1.total;
    {
        // fused tick vs pipeline (see pipeline_min_scen): workgroups of the fused kernel that fit one compute unit by LDS (its footprint is
        // fused_tick_lds), at most two counted, against the 160 KiB of LDS of one compute unit. (Lattices whose footprint is above the budget
        // never run the fused tick: fused_fits.)
        const size_t lds_tick = fused_tick_lds(h->lp4.total, h->caps.max_path_pts);
        const int per_cu = 160 * 1024 / lds_tick >= 2 ? 2 : 1;
        h->pipeline_min_scen = (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256) * per_cu + 1;
        if (h->pipeline_min_scen < PIPELINE_MIN_SCEN) h->pipeline_min_scen = PIPELINE_MIN_SCEN;
        if (const char* e = getenv("LTPL_PIPELINE_MIN_SCEN")) { if (atoi(e) > 0) h->pipeline_min_scen = atoi(e); }
        if (const char* e = getenv("LTPL_FOLLOW_EMIT_MIN_SCEN")) { if (atoi(e) > 0) h->follow_emit_min_scen = atoi(e); }
        if (getenv("LTPL_NO_SCEN_ORDER")) h->scen_order = 0;
    }
    if (d->raceline_x && d->raceline_y && d->node_psi) {
        std::string why;
        h->has_hostlat = h->hostlat.init(d, h->caps.max_path_nodes, h->caps.max_path_pts, &why) == LTPL_OK;
    }
    if (!getenv("LTPL_NO_SELFTEST")) {
        if ((rc = self_test(h, d)) != LTPL_OK) return fail(rc);
    }
    guard.h = nullptr;
    *out_handle = h;
    return LTPL_OK;
} LTPL_ABI_CATCH(nullptr)

extern "C" int ltpl_get_caps(const ltpl_handle* h, ltpl_caps* caps)
{
    if (!h || !caps) return LTPL_ERR_INVALID_ARG;
    *caps = h->caps;
    return LTPL_OK;
}

// ---- staging arena ---------------------------------------------------------------------------------------------------
struct Arena {
    size_t size = 0;
    size_t add(size_t bytes) { size_t o = size; size = align_up(size + bytes, 256); return o; }   // arrays start on cache-line multiples
};
template <class T> static void bind_at(T*& p, unsigned char* base, size_t off) { p = reinterpret_cast<T*>(base + off); }      // p = the array `off` bytes behind base

// The device-resident batch of ltpl_batch_upload points into the staging buffers (d_in / d_out / d_planes). Every other
// entry point reuses (and may reallocate) them, so it drops the resident batch first: a later ltpl_batch_run / _download then
// fails with "no resident batch" instead of reading overwritten or freed memory.
static void drop_resident(ltpl_handle* h, bool keep_persistent_tick = false)
{
    // (a resident tick kernel reads the staging buffers too -- and would keep a device-wide synchronisation waiting: it leaves first)
    if (!keep_persistent_tick) persist_stop(h);
    if (h->resident || h->resident_x[0]) { persist_stop(h); (void)hipDeviceSynchronize(); }
    free_resident(h->resident); h->resident = nullptr;
    for (int i = 0; i < ltpl_handle::PIPE_SETS - 1; ++i) { free_resident(h->resident_x[i]); h->resident_x[i] = nullptr; }
}

// grow-only device buffer: when `need` exceeds its capacity it is freed and allocated anew with `alloc` bytes (default: exactly `need`); the
// contents are not kept. After a failed allocation the buffer is empty (null, capacity 0).
static int grow_device(ltpl_handle* h, void** p, size_t* cap, size_t need, size_t alloc = 0)
{
    if (need <= *cap) return LTPL_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    HIP_TRY(h, hipMalloc(p, alloc ? alloc : need));
    *cap = alloc ? alloc : need;
    return LTPL_OK;
}

// the staging pair of an entry point: page-locked host buffer + device buffer, both grown by half more than needed
static int ensure(ltpl_handle* h, void** hp, size_t* hcap, void** dp, size_t* dcap, size_t need)
{
    if (need > *hcap) {
        if (*hp) (void)hipHostFree(*hp);
        *hp = nullptr; *hcap = 0;
        size_t cap = align_up(need + need / 2, 4096);
        HIP_TRY(h, hipHostMalloc(hp, cap, hipHostMallocDefault));
        *hcap = cap;
    }
    return grow_device(h, dp, dcap, need, align_up(need + need / 2, 4096));
}

// The dynamic-LDS limit of a kernel is process-wide state per device: raised when a launch needs more than the default 48 KiB and more than
// the last value set, never lowered, not re-set per call. `slot`: the kernel's place in the table = LDS_SLOT_* + its velocity variant.
enum { LDS_SLOT_VEL = 0, LDS_SLOT_TICK = 8, LDS_SLOT_TICK_A = 16, LDS_SLOT_PTICK = 24, LDS_SLOTS = 32 };
static int raise_lds_limit(ltpl_handle* h, const void* func, size_t lds, int slot)
{
    static std::atomic<size_t> g_set[16][LDS_SLOTS];
    std::atomic<size_t>* cur = (unsigned)h->device < 16u ? &g_set[h->device][slot] : nullptr;      // (a device beyond the table: set every time)
    if (lds > 48 * 1024 && (!cur || lds > cur->load(std::memory_order_relaxed))) {
        HIP_TRY(h, hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (cur) *cur = lds;
    }
    return LTPL_OK;
}

struct InLayout {
    size_t w_last, start_layer, start_node, flags, last_action, const_closest, psi_s, veh_off, pos_off, veh_radius,
        pos_x, pos_y, zone_off, zone_gid, n_last, last_layer, last_node, order, total;
    int n_veh, n_pos, n_zone;
};

static int validate_and_layout(ltpl_handle* h, const ltpl_paths_in* in, InLayout* lo)
{
    if (!in || in->n_scen < 1) { h->err = "n_scen < 1"; return LTPL_ERR_INVALID_ARG; }
    const int n = in->n_scen;
    if (in->n_w_last < 0 || in->n_w_last > LTPL_MAX_LAST_NODES - 1) { h->err = "n_w_last out of range"; return LTPL_ERR_INVALID_ARG; }
    if (in->veh_off[0] != 0 || in->zone_off[0] != 0) { h->err = "offset arrays must start at 0"; return LTPL_ERR_INVALID_ARG; }
    lo->n_veh = in->veh_off[n]; lo->n_zone = in->zone_off[n];
    if (lo->n_veh < 0 || lo->n_zone < 0) { h->err = "negative offsets"; return LTPL_ERR_INVALID_ARG; }
    if (in->pos_off[0] != 0) { h->err = "pos_off must start at 0"; return LTPL_ERR_INVALID_ARG; }
    lo->n_pos = in->pos_off[lo->n_veh];
    for (int s = 0; s < n; ++s) {
        const int sl = in->start_layer[s];
        if (sl < 0 || sl >= h->lat.L) { h->err = "start_layer out of range"; return LTPL_ERR_INVALID_ARG; }
        if (h->rng_end_host[(size_t)sl] < 0) { h->err = "start layer without a planning range (end of an open track)"; return LTPL_ERR_INVALID_ARG; }
        const int nv = in->veh_off[s + 1] - in->veh_off[s];
        if (nv < 0 || nv > MAX_VEH) { h->err = "more than 96 vehicles in one scenario"; return LTPL_ERR_CAPACITY; }
        const int np = in->pos_off[in->veh_off[s + 1]] - in->pos_off[in->veh_off[s]];
        if (np < 0 || np > MAX_POS) { h->err = "more than 192 obstacle positions in one scenario"; return LTPL_ERR_CAPACITY; }
        if (in->n_last[s] < 0 || in->n_last[s] > LTPL_MAX_LAST_NODES) { h->err = "n_last out of range"; return LTPL_ERR_INVALID_ARG; }
        for (int v = in->veh_off[s]; v < in->veh_off[s + 1]; ++v)
            if (in->pos_off[v + 1] - in->pos_off[v] < 1) { h->err = "vehicle without position"; return LTPL_ERR_INVALID_ARG; }
    }
    for (int i = 0; i < lo->n_zone; ++i)
        if (in->zone_gid[i] < 0 || in->zone_gid[i] >= h->lat.V) { h->err = "zone node id out of range"; return LTPL_ERR_INVALID_ARG; }
    Arena a;
    lo->w_last = a.add(sizeof(double) * (size_t)(in->n_w_last + 1));
    lo->start_layer = a.add(sizeof(int) * (size_t)n); lo->start_node = a.add(sizeof(int) * (size_t)n);
    lo->flags = a.add(sizeof(int) * (size_t)n); lo->last_action = a.add(sizeof(int) * (size_t)n);
    lo->const_closest = a.add(sizeof(int) * (size_t)n); lo->psi_s = a.add(sizeof(double) * (size_t)n);
    lo->veh_off = a.add(sizeof(int) * (size_t)(n + 1)); lo->pos_off = a.add(sizeof(int) * (size_t)(lo->n_veh + 1));
    lo->veh_radius = a.add(sizeof(double) * (size_t)(lo->n_veh + 1));
    lo->pos_x = a.add(sizeof(double) * (size_t)(lo->n_pos + 1)); lo->pos_y = a.add(sizeof(double) * (size_t)(lo->n_pos + 1));
    lo->zone_off = a.add(sizeof(int) * (size_t)(n + 1)); lo->zone_gid = a.add(sizeof(int) * (size_t)(lo->n_zone + 1));
    lo->n_last = a.add(sizeof(int) * (size_t)n);
    lo->last_layer = a.add(sizeof(int) * (size_t)n * LTPL_MAX_LAST_NODES);
    lo->last_node = a.add(sizeof(int) * (size_t)n * LTPL_MAX_LAST_NODES);
    lo->order = a.add(sizeof(int) * (size_t)n);
    lo->total = a.size;
    return LTPL_OK;
}

#ifndef LTPL_SCEN_ORDER_MIN_SCEN
#define LTPL_SCEN_ORDER_MIN_SCEN 2048       // batches from this size on plan their scenarios in the order of their start layers (DevPathsIn::order)
#endif
static void pack_in(const ltpl_paths_in* in, const InLayout& lo, unsigned char* hb, const unsigned char* db, DevPathsIn* di, bool scen_order = true)
{
    const int n = in->n_scen;
#define CP(field, src, count, T) do { if ((count) > 0) memcpy(hb + lo.field, src, sizeof(T) * (size_t)(count)); } while (0)
    CP(w_last, in->w_last_edges, in->n_w_last, double);
    CP(start_layer, in->start_layer, n, int); CP(start_node, in->start_node, n, int); CP(flags, in->flags, n, int);
    CP(last_action, in->last_action, n, int); CP(const_closest, in->const_closest, n, int); CP(psi_s, in->psi_s, n, double);
    CP(veh_off, in->veh_off, n + 1, int); CP(pos_off, in->pos_off, lo.n_veh + 1, int);
    CP(veh_radius, in->veh_radius, lo.n_veh, double); CP(pos_x, in->pos_x, lo.n_pos, double); CP(pos_y, in->pos_y, lo.n_pos, double);
    CP(zone_off, in->zone_off, n + 1, int); CP(zone_gid, in->zone_gid, lo.n_zone, int);
    CP(n_last, in->n_last, n, int); CP(last_layer, in->last_layer, n * LTPL_MAX_LAST_NODES, int);
    CP(last_node, in->last_node, n * LTPL_MAX_LAST_NODES, int);
#undef CP
    di->n_scen = n; di->n_w_last = in->n_w_last;
    di->w_last = reinterpret_cast<const double*>(db + lo.w_last);
    di->start_layer = reinterpret_cast<const int*>(db + lo.start_layer);
    di->start_node = reinterpret_cast<const int*>(db + lo.start_node);
    di->flags = reinterpret_cast<const int*>(db + lo.flags);
    di->last_action = reinterpret_cast<const int*>(db + lo.last_action);
    di->const_closest = reinterpret_cast<const int*>(db + lo.const_closest);
    di->psi_s = reinterpret_cast<const double*>(db + lo.psi_s);
    di->veh_off = reinterpret_cast<const int*>(db + lo.veh_off);
    di->pos_off = reinterpret_cast<const int*>(db + lo.pos_off);
    di->veh_radius = reinterpret_cast<const double*>(db + lo.veh_radius);
    di->pos_x = reinterpret_cast<const double*>(db + lo.pos_x);
    di->pos_y = reinterpret_cast<const double*>(db + lo.pos_y);
    di->zone_off = reinterpret_cast<const int*>(db + lo.zone_off);
    di->zone_gid = reinterpret_cast<const int*>(db + lo.zone_gid);
    di->order = nullptr;
    if (n >= LTPL_SCEN_ORDER_MIN_SCEN && scen_order) {
        // counting sort of the scenarios by start layer (stable: equal layers keep the caller's order)
        int* ord = reinterpret_cast<int*>(hb + lo.order);
        int lmax = 0;
        for (int i = 0; i < n; ++i) { const int l = in->start_layer[i]; if (l > lmax) lmax = l; }
        std::vector<int> cnt((size_t)(lmax > 0 ? lmax : 0) + 2, 0);
        for (int i = 0; i < n; ++i) { const int l = in->start_layer[i]; ++cnt[(size_t)(l > 0 ? l : 0) + 1]; }
        for (size_t l = 1; l < cnt.size(); ++l) cnt[l] += cnt[l - 1];
        for (int i = 0; i < n; ++i) { const int l = in->start_layer[i]; ord[(size_t)cnt[(size_t)(l > 0 ? l : 0)]++] = i; }
        di->order = reinterpret_cast<const int*>(db + lo.order);
    }
    di->n_last = reinterpret_cast<const int*>(db + lo.n_last);
    di->last_layer = reinterpret_cast<const int*>(db + lo.last_layer);
    di->last_node = reinterpret_cast<const int*>(db + lo.last_node);
}

struct OutLayout {
    size_t end_layer, closest_obj_index, closest_obj_node, n_actions, action_id, valid, reduced, goal_layer, n_nodes,
        n_pts, n_ties, nodes, node_idx, coeff, path_param, total;
};

static void layout_out(int n, int cap_nodes, int cap_pts, OutLayout* lo)
{
    Arena a; const size_t A = LTPL_MAX_ACTIONS;
    lo->end_layer = a.add(sizeof(int) * (size_t)n); lo->closest_obj_index = a.add(sizeof(int) * (size_t)n);
    lo->closest_obj_node = a.add(sizeof(int) * (size_t)n * 2); lo->n_actions = a.add(sizeof(int) * (size_t)n);
    lo->action_id = a.add(sizeof(int) * n * A); lo->valid = a.add(sizeof(int) * n * A);
    lo->reduced = a.add(sizeof(int) * n * A); lo->goal_layer = a.add(sizeof(int) * n * A);
    lo->n_nodes = a.add(sizeof(int) * n * A); lo->n_pts = a.add(sizeof(int) * n * A); lo->n_ties = a.add(sizeof(int) * n * A);
    lo->nodes = a.add(sizeof(int) * n * A * (size_t)cap_nodes); lo->node_idx = a.add(sizeof(int) * n * A * (size_t)cap_nodes);
    lo->coeff = a.add(sizeof(double) * n * A * (size_t)cap_nodes * 8);
    lo->path_param = a.add(sizeof(double) * n * A * (size_t)cap_pts * 5);
    lo->total = a.size;
}

static void bind_out(unsigned char* db, const OutLayout& lo, int cap_nodes, int cap_pts, DevPathsOut* d)
{
    d->cap_nodes = cap_nodes; d->cap_pts = cap_pts;
    d->end_layer = reinterpret_cast<int*>(db + lo.end_layer);
    d->closest_obj_index = reinterpret_cast<int*>(db + lo.closest_obj_index);
    d->closest_obj_node = reinterpret_cast<int*>(db + lo.closest_obj_node);
    d->n_actions = reinterpret_cast<int*>(db + lo.n_actions);
    d->action_id = reinterpret_cast<int*>(db + lo.action_id); d->valid = reinterpret_cast<int*>(db + lo.valid);
    d->reduced = reinterpret_cast<int*>(db + lo.reduced); d->goal_layer = reinterpret_cast<int*>(db + lo.goal_layer);
    d->n_nodes = reinterpret_cast<int*>(db + lo.n_nodes); d->n_pts = reinterpret_cast<int*>(db + lo.n_pts);
    d->n_ties = reinterpret_cast<int*>(db + lo.n_ties); d->nodes = reinterpret_cast<int*>(db + lo.nodes);
    d->node_idx = reinterpret_cast<int*>(db + lo.node_idx); d->coeff = reinterpret_cast<double*>(db + lo.coeff);
    d->path_param = reinterpret_cast<double*>(db + lo.path_param);
    d->vke = nullptr; d->vxy = nullptr; d->job_cnt = nullptr; d->job_slot = nullptr; d->n_slots_pad = 0;
    d->done.host_flag = nullptr; d->done.dev_count = nullptr; d->done.seq = 0u;
}

static void scatter_out(const unsigned char* hb, const OutLayout& lo, int n, ltpl_paths_out* out)
{
    const size_t A = LTPL_MAX_ACTIONS, cn = (size_t)out->cap_nodes, cp = (size_t)out->cap_pts;
    memcpy(out->end_layer, hb + lo.end_layer, sizeof(int) * (size_t)n);
    memcpy(out->closest_obj_index, hb + lo.closest_obj_index, sizeof(int) * (size_t)n);
    memcpy(out->closest_obj_node, hb + lo.closest_obj_node, sizeof(int) * (size_t)n * 2);
    memcpy(out->n_actions, hb + lo.n_actions, sizeof(int) * (size_t)n);
    memcpy(out->action_id, hb + lo.action_id, sizeof(int) * n * A);
    memcpy(out->valid, hb + lo.valid, sizeof(int) * n * A);
    memcpy(out->reduced, hb + lo.reduced, sizeof(int) * n * A);
    memcpy(out->goal_layer, hb + lo.goal_layer, sizeof(int) * n * A);
    memcpy(out->n_nodes, hb + lo.n_nodes, sizeof(int) * n * A);
    memcpy(out->n_pts, hb + lo.n_pts, sizeof(int) * n * A);
    memcpy(out->n_ties, hb + lo.n_ties, sizeof(int) * n * A);
    memcpy(out->nodes, hb + lo.nodes, sizeof(int) * n * A * cn);
    memcpy(out->node_idx, hb + lo.node_idx, sizeof(int) * n * A * cn);
    memcpy(out->coeff, hb + lo.coeff, sizeof(double) * n * A * cn * 8);
    memcpy(out->path_param, hb + lo.path_param, sizeof(double) * n * A * cp * 5);
}

// testing only (LTPL_SCRATCH_POISON=<hex word>): fills the private-segment arena of the stream with a pattern before the
// path kernel runs, so that a reload of a register spill slot the lane never stored shows up as a parity failure
#ifdef LTPL_EXPERIMENT
__global__ __launch_bounds__(64) void k_scratch_poison(unsigned pattern, unsigned* sink)
{
    volatile unsigned a[256];
    for (int i = 0; i < 256; ++i) a[i] = pattern;
    unsigned acc = 0;
    for (int i = 0; i < 256; i += 37) acc += a[i];
    if (acc == 0x12345u && sink) *sink = acc;
}
#endif

static void scratch_poison(ltpl_handle* h)
{
#ifdef LTPL_EXPERIMENT
    if (h->scratch_poison_on)
        hipLaunchKernelGGL(k_scratch_poison, dim3(256 * 64), dim3(64), 0, h->stream, h->scratch_poison_word, (unsigned*)nullptr);
#else
    (void)h;
#endif
}

// completion of a small zero-copy call. The polled word is written by the kernel's last block (signal_done); a launch that
// never signals (fault) is picked up by the stream synchronisation the wait falls back to after 20 ms.
static DoneSignal next_done_signal(ltpl_handle* h)
{
    DoneSignal d; d.host_flag = h->h_flag; d.dev_count = h->d_done_cnt; d.seq = ++h->done_seq;
    if (d.seq == 0u) d.seq = ++h->done_seq;                    // 0 is the initial value of the word
    return d;
}
static int wait_done(ltpl_handle* h, unsigned seq)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 1;; ++spins) {
        if (__atomic_load_n(h->h_flag, __ATOMIC_ACQUIRE) == seq) break;
        if ((spins & 0x3fffu) == 0u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) {
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            if (__atomic_load_n(h->h_flag, __ATOMIC_ACQUIRE) != seq) { h->err = "kernel finished without its completion signal"; return LTPL_ERR_HIP; }
            break;
        }
    }
    if (h->poll_query) (void)hipStreamQuery(h->stream);       // non-blocking: lets the runtime retire the launch's bookkeeping
    // let the runtime retire its bookkeeping of the launches now and then (LTPL_POLL_SYNC_EVERY calls, 0 = never)
    if (h->poll_sync_every > 0 && (++h->polled_calls % (unsigned)h->poll_sync_every) == 0u) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return LTPL_OK;
}

static int plan_paths_impl(ltpl_handle* h, const ltpl_paths_in* in, ltpl_paths_out* out, int force_nw, uint8_t* blocked = nullptr);

extern "C" int ltpl_plan_paths(ltpl_handle* h, const ltpl_paths_in* in, ltpl_paths_out* out)
try {
    return plan_paths_impl(h, in, out, 0);
} LTPL_ABI_CATCH(abi_err_of(h))

extern "C" int ltpl_plan_paths_mask(ltpl_handle* h, const ltpl_paths_in* in, ltpl_paths_out* out, int32_t team_waves, uint8_t* blocked)
try {
    if (!h) return LTPL_ERR_INVALID_ARG;
    if (!blocked || !(team_waves == 0 || team_waves == 1 || team_waves == NUM_WAVES)) { h->err = "ltpl_plan_paths_mask: bad argument"; return LTPL_ERR_INVALID_ARG; }
    return plan_paths_impl(h, in, out, team_waves, blocked);
} LTPL_ABI_CATCH(abi_err_of(h))

// force_nw: 0 = choose by batch size, 1 / NUM_WAVES = one-wave batch kernel / four-wave latency kernel (self-test, diagnostics);
// blocked: [n_scen * E] bytes or nullptr -- the obstacle x edge mask as the kernel computed it (ltpl_plan_paths_mask)
static int plan_paths_impl(ltpl_handle* h, const ltpl_paths_in* in, ltpl_paths_out* out, int force_nw, uint8_t* blocked)
{
    if (!h) return LTPL_ERR_INVALID_ARG;
    if (!out) { h->err = "null output"; return LTPL_ERR_INVALID_ARG; }
    LTPL_PROF(prof_pack, "plan_paths.validate+pack");
    HIP_TRY(h, hipSetDevice(h->device));
    drop_resident(h);
    InLayout li;
    int rc = validate_and_layout(h, in, &li);
    if (rc) return rc;
    if (out->cap_nodes < h->caps.max_path_nodes || out->cap_pts < h->caps.max_path_pts) {
        h->err = "output capacity below ltpl_caps.max_path_nodes / max_path_pts"; return LTPL_ERR_CAPACITY;
    }
    OutLayout lo;
    layout_out(in->n_scen, out->cap_nodes, out->cap_pts, &lo);
    if ((rc = ensure(h, &h->h_in, &h->h_in_cap, &h->d_in, &h->d_in_cap, li.total))) return rc;
    if ((rc = ensure(h, &h->h_out, &h->h_out_cap, &h->d_out, &h->d_out_cap, lo.total))) return rc;
    DevPathsIn di; DevPathsOut dout;
    const bool zci = h->zc_in && in->n_scen <= 8;
    pack_in(in, li, static_cast<unsigned char*>(h->h_in), static_cast<const unsigned char*>(zci ? h->h_in : h->d_in), &di, h->scen_order != 0);
    // small calls (latency path): the output slab is the page-locked host buffer itself (device-accessible under unified
    // addressing): the kernel's stores cross PCIe as posted writes, no D2H copy is enqueued
    const bool zc = h->zc_out && in->n_scen <= 8;
    bind_out(static_cast<unsigned char*>(zc ? h->h_out : h->d_out), lo, out->cap_nodes, out->cap_pts, &dout);
    const int nw = force_nw ? force_nw : ((in->n_scen >= h->nw1_min_scen && h->batch_nw == 1) ? 1 : NUM_WAVES);
    const bool polled = zc && h->poll && !h->d_dbg && nw != 1;      // (the one-wave batch form carries no completion word)
    if (polled) dout.done = next_done_signal(h);
    prof_pack.stop();
    LTPL_PROF(prof_enq, "plan_paths.enqueue");
    {
        LTPL_PROF(prof_h2d, "plan_paths.enqueue.h2d");
        if (!zci) HIP_TRY(h, hipMemcpyAsync(h->d_in, h->h_in, li.total, hipMemcpyHostToDevice, h->stream));
    }
    scratch_poison(h);
    unsigned* d_mask = nullptr;
    const size_t mask_words = (size_t)((nw == 1 ? h->lp1 : h->lp4).words_blocked + 2);
    struct MaskGuard { unsigned* p = nullptr; ~MaskGuard() { if (p) (void)hipFree(p); } } mask_guard;
    if (blocked) {
        HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&d_mask), sizeof(unsigned) * mask_words * (size_t)in->n_scen));
        mask_guard.p = d_mask;
    }
    {
        LTPL_PROF(prof_l, "plan_paths.enqueue.launch");
        if ((rc = launch_paths(h, nw, in->n_scen, h->stream, di, dout, d_mask))) return rc;
    }
    if (!zc) HIP_TRY(h, hipMemcpyAsync(h->h_out, h->d_out, lo.total, hipMemcpyDeviceToHost, h->stream));
    prof_enq.stop();
    LTPL_PROF(prof_sync, "plan_paths.sync");
    if (polled) { if ((rc = wait_done(h, dout.done.seq))) return rc; }
    else HIP_TRY(h, hipStreamSynchronize(h->stream));
    prof_sync.stop();
    dbg_report(h, "k_paths", in->n_scen);
    if (blocked) {
        // per scenario: first edge of the planning range, its layer count, one bit per edge of the range in edge-id order (wraps at E)
        std::vector<unsigned> hm(mask_words * (size_t)in->n_scen);
        HIP_TRY(h, hipMemcpy(hm.data(), d_mask, sizeof(unsigned) * hm.size(), hipMemcpyDeviceToHost));
        const size_t E = (size_t)h->lat.E;
        memset(blocked, 0, E * (size_t)in->n_scen);
        for (int s = 0; s < in->n_scen; ++s) {
            const unsigned* w = hm.data() + mask_words * (size_t)s;
            const size_t e_base = w[0];
            for (size_t i = 0; i < (mask_words - 2) * 32 && i < E; ++i)
                if ((w[2 + (i >> 5)] >> (i & 31)) & 1u) blocked[(size_t)s * E + (size_t)h->sw2csc_host[(e_base + i) % E]] = 1;   // bitmap in sweep order
        }
    }
    LTPL_PROF(prof_sc, "plan_paths.scatter");
    scatter_out(static_cast<const unsigned char*>(h->h_out), lo, in->n_scen, out);
    return LTPL_OK;
}

extern "C" int ltpl_process_objects(ltpl_handle* h, const ltpl_objects_in* in, ltpl_objects_out* out)
try {
    if (!h) return LTPL_ERR_INVALID_ARG;
    if (!in || !out || in->n_obj < 1 || !in->x || !in->y || !in->theta || !in->v || !in->length ||
        !out->on_track || !out->pred_x || !out->pred_y || !out->radius) { h->err = "null argument or n_obj < 1"; return LTPL_ERR_INVALID_ARG; }
    if (!h->lat.ctx) { h->err = "the lattice was created without track bounds (normvec / width_right / width_left)"; return LTPL_ERR_UNSUPPORTED; }
    HIP_TRY(h, hipSetDevice(h->device));
    drop_resident(h);
    const size_t n = (size_t)in->n_obj;
    Arena ain, aout;
    const size_t o_x = ain.add(8 * n), o_y = ain.add(8 * n), o_t = ain.add(8 * n), o_v = ain.add(8 * n), o_l = ain.add(8 * n);
    const size_t o_px = aout.add(8 * n), o_py = aout.add(8 * n), o_r = aout.add(8 * n), o_on = aout.add(4 * n);
    int rc;
    if ((rc = ensure(h, &h->h_in, &h->h_in_cap, &h->d_in, &h->d_in_cap, ain.size))) return rc;
    if ((rc = ensure(h, &h->h_out, &h->h_out_cap, &h->d_out, &h->d_out_cap, aout.size))) return rc;
    unsigned char* hb = static_cast<unsigned char*>(h->h_in); unsigned char* db = static_cast<unsigned char*>(h->d_in);
    unsigned char* dob = static_cast<unsigned char*>(h->d_out);
    memcpy(hb + o_x, in->x, 8 * n); memcpy(hb + o_y, in->y, 8 * n); memcpy(hb + o_t, in->theta, 8 * n);
    memcpy(hb + o_v, in->v, 8 * n); memcpy(hb + o_l, in->length, 8 * n);
    HIP_TRY(h, hipMemcpyAsync(h->d_in, h->h_in, ain.size, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_process_objects, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, h->lat, in->n_obj, in->dt,
                       reinterpret_cast<const double*>(db + o_x), reinterpret_cast<const double*>(db + o_y),
                       reinterpret_cast<const double*>(db + o_t), reinterpret_cast<const double*>(db + o_v),
                       reinterpret_cast<const double*>(db + o_l), reinterpret_cast<int*>(dob + o_on),
                       reinterpret_cast<double*>(dob + o_px), reinterpret_cast<double*>(dob + o_py), reinterpret_cast<double*>(dob + o_r));
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(h->h_out, h->d_out, aout.size, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const unsigned char* ho = static_cast<const unsigned char*>(h->h_out);
    memcpy(out->pred_x, ho + o_px, 8 * n); memcpy(out->pred_y, ho + o_py, 8 * n); memcpy(out->radius, ho + o_r, 8 * n);
    memcpy(out->on_track, ho + o_on, 4 * n);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(h))

// --- velocity seam / fused tick ---------------------------------------------------------------------------------------
// kernel variant = (exponent mode, single-row machine table): compile-time specialisations of the recurrences
static int vel_variant(const ltpl_vel_params* vp)
{
    const int em = vp->dyn_model_exp == 1.0 ? 1 : (vp->dyn_model_exp == 2.0 ? 2 : 0);
    return em * 2 + (vp->n_ax_max_machines == 1 ? 1 : 0);
}
typedef void (*vel_kernel_t)(DevLat, DevVelParams, const DevVelJob*, const double*, double*, int*, int, long long*, DoneSignal, int);
typedef void (*tick_kernel_t)(DevLat, DevPathsIn, DevPathsOut, TeamLds, DevVelParams, DevTickVelIn, DevTickVelOut, int, int, int);
typedef void (*lanes_kernel_t)(DevLat, DevPathsIn, DevPathsOut, DevVelParams, DevTickVelIn, DevVelPrep, VelPlanes, int, int, int, long long*, DevTickVelOut, int);
#ifndef LTPL_EMIT_MIN_SCEN
#define LTPL_EMIT_MIN_SCEN 256        // launches with at least this many scenarios write the generic jobs' vx / ax from the lane kernel (k_vel_lanes)
#endif
// (one line per kernel family; the six (EM, AXM1) cases: with_vel_variant, vel_layout.hpp)
static lanes_kernel_t lanes_kernel_of(int v) { return with_vel_variant(v, [](auto em, auto axm1) -> lanes_kernel_t { return k_vel_lanes<em.value, axm1.value>; }); }
static vel_kernel_t vel_kernel_of(int v) { return with_vel_variant(v, [](auto em, auto axm1) -> vel_kernel_t { return k_vel_profile<em.value, axm1.value>; }); }
template <int SEL>
static vel_kernel_t vel_kernel_const_of(int v)          // constant friction limits per job (fleet); SEL: see k_vel_profile
{
    return with_vel_variant(v, [](auto em, auto axm1) -> vel_kernel_t { return k_vel_profile<em.value, axm1.value, false, SEL>; });
}
template <int SEL>
static vel_kernel_t vel_kernel_rows_of(int v)           // friction limits as rows per job (fleet, local_gg as a dict): the interpolating machine-table form only
{
    return with_vel_variant(v, [](auto em, auto) -> vel_kernel_t { return k_vel_profile<em.value, false, true, SEL>; });
}
static tick_kernel_t tick_kernel_of(int v, bool plan_a = false)
{
    if (plan_a) return with_vel_variant(v, [](auto em, auto axm1) -> tick_kernel_t { return k_tick<em.value, axm1.value, PlanA4>; });
    return with_vel_variant(v, [](auto em, auto axm1) -> tick_kernel_t { return k_tick<em.value, axm1.value, PlanRt>; });
}

static int make_vel_params(ltpl_handle* h, const ltpl_vel_params* vp, const double* d_axm, DevVelParams* p)
{
    if (!vp || vp->n_ax_max_machines < 1 || !vp->ax_max_machines) { h->err = "ax_max_machines missing"; return LTPL_ERR_INVALID_ARG; }
    if (vp->n_ax_max_machines > 64) { h->err = "ax_max_machines with more than 64 rows"; return LTPL_ERR_CAPACITY; }
    if (!(vp->dyn_model_exp > 0.0) || !(vp->m_veh > 0.0)) { h->err = "invalid vehicle parameters"; return LTPL_ERR_INVALID_ARG; }
    p->e = vp->dyn_model_exp; p->inv_e = 1.0 / vp->dyn_model_exp; p->drag_m = vp->drag_coeff / vp->m_veh;
    p->len_veh = vp->len_veh; p->v_max = vp->v_max; p->n_axm = vp->n_ax_max_machines; p->ctrl = vp->follow_control_type;
    p->axm = d_axm; p->c_p = vp->c_p; p->k_p = vp->k_p; p->k_d = vp->k_d; p->tan_w = vp->tan_w;
    return LTPL_OK;
}

extern "C" int ltpl_vel_profile(ltpl_handle* h, const ltpl_vel_params* vp, int n_jobs, const ltpl_vel_job* jobs,
                                ltpl_vel_result* results)
try {
    if (!h) return LTPL_ERR_INVALID_ARG;
    if (n_jobs < 1 || !jobs || !results) { h->err = "no jobs"; return LTPL_ERR_INVALID_ARG; }
    LTPL_PROF(prof_pack, "vel_profile.validate+pack");
    HIP_TRY(h, hipSetDevice(h->device));
    drop_resident(h);
    // pooled layout: [axm table][jobs][kappa | el | gg per job] ; outputs: [flags][vx per job]
    Arena ain, aout;
    const size_t o_axm = ain.add(sizeof(double) * 2 * (size_t)(vp ? vp->n_ax_max_machines : 1));
    const size_t o_jobs = ain.add(sizeof(DevVelJob) * (size_t)n_jobs);
    const size_t o_pool = ain.add(0);
    size_t pool_doubles = 0, out_doubles = 0; int cap = 0;
    std::vector<DevVelJob> dj((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const ltpl_vel_job& jb = jobs[j];
        if (jb.n < 1 || !jb.kappa || !jb.loc_gg || !results[j].vx) { h->err = "job without data"; return LTPL_ERR_INVALID_ARG; }
        if (jb.mode == LTPL_VEL_FOLLOW || jb.mode == LTPL_VEL_FOLLOW_CONTROLLED) { if (jb.n_el < jb.n) { h->err = "follow: el_lengths shorter than kappa"; return LTPL_ERR_INVALID_ARG; } }
        else if (jb.mode == LTPL_VEL_FB || jb.mode == LTPL_VEL_BRAKE) {
            if (jb.n_el != jb.n - 1) { h->err = "kappa must have the length of el_lengths + 1"; return LTPL_ERR_INVALID_ARG; }
        } else { h->err = "unknown velocity mode"; return LTPL_ERR_INVALID_ARG; }
        DevVelJob& d = dj[(size_t)j];
        d.mode = jb.mode; d.n = jb.n; d.n_el = jb.n_el; d.has_v_end = jb.has_v_end;
        d.off_kappa = (int)pool_doubles; pool_doubles += (size_t)jb.n;
        d.off_el = (int)pool_doubles; pool_doubles += (size_t)jb.n_el;
        d.off_gg = (int)pool_doubles; pool_doubles += 2 * (size_t)jb.n;
        d.off_out = (int)out_doubles; out_doubles += (size_t)jb.n;
        d.v_start = jb.v_start; d.v_end = jb.v_end; d.v_ego = jb.v_ego; d.v_obj = jb.v_obj; d.safety_d = jb.safety_d;
        d.obj_dist = jb.obj_dist; d.obj_x = jb.obj_x; d.obj_y = jb.obj_y;
        const int need = jb.n_el > jb.n ? jb.n_el : jb.n;
        if (need > cap) cap = need;
    }
    ain.add(sizeof(double) * pool_doubles);
    const size_t o_flags = aout.add(sizeof(int) * 2 * (size_t)n_jobs);
    const size_t o_vx = aout.add(sizeof(double) * out_doubles);
    const size_t lds = vel_scratch_bytes(cap, true, false);
    if (lds > 150 * 1024) { h->err = "velocity profile too long for the LDS-resident solver"; return LTPL_ERR_CAPACITY; }
    int rc;
    if ((rc = ensure(h, &h->h_in, &h->h_in_cap, &h->d_in, &h->d_in_cap, ain.size))) return rc;
    if ((rc = ensure(h, &h->h_out, &h->h_out_cap, &h->d_out, &h->d_out_cap, aout.size))) return rc;
    unsigned char* hb = static_cast<unsigned char*>(h->h_in);
    const bool zci = h->zc_in && n_jobs <= 16;
    unsigned char* db = static_cast<unsigned char*>(zci ? h->h_in : h->d_in);
    DevVelParams p;
    if ((rc = make_vel_params(h, vp, reinterpret_cast<const double*>(db + o_axm), &p))) return rc;
    memcpy(hb + o_axm, vp->ax_max_machines, sizeof(double) * 2 * (size_t)vp->n_ax_max_machines);
    memcpy(hb + o_jobs, dj.data(), sizeof(DevVelJob) * (size_t)n_jobs);
    double* pool = reinterpret_cast<double*>(hb + o_pool);
    for (int j = 0; j < n_jobs; ++j) {
        const ltpl_vel_job& jb = jobs[j]; const DevVelJob& d = dj[(size_t)j];
        memcpy(pool + d.off_kappa, jb.kappa, sizeof(double) * (size_t)jb.n);
        if (jb.n_el > 0) memcpy(pool + d.off_el, jb.el_lengths, sizeof(double) * (size_t)jb.n_el);
        memcpy(pool + d.off_gg, jb.loc_gg, sizeof(double) * 2 * (size_t)jb.n);
    }
    vel_kernel_t kern = vel_kernel_of(vel_variant(vp));
    if ((rc = raise_lds_limit(h, reinterpret_cast<const void*>(kern), lds, LDS_SLOT_VEL + vel_variant(vp)))) return rc;
    prof_pack.stop();
    LTPL_PROF(prof_enq, "vel_profile.enqueue");
    if (!zci) HIP_TRY(h, hipMemcpyAsync(h->d_in, h->h_in, ain.size, hipMemcpyHostToDevice, h->stream));
    const bool zc = h->zc_out && n_jobs <= 16;
    unsigned char* dob = static_cast<unsigned char*>(zc ? h->h_out : h->d_out);
    const bool polled = zc && h->poll && !h->d_dbg;
    DoneSignal done; done.host_flag = nullptr; done.dev_count = nullptr; done.seq = 0u;
    if (polled) done = next_done_signal(h);
    hipLaunchKernelGGL(kern, dim3(n_jobs), dim3(64), lds, h->stream, h->lat, p,
                       reinterpret_cast<const DevVelJob*>(db + o_jobs), reinterpret_cast<const double*>(db + o_pool),
                       reinterpret_cast<double*>(dob + o_vx), reinterpret_cast<int*>(dob + o_flags), cap, h->lp4.dbg, done, 1);
    HIP_TRY(h, hipGetLastError());
    if (!zc) HIP_TRY(h, hipMemcpyAsync(h->h_out, h->d_out, aout.size, hipMemcpyDeviceToHost, h->stream));
    prof_enq.stop();
    LTPL_PROF(prof_sync, "vel_profile.sync");
    if (polled) { if ((rc = wait_done(h, done.seq))) return rc; }
    else HIP_TRY(h, hipStreamSynchronize(h->stream));
    prof_sync.stop();
    dbg_report(h, "k_vel_profile", n_jobs);
    LTPL_PROF(prof_sc, "vel_profile.scatter");
    const unsigned char* ho = static_cast<const unsigned char*>(h->h_out);
    const int* flags = reinterpret_cast<const int*>(ho + o_flags);
    const double* vx = reinterpret_cast<const double*>(ho + o_vx);
    for (int j = 0; j < n_jobs; ++j) {
        memcpy(results[j].vx, vx + dj[(size_t)j].off_out, sizeof(double) * (size_t)jobs[j].n);
        results[j].too_close = flags[2 * j]; results[j].vel_bound = flags[2 * j + 1];
    }
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(h))

#include "tick_host.hpp"

// ---------------------------------------------------------------------------------------------------------------------
// offline lattice build: every candidate edge of a track in one launch, lane = edge
// ---------------------------------------------------------------------------------------------------------------------
struct DevOfflineIn {
    int n_edges, cap; double step, kmax_turn;
    const double* sx; const double* sy; const double* spsi; const double* ex; const double* ey; const double* epsi;
    const double* kmax_vel; const int* rl_edge; const double* given;
};
struct DevOfflineOut { int* n_samples; int* valid; double* coeff; double* length; double* kavg; double* krange; double* samples; };

__global__ __launch_bounds__(64) void k_offline_edges(DevOfflineIn in, DevOfflineOut out)
{
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= in.n_edges) return;
    double cx[4], cy[4];
    if (in.rl_edge[e]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { cx[k] = in.given[(size_t)e * 8 + k]; cy[k] = in.given[(size_t)e * 8 + 4 + k]; }
    } else {
        // tph.calc_splines on two points with heading constraints (gen_edges.py:80-84): cubic Hermite segment, end slopes scaled
        // by the chord length (psi = 0 is north, hence + pi / 2)
        const double x0 = in.sx[e], y0 = in.sy[e], x1 = in.ex[e], y1 = in.ey[e];
        const double el = sqrt((x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0));
        const double tx0 = cos(in.spsi[e] + D_PI / 2) * el, ty0 = sin(in.spsi[e] + D_PI / 2) * el;
        const double tx1 = cos(in.epsi[e] + D_PI / 2) * el, ty1 = sin(in.epsi[e] + D_PI / 2) * el;
        cx[0] = x0; cx[1] = tx0; cx[2] = 3.0 * (x1 - x0) - 2.0 * tx0 - tx1; cx[3] = -2.0 * (x1 - x0) + tx0 + tx1;
        cy[0] = y0; cy[1] = ty0; cy[2] = 3.0 * (y1 - y0) - 2.0 * ty0 - ty1; cy[3] = -2.0 * (y1 - y0) + ty0 + ty1;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { out.coeff[(size_t)e * 8 + k] = cx[k]; out.coeff[(size_t)e * 8 + 4 + k] = cy[k]; }
    auto px = [&](double t) { return cx[0] + cx[1] * t + cx[2] * (t * t) + cx[3] * (t * t * t); };
    auto py = [&](double t) { return cy[0] + cy[1] * t + cy[2] * (t * t) + cy[3] * (t * t * t); };
    // tph.calc_spline_lengths: polyline over 15 uniform-t points
    double len = 0.0;
    {
        double lx = px(0.0), ly = py(0.0);
        for (int i = 1; i < 15; ++i) {
            const double t = i == 14 ? 1.0 : (double)i * (1.0 / 14.0);
            const double qx = px(t), qy = py(t);
            len += sqrt((qx - lx) * (qx - lx) + (qy - ly) * (qy - ly));
            lx = qx; ly = qy;
        }
    }
    const int n = (int)ceil(len / in.step) + 1;                  // tph.interp_splines(stepsize_approx, incl_last_point=True)
    out.n_samples[e] = n;
    if (n > in.cap || n < 2) { out.valid[e] = 0; out.length[e] = 0.0; out.kavg[e] = 0.0; out.krange[e] = 0.0; return; }
    double* S = out.samples + (size_t)e * in.cap * 5;
    const double lin_step = len / (double)(n - 1);
    const double kmax_v = in.kmax_vel[e], kmax_t = in.kmax_turn;
    bool ok = true; double sum_abs = 0.0, kmin = INFINITY, kmax = -INFINITY, slen = 0.0, lx = 0.0, ly = 0.0;
    for (int i = 0; i < n; ++i) {
        const bool last = i == n - 1;
        const double t = last ? 1.0 : ((double)i * lin_step) / len;
        double x = px(t), y = py(t);
        if (last) { x = ((cx[0] + cx[1]) + cx[2]) + cx[3]; y = ((cy[0] + cy[1]) + cy[2]) + cy[3]; }
        const double xd = cx[1] + 2.0 * cx[2] * t + 3.0 * cx[3] * (t * t), yd = cy[1] + 2.0 * cy[2] * t + 3.0 * cy[3] * (t * t);
        const double xdd = 2.0 * cx[2] + 6.0 * cx[3] * t, ydd = 2.0 * cy[2] + 6.0 * cy[3] * t;
        const double psi = normalize_psi_dev(atan2(yd, xd) - D_PI / 2);
        const double q = xd * xd + yd * yd;
        const double kap = (xd * ydd - yd * xdd) / (q * sqrt(q));
        double* r = S + (size_t)i * 5;
        r[0] = x; r[1] = y; r[2] = psi; r[3] = kap; r[4] = 0.0;
        if (i > 0) { const double el = sqrt((x - lx) * (x - lx) + (y - ly) * (y - ly)); S[(size_t)(i - 1) * 5 + 4] = el; slen += el; }
        lx = x; ly = y;
        const double ka = fabs(kap);
        ok = ok && ka <= kmax_t && ka <= kmax_v;
        sum_abs += ka; kmin = kap < kmin ? kap : kmin; kmax = kap > kmax ? kap : kmax;
    }
    out.valid[e] = (ok || in.rl_edge[e]) ? 1 : 0;
    out.length[e] = slen; out.kavg[e] = sum_abs / (double)n; out.krange[e] = fabs(kmax - kmin);
}

extern "C" int ltpl_offline_edges(int device, const ltpl_offline_edges_in* in, ltpl_offline_edges_out* out)
try {
    g_create_error.clear();
    if (!in || !out || in->n_edges < 1 || in->cap_samples < 2 || !(in->stepsize_approx > 0.0)) { g_create_error = "offline edges: invalid argument"; return LTPL_ERR_INVALID_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_create_error = "no HIP device visible"; return LTPL_ERR_NO_DEVICE; }
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    if (device >= ndev || hipSetDevice(device) != hipSuccess) { g_create_error = "device index out of range"; return LTPL_ERR_NO_DEVICE; }
    const size_t n = (size_t)in->n_edges, cap = (size_t)in->cap_samples;
    Arena ai, ao;
    const size_t o_sx = ai.add(8 * n), o_sy = ai.add(8 * n), o_sp = ai.add(8 * n), o_ex = ai.add(8 * n), o_ey = ai.add(8 * n), o_ep = ai.add(8 * n),
                 o_kv = ai.add(8 * n), o_rl = ai.add(4 * n), o_gc = ai.add(64 * n);
    const size_t q_ns = ao.add(4 * n), q_va = ao.add(4 * n), q_co = ao.add(64 * n), q_le = ao.add(8 * n), q_ka = ao.add(8 * n), q_kr = ao.add(8 * n),
                 q_sa = ao.add(8 * 5 * cap * n);
    unsigned char *di = nullptr, *dobuf = nullptr;
    auto fail = [&](const char* why) { g_create_error = why; if (di) (void)hipFree(di); if (dobuf) (void)hipFree(dobuf); return LTPL_ERR_HIP; };
    if (hipMalloc(reinterpret_cast<void**>(&di), ai.size) != hipSuccess) return fail("offline edges: hipMalloc failed");
    if (hipMalloc(reinterpret_cast<void**>(&dobuf), ao.size) != hipSuccess) return fail("offline edges: hipMalloc failed");
    auto up = [&](size_t off, const void* src, size_t bytes) { return hipMemcpy(di + off, src, bytes, hipMemcpyHostToDevice) == hipSuccess; };
    if (!up(o_sx, in->start_x, 8 * n) || !up(o_sy, in->start_y, 8 * n) || !up(o_sp, in->start_psi, 8 * n) || !up(o_ex, in->end_x, 8 * n) ||
        !up(o_ey, in->end_y, 8 * n) || !up(o_ep, in->end_psi, 8 * n) || !up(o_kv, in->kappa_max_vel, 8 * n) || !up(o_rl, in->raceline_edge, 4 * n) ||
        !up(o_gc, in->given_coeff, 64 * n)) return fail("offline edges: upload failed");
    DevOfflineIn d; d.n_edges = in->n_edges; d.cap = in->cap_samples; d.step = in->stepsize_approx; d.kmax_turn = in->kappa_max_turn;
    d.sx = reinterpret_cast<double*>(di + o_sx); d.sy = reinterpret_cast<double*>(di + o_sy); d.spsi = reinterpret_cast<double*>(di + o_sp);
    d.ex = reinterpret_cast<double*>(di + o_ex); d.ey = reinterpret_cast<double*>(di + o_ey); d.epsi = reinterpret_cast<double*>(di + o_ep);
    d.kmax_vel = reinterpret_cast<double*>(di + o_kv); d.rl_edge = reinterpret_cast<int*>(di + o_rl); d.given = reinterpret_cast<double*>(di + o_gc);
    DevOfflineOut o; o.n_samples = reinterpret_cast<int*>(dobuf + q_ns); o.valid = reinterpret_cast<int*>(dobuf + q_va);
    o.coeff = reinterpret_cast<double*>(dobuf + q_co); o.length = reinterpret_cast<double*>(dobuf + q_le); o.kavg = reinterpret_cast<double*>(dobuf + q_ka);
    o.krange = reinterpret_cast<double*>(dobuf + q_kr); o.samples = reinterpret_cast<double*>(dobuf + q_sa);
    hipLaunchKernelGGL(k_offline_edges, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, d, o);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail("offline edges: kernel failed");
    auto down = [&](void* dst, size_t off, size_t bytes) { return hipMemcpy(dst, dobuf + off, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
    if (!down(out->n_samples, q_ns, 4 * n) || !down(out->valid, q_va, 4 * n) || !down(out->coeff, q_co, 64 * n) || !down(out->length, q_le, 8 * n) ||
        !down(out->kappa_avg, q_ka, 8 * n) || !down(out->kappa_range, q_kr, 8 * n) || !down(out->samples, q_sa, 8 * 5 * cap * n)) return fail("offline edges: download failed");
    (void)hipFree(di); (void)hipFree(dobuf);
    return LTPL_OK;
} LTPL_ABI_CATCH(nullptr)

// ---------------------------------------------------------------------------------------------------------------------
// self-test at ltpl_create: the one-wave batch kernel and the four-wave latency kernel are two differently scheduled builds
// of the same source (different register budgets, LDS plans and synchronisation); 64 probe scenarios derived from the
// lattice itself (an obstacle on the race line four layers ahead: mask, three filters, tie-break rounds) must come out
// IDENTICAL from both, otherwise the handle is refused. Guards against a toolchain that miscompiles one of them
//  for lattices no parity test has seen. LTPL_NO_SELFTEST=1 skips it.
// ---------------------------------------------------------------------------------------------------------------------
// the cross-lane helpers of the kernels (reductions, scans, lexicographic minima: DPP row operations + v_permlane16/32_swap) against plain loops,
// on 16 waves of values with many ties -- one launch of k_exp_wave_ops at create time
static int wave_ops_selftest(ltpl_handle* h)
{
    const int rounds = 16;
    std::vector<double> vals((size_t)rounds * 128); std::vector<int> ivals((size_t)rounds * 64);
    unsigned long long x = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { x = x * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(x >> 33); };
    for (size_t i = 0; i < vals.size(); ++i) vals[i] = (double)(next() % 23u) * 0.25 - 2.0;          // few distinct values: ties in every reduction
    for (size_t i = 0; i < ivals.size(); ++i) ivals[i] = (int)(next() % 200u) - 60;
    double* dv = nullptr; int* di = nullptr; int* de = nullptr;
    struct Guard { void** p[3]; ~Guard() { for (void** q : p) if (*q) (void)hipFree(*q); } } guard{{reinterpret_cast<void**>(&dv), reinterpret_cast<void**>(&di), reinterpret_cast<void**>(&de)}};
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&dv), sizeof(double) * vals.size()));
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&di), sizeof(int) * ivals.size()));
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&de), sizeof(int)));
    HIP_TRY(h, hipMemcpy(dv, vals.data(), sizeof(double) * vals.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(di, ivals.data(), sizeof(int) * ivals.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemset(de, 0, sizeof(int)));
    hipLaunchKernelGGL(k_exp_wave_ops, dim3(1), dim3(64), 0, h->stream, dv, di, rounds, de);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int bad = 0;
    HIP_TRY(h, hipMemcpy(&bad, de, sizeof(int), hipMemcpyDeviceToHost));
    if (bad) { h->err = "self-test failed: the wave reductions / scans of the kernels disagree with plain loops on this device"; return LTPL_ERR_UNSUPPORTED; }
    return LTPL_OK;
}

static int self_test(ltpl_handle* h, const ltpl_lattice_desc* d)
{
    {
        const int rc = wave_ops_selftest(h);
        if (rc) return rc;
    }
    const int n = 64, L = d->num_layers, A = LTPL_MAX_ACTIONS;
    std::vector<int> sl(n), sn(n), flags(n, LTPL_FLAG_ACTION_SETS), la(n, LTPL_ACT_NONE), cc(n, -1), veh_off(n + 1), pos_off(n + 1),
        zone_off(n + 1, 0), zone(1, 0), n_last(n, 0), ll((size_t)n * LTPL_MAX_LAST_NODES, -1), ln((size_t)n * LTPL_MAX_LAST_NODES, -1);
    std::vector<double> psi(n, 0.0), rad(n, 2.5), px(n), py(n), w(1, 0.0);
    for (int i = 0; i < n; ++i) {
        sl[i] = (int)(((long long)i * L) / n);
        while (h->rng_end_host[(size_t)sl[i]] < 0 && sl[i] > 0) --sl[i];     // open tracks: the last layer(s) have no planning range
        sn[i] = d->raceline_index[sl[i]];
        const int ol = (sl[i] + 4) % L, g = d->layer_node_off[ol] + d->raceline_index[ol];
        px[i] = d->node_x[g]; py[i] = d->node_y[g];
        veh_off[i] = i; pos_off[i] = i;
        if (i % 4 == 3) flags[i] |= LTPL_FLAG_OBJ_BESIDES;            // constant-segment template: follow + left + right on `default`
    }
    veh_off[n] = n; pos_off[n] = n;
    ltpl_paths_in in; memset(&in, 0, sizeof(in));
    in.n_scen = n; in.n_w_last = 0; in.w_last_edges = w.data(); in.start_layer = sl.data(); in.start_node = sn.data();
    in.flags = flags.data(); in.last_action = la.data(); in.const_closest = cc.data(); in.psi_s = psi.data();
    in.veh_off = veh_off.data(); in.pos_off = pos_off.data(); in.veh_radius = rad.data(); in.pos_x = px.data(); in.pos_y = py.data();
    in.zone_off = zone_off.data(); in.zone_gid = zone.data(); in.n_last = n_last.data(); in.last_layer = ll.data(); in.last_node = ln.data();
    const int cn = h->caps.max_path_nodes, cp = h->caps.max_path_pts;
    struct Out {
        std::vector<int> end_layer, coi, con, n_actions, action_id, valid, reduced, goal_layer, n_nodes, n_pts, n_ties, nodes, node_idx;
        std::vector<double> coeff, pp; ltpl_paths_out o;
    };
    auto make = [&](Out& O) {
        O.end_layer.assign(n, 0); O.coi.assign(n, 0); O.con.assign((size_t)n * 2, 0); O.n_actions.assign(n, 0);
        for (auto* v : {&O.action_id, &O.valid, &O.reduced, &O.goal_layer, &O.n_nodes, &O.n_pts, &O.n_ties}) v->assign((size_t)n * A, 0);
        O.nodes.assign((size_t)n * A * cn, 0); O.node_idx.assign((size_t)n * A * cn, 0);
        O.coeff.assign((size_t)n * A * cn * 8, 0.0); O.pp.assign((size_t)n * A * cp * 5, 0.0);
        memset(&O.o, 0, sizeof(O.o));
        O.o.cap_nodes = cn; O.o.cap_pts = cp; O.o.end_layer = O.end_layer.data(); O.o.closest_obj_index = O.coi.data();
        O.o.closest_obj_node = O.con.data(); O.o.n_actions = O.n_actions.data(); O.o.action_id = O.action_id.data();
        O.o.valid = O.valid.data(); O.o.reduced = O.reduced.data(); O.o.goal_layer = O.goal_layer.data(); O.o.n_nodes = O.n_nodes.data();
        O.o.n_pts = O.n_pts.data(); O.o.n_ties = O.n_ties.data(); O.o.nodes = O.nodes.data(); O.o.node_idx = O.node_idx.data();
        O.o.coeff = O.coeff.data(); O.o.path_param = O.pp.data();
    };
    Out a, b; make(a); make(b);
    int rc = plan_paths_impl(h, &in, &a.o, 1);
    if (rc) return rc;
    if ((rc = plan_paths_impl(h, &in, &b.o, NUM_WAVES))) return rc;
    bool same = a.n_actions == b.n_actions && a.action_id == b.action_id && a.valid == b.valid && a.reduced == b.reduced &&
                a.n_nodes == b.n_nodes && a.n_pts == b.n_pts && a.n_ties == b.n_ties && a.coi == b.coi;
    int n_paths = 0;
    for (size_t slot = 0; same && slot < (size_t)n * A; ++slot) {
        if (!a.valid[slot]) continue;
        ++n_paths;
        for (int i = 0; i < a.n_nodes[slot]; ++i) same = same && a.nodes[slot * cn + i] == b.nodes[slot * cn + i];
    }
    if (!same) { h->err = "self-test failed: the one-wave batch kernel and the four-wave kernel disagree on the probe scenarios"; return LTPL_ERR_HIP; }
    if (n_paths == 0) { h->err = "self-test failed: no path found on any probe scenario"; return LTPL_ERR_HIP; }
    return LTPL_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// planner (ABI v3): the OnlineTrajectoryHandler state machine of planner_core.hpp on top of the kernels above
// ---------------------------------------------------------------------------------------------------------------------
namespace {
struct HipCompute : ltplp::Compute {
    ltpl_handle* h;
    // a planner holds on to its lattice handle: the handle counts its planners and ltpl_destroy refuses while one is alive
    explicit HipCompute(ltpl_handle* handle) : h(handle) { ++h->n_planners; }
    ~HipCompute() override { --h->n_planners; }
    int plan_paths(const ltpl_paths_in* in, ltpl_paths_out* out) override { return ltpl_plan_paths(h, in, out); }
    int vel_profile(const ltpl_vel_params* p, int n, const ltpl_vel_job* jobs, ltpl_vel_result* res) override
    {
        return ltpl_vel_profile(h, p, n, jobs, res);
    }
    const char* last_error() override { return h->err.c_str(); }
};
}

extern "C" int ltpl_const_segment_test(const ltpl_handle* h, const double* seg, int32_t n_rows, const double* pos_est, int32_t n_veh,
                                       const double* veh_x, const double* veh_y, const double* veh_radius, int32_t* flags_out,
                                       int32_t* closest_out)
try {
    if (!h || !flags_out || !closest_out || n_veh < 0 || n_rows < 0) return LTPL_ERR_INVALID_ARG;
    if (!h->has_hostlat) return LTPL_ERR_UNSUPPORTED;
    int in_const, besides, closest;
    ltplp::const_segment_test(h->hostlat, n_rows > 0 ? seg : nullptr, n_rows, pos_est, n_veh, veh_x, veh_y, veh_radius, &in_const, &besides, &closest);
    *flags_out = (in_const ? LTPL_FLAG_OBJ_IN_CONST : 0) | (besides ? LTPL_FLAG_OBJ_BESIDES : 0);
    *closest_out = closest;
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(h))

extern "C" int ltpl_edge_capsules(int32_t n_edges, const int32_t* samp_ptr, const double* samp_x, const double* samp_y, int32_t n_samples,
                                  float* capsules_out, float* slack_out)
try {
    if (n_edges < 0 || !samp_ptr || !samp_x || !samp_y || !capsules_out || !slack_out) return LTPL_ERR_INVALID_ARG;
    *slack_out = ltplcap::build(n_edges, samp_ptr, samp_x, samp_y, n_samples, capsules_out);
    return LTPL_OK;
} LTPL_ABI_CATCH(nullptr)

extern "C" int ltpl_layer_grid(int32_t n_layers, const double* ref_x, const double* ref_y, double* origin_cell, int32_t* dims, int32_t* cells,
                               int32_t cap_cells)
try {
    if (n_layers < 1 || !ref_x || !ref_y || !origin_cell || !dims) return LTPL_ERR_INVALID_ARG;
    const ltplgrid::Grid g = ltplgrid::build(n_layers, ref_x, ref_y);
    origin_cell[0] = g.x0; origin_cell[1] = g.y0; origin_cell[2] = g.inv_cell;
    dims[0] = g.nx; dims[1] = g.ny;
    if (cells) {
        if ((size_t)cap_cells < (size_t)g.nx * g.ny) return LTPL_ERR_CAPACITY;
        memcpy(cells, g.cells.data(), sizeof(int32_t) * g.cells.size());
    }
    return LTPL_OK;
} LTPL_ABI_CATCH(nullptr)

extern "C" int ltpl_assembly_records(int32_t n_nodes, int32_t n_edges, const int32_t* in_ptr, const int32_t* edge_src, const double* edge_len,
                                     const int32_t* samp_ptr, const double* samp_x, const double* samp_y, const double* samp_psi,
                                     int32_t* node_rec_out, double* edge_rec_out)
try {
    if (n_nodes < 1 || n_edges < 1 || !in_ptr || !edge_src || !edge_len || !samp_ptr || !samp_x || !samp_y || !samp_psi || !node_rec_out ||
        !edge_rec_out) return LTPL_ERR_INVALID_ARG;
    std::vector<int32_t> nrec; std::vector<double> erec;
    ltplrec::build(n_nodes, n_edges, in_ptr, edge_src, edge_len, samp_ptr, samp_x, samp_y, samp_psi, nrec, erec);
    memcpy(node_rec_out, nrec.data(), sizeof(int32_t) * nrec.size());
    memcpy(edge_rec_out, erec.data(), sizeof(double) * erec.size());
    return LTPL_OK;
} LTPL_ABI_CATCH(nullptr)

extern "C" int ltpl_raceline_s(const ltpl_handle* h, double x, double y, double* s_out)
try {
    if (!h || !s_out) return LTPL_ERR_INVALID_ARG;
    if (!h->has_hostlat) return LTPL_ERR_UNSUPPORTED;
    *s_out = ltplp::raceline_s(h->hostlat, x, y);
    return LTPL_OK;
} LTPL_ABI_CATCH(abi_err_of(h))

extern "C" int ltpl_planner_create(ltpl_handle* h, const ltpl_planner_config* cfg, ltpl_planner** out)
try {
    g_create_error.clear();
    if (!h) { g_create_error = "planner: null handle"; return LTPL_ERR_INVALID_ARG; }
    if (!h->has_hostlat) { g_create_error = "planner: the lattice was created without raceline_x / raceline_y / node_psi"; return LTPL_ERR_UNSUPPORTED; }
    return ltplp::api_create(new HipCompute(h), h->hostlat, cfg, out, &g_create_error);
} LTPL_ABI_CATCH(nullptr)
extern "C" int ltpl_planner_destroy(ltpl_planner* p) { delete p; return LTPL_OK; }
extern "C" int ltpl_planner_get_caps(const ltpl_planner* p, ltpl_planner_caps* c) try { return ltplp::api_get_caps(p, c); } LTPL_ABI_CATCH(abi_err_of(p))
extern "C" const char* ltpl_planner_last_error(const ltpl_planner* p) { return p ? p->P.err.c_str() : g_create_error.c_str(); }
extern "C" int ltpl_planner_set_start(ltpl_planner* p, int32_t scen, double x, double y, double heading, double vel,
                                      double max_heading_offset, int32_t* in_track, int32_t* cor_heading)
try {
    if (!p || !in_track || !cor_heading) return LTPL_ERR_INVALID_ARG;
    return p->P.set_start(scen, x, y, heading, vel, max_heading_offset, in_track, cor_heading);
} LTPL_ABI_CATCH(abi_err_of(p))
extern "C" int ltpl_planner_calc_paths(ltpl_planner* p, const ltpl_planner_paths_in* in) try { return ltplp::api_calc_paths(p, in); } LTPL_ABI_CATCH(abi_err_of(p))
extern "C" int ltpl_planner_calc_paths_begin(ltpl_planner* p, const ltpl_planner_paths_in* in) try { return ltplp::api_calc_paths_begin(p, in); } LTPL_ABI_CATCH(abi_err_of(p))
extern "C" int ltpl_planner_calc_paths_finish(ltpl_planner* p, const int32_t* zo, const int32_t* zg) try { return ltplp::api_calc_paths_finish(p, zo, zg); } LTPL_ABI_CATCH(abi_err_of(p))
extern "C" int ltpl_planner_get_ref_idx(ltpl_planner* p, const double* px, const double* py) try { return (p && px && py) ? p->P.get_ref_idx(px, py) : LTPL_ERR_INVALID_ARG; } LTPL_ABI_CATCH(abi_err_of(p))
extern "C" int ltpl_planner_calc_vel_profile(ltpl_planner* p, const ltpl_planner_vel_in* in) try { return ltplp::api_calc_vel_profile(p, in); } LTPL_ABI_CATCH(abi_err_of(p))
extern "C" int ltpl_planner_get_paths(const ltpl_planner* p, int32_t scen, ltpl_planner_paths_view* v) try { return ltplp::api_get_paths(p, scen, v); } LTPL_ABI_CATCH(abi_err_of(p))
extern "C" int ltpl_planner_get_trajectories(const ltpl_planner* p, int32_t scen, ltpl_planner_traj_view* v) try { return ltplp::api_get_trajectories(p, scen, v); } LTPL_ABI_CATCH(abi_err_of(p))

#ifdef LTPL_EXPERIMENT
// experiment build only: the cross-lane helpers against plain loops on `rounds` waves of caller-provided values (vals: rounds x 128
// doubles, ivals: rounds x 64 ints, host memory); *n_bad = lanes that disagreed in some round
extern "C" int ltpl_exp_wave_ops_check(int32_t device, const double* vals, const int32_t* ivals, int32_t rounds, int32_t* n_bad)
try {
    if (!vals || !ivals || !n_bad || rounds <= 0) return LTPL_ERR_INVALID_ARG;
    if (hipSetDevice(device) != hipSuccess) return LTPL_ERR_HIP;
    double* dv = nullptr; int* di = nullptr; int* de = nullptr;
    int rc = LTPL_OK, zero = 0;
    if (hipMalloc(&dv, sizeof(double) * 128 * (size_t)rounds) != hipSuccess || hipMalloc(&di, sizeof(int) * 64 * (size_t)rounds) != hipSuccess ||
        hipMalloc(&de, sizeof(int)) != hipSuccess) rc = LTPL_ERR_HIP;
    if (!rc && (hipMemcpy(dv, vals, sizeof(double) * 128 * (size_t)rounds, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(di, ivals, sizeof(int) * 64 * (size_t)rounds, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(de, &zero, sizeof(int), hipMemcpyHostToDevice) != hipSuccess)) rc = LTPL_ERR_HIP;
    if (!rc) {
        hipLaunchKernelGGL(k_exp_wave_ops, dim3(1), dim3(64), 0, 0, dv, di, rounds, de);
        if (hipGetLastError() != hipSuccess || hipMemcpy(n_bad, de, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) rc = LTPL_ERR_HIP;
    }
    (void)hipFree(dv); (void)hipFree(di); (void)hipFree(de);
    return rc;
} LTPL_ABI_CATCH(nullptr)
#endif

#ifdef LTPL_EXPERIMENT
// experiment build only: heading_atan2 (path re-sampling) for n caller-provided (y, x) pairs (host memory)
__global__ void k_exp_heading(const double* y, const double* x, double* out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = heading_atan2(y[i], x[i]);
}
__global__ void k_exp_sincos(const double* x, double* sn, double* cs, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) heading_sincos(x[i], &sn[i], &cs[i]);
}
// experiment build only: heading_sincos (start heading of a scenario) for n caller-provided angles (host memory)
extern "C" int ltpl_exp_heading_sincos(int32_t device, const double* x, double* sn, double* cs, int32_t n)
try {
    if (!x || !sn || !cs || n <= 0) return LTPL_ERR_INVALID_ARG;
    if (hipSetDevice(device) != hipSuccess) return LTPL_ERR_HIP;
    double* d = nullptr;
    int rc = LTPL_OK;
    const size_t b = sizeof(double) * (size_t)n;
    if (hipMalloc(&d, 3 * b) != hipSuccess) return LTPL_ERR_HIP;
    if (hipMemcpy(d, x, b, hipMemcpyHostToDevice) != hipSuccess) rc = LTPL_ERR_HIP;
    if (!rc) {
        hipLaunchKernelGGL(k_exp_sincos, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d, d + n, d + 2 * (size_t)n, n);
        if (hipGetLastError() != hipSuccess || hipMemcpy(sn, d + n, b, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(cs, d + 2 * (size_t)n, b, hipMemcpyDeviceToHost) != hipSuccess) rc = LTPL_ERR_HIP;
    }
    (void)hipFree(d);
    return rc;
} LTPL_ABI_CATCH(nullptr)
extern "C" int ltpl_exp_heading_atan2(int32_t device, const double* y, const double* x, double* out, int32_t n)
try {
    if (!y || !x || !out || n <= 0) return LTPL_ERR_INVALID_ARG;
    if (hipSetDevice(device) != hipSuccess) return LTPL_ERR_HIP;
    double* d = nullptr;
    int rc = LTPL_OK;
    const size_t b = sizeof(double) * (size_t)n;
    if (hipMalloc(&d, 3 * b) != hipSuccess) return LTPL_ERR_HIP;
    if (hipMemcpy(d, y, b, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d + n, x, b, hipMemcpyHostToDevice) != hipSuccess) rc = LTPL_ERR_HIP;
    if (!rc) {
        hipLaunchKernelGGL(k_exp_heading, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d, d + n, d + 2 * (size_t)n, n);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, d + 2 * (size_t)n, b, hipMemcpyDeviceToHost) != hipSuccess) rc = LTPL_ERR_HIP;
    }
    (void)hipFree(d);
    return rc;
} LTPL_ABI_CATCH(nullptr)
// experiment build only: fast_rcp (reciprocals of the spline solve and of the re-sampling parameter) / rsqrt_cubed (curvature of a path
// sample) for n caller-provided values (host memory)
__global__ void k_exp_fast_rcp(const double* x, double* out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = fast_rcp(x[i]);
}
__global__ void k_exp_rsqrt_cubed(const double* x, double* out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rsqrt_cubed(x[i]);
}
static int exp_unary(int32_t device, const double* x, double* out, int32_t n, bool cubed)
{
    if (!x || !out || n <= 0) return LTPL_ERR_INVALID_ARG;
    if (hipSetDevice(device) != hipSuccess) return LTPL_ERR_HIP;
    double* d = nullptr;
    int rc = LTPL_OK;
    const size_t b = sizeof(double) * (size_t)n;
    if (hipMalloc(&d, 2 * b) != hipSuccess) return LTPL_ERR_HIP;
    if (hipMemcpy(d, x, b, hipMemcpyHostToDevice) != hipSuccess) rc = LTPL_ERR_HIP;
    if (!rc) {
        const dim3 grid((unsigned)((n + 255) / 256));
        if (cubed) hipLaunchKernelGGL(k_exp_rsqrt_cubed, grid, dim3(256), 0, 0, d, d + n, n);
        else hipLaunchKernelGGL(k_exp_fast_rcp, grid, dim3(256), 0, 0, d, d + n, n);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, d + n, b, hipMemcpyDeviceToHost) != hipSuccess) rc = LTPL_ERR_HIP;
    }
    (void)hipFree(d);
    return rc;
}
extern "C" int ltpl_exp_fast_rcp(int32_t device, const double* x, double* out, int32_t n)
try { return exp_unary(device, x, out, n, false); } LTPL_ABI_CATCH(nullptr)
extern "C" int ltpl_exp_rsqrt_cubed(int32_t device, const double* x, double* out, int32_t n)
try { return exp_unary(device, x, out, n, true); } LTPL_ABI_CATCH(nullptr)
#endif

// ---------------------------------------------------------------------------------------------------------------------
// fleet (ABI v5): planners with device-resident state
// ---------------------------------------------------------------------------------------------------------------------
#include "fleet_dev.hpp"
#include "fleet_sim.hpp"
#include "fleet_branch.hpp"
#include "fleet_friction.hpp"
#include "fleet_events.hpp"

#ifdef LTPL_EXPERIMENT
// experiment build only: the device's projections of a point on a polyline (get_s_coord.py:8-99), one form per call, for nq caller-provided
// queries on a caller-provided polyline (x, y, s: n entries each, host memory). form 0: get_s_coord_dev (one wave per query; i1_out = -1),
// 1: globrl_index_dev (one wave per query) and 2: lane_globrl_index (one lane per query) through a DevLat in which only grx, gry and G are
// set (closed lines; s_out = NaN, i1_out = -1), 3: project_on_polyline of fleet_core.hpp through WaveX (one wave per query).
__global__ __launch_bounds__(64) void k_exp_project(int form, int n, const double* x, const double* y, const double* s, int closed, int nq,
                                                    const double* qx, const double* qy, double* s_out, int* i0_out, int* i1_out)
{
    const int lane = threadIdx.x;
    if (form == 2) {
        const int q0 = (int)blockIdx.x * 64 + lane, q = q0 < nq ? q0 : nq - 1;      // (idle lanes repeat the last query: every lane must call)
        DevLat lat; memset(&lat, 0, sizeof(lat));
        lat.grx = x; lat.gry = y; lat.G = n + 1;
        const int idx = lane_globrl_index(lat, qx[q], qy[q]);
        if (q0 < nq) { s_out[q] = NAN; i0_out[q] = idx; i1_out[q] = -1; }
        return;
    }
    const int q = (int)blockIdx.x;
    if (q >= nq) return;
    double sv = NAN; int i0 = -1, i1 = -1;
    if (form == 0) sv = get_s_coord_dev(n, x, y, 1, s, 1, qx[q], qy[q], closed != 0, lane, &i0);
    else if (form == 1) {
        DevLat lat; memset(&lat, 0, sizeof(lat));
        lat.grx = x; lat.gry = y; lat.G = n + 1;
        i0 = globrl_index_dev(lat, qx[q], qy[q], lane);
    } else {
        const WaveX wx{lane};
        const fleet::Poly pl{x, y, 1, n};
        const fleet::Foot f = fleet::project_on_polyline(wx, pl, qx[q], qy[q], closed != 0, true, s, 1, n);
        sv = f.s; i0 = f.i0; i1 = f.i1;
    }
    if (lane == 0) { s_out[q] = sv; i0_out[q] = i0; i1_out[q] = i1; }
}
extern "C" int ltpl_exp_project(int32_t device, int32_t form, int32_t n, const double* x, const double* y, const double* s, int32_t closed,
                                int32_t nq, const double* qx, const double* qy, double* s_out, int32_t* i0_out, int32_t* i1_out)
try {
    if (!x || !y || !s || !qx || !qy || !s_out || !i0_out || !i1_out || n < 2 || nq <= 0 || form < 0 || form > 3) return LTPL_ERR_INVALID_ARG;
    if ((form == 1 || form == 2) && !closed) return LTPL_ERR_INVALID_ARG;
    if (hipSetDevice(device) != hipSuccess) return LTPL_ERR_HIP;
    double* d = nullptr; int* di = nullptr;
    int rc = LTPL_OK;
    const size_t bn = sizeof(double) * (size_t)n, bq = sizeof(double) * (size_t)nq, iq = sizeof(int) * (size_t)nq;
    if (hipMalloc(&d, 3 * bn + 3 * bq) != hipSuccess) return LTPL_ERR_HIP;
    if (hipMalloc(&di, 2 * iq) != hipSuccess) { (void)hipFree(d); return LTPL_ERR_HIP; }
    double* dx = d; double* dy = d + n; double* ds = d + 2 * (size_t)n; double* dqx = d + 3 * (size_t)n; double* dqy = dqx + nq; double* dso = dqy + nq;
    if (hipMemcpy(dx, x, bn, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dy, y, bn, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ds, s, bn, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dqx, qx, bq, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dqy, qy, bq, hipMemcpyHostToDevice) != hipSuccess) rc = LTPL_ERR_HIP;
    if (!rc) {
        const unsigned blocks = form == 2 ? (unsigned)((nq + 63) / 64) : (unsigned)nq;
        hipLaunchKernelGGL(k_exp_project, dim3(blocks), dim3(64), 0, 0, form, n, dx, dy, ds, closed, nq, dqx, dqy, dso, di, di + nq);
        if (hipGetLastError() != hipSuccess || hipMemcpy(s_out, dso, bq, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(i0_out, di, iq, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(i1_out, di + nq, iq, hipMemcpyDeviceToHost) != hipSuccess) rc = LTPL_ERR_HIP;
    }
    (void)hipFree(d); (void)hipFree(di);
    return rc;
} LTPL_ABI_CATCH(nullptr)
#endif
