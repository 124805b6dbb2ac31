// vel_layout.hpp -- the ONE definition of every buffer the velocity stage carves, and of its kernel-variant table: the per-wave LDS scratch
// (the device carves, the host sizes the launch by running the same carve), the dynamic LDS of the fused tick, the tiled planes of the lane
// kernels in HBM, and with_vel_variant. Plain functions, host- and device-compilable, no HIP types: tests/vel_layout_shim.cpp compiles this
// file alone with the host compiler.
#pragma once

#include <cstddef>
#include <type_traits>

#include "../../include/ltpl_hip.h"

#if defined(__HIPCC__)
#define VEL_LAYOUT_FN __host__ __device__ __forceinline__
#else
#define VEL_LAYOUT_FN inline
#endif

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// per-wave LDS scratch of the velocity stage; every array holds cap + 2 doubles
struct VelScratch {
    double* w;        // profile state (v^2)
    double* kabs;     // |kappa|
    double* el;       // element lengths
    double* gax;      // per-point longitudinal limit (nullptr -> constant)
    double* gay;      // per-point lateral limit      (nullptr -> constant)
    double* igay;     // 1 / gay (division-free recurrence)
    double* axm;      // LDS copy of ax_max_machines rows [v, ax] (<= 64 rows)
    long long* dbg;
    double* s;        // arc length (cap + 1)
    double* wb;       // ego brake profile (follow)
    double* wc;       // scratch profile (follow)
    unsigned char* start;   // run-start flags (cap + 16 bytes)
    double* chunk;    // 128 doubles: staging of the global race line for the opponent brake scan
    int cap;
};

// `lite`: only what the forward-backward and brake profiles touch (w, kabs, el, machine table, run flags) -- no arc length, no follow scratch
VEL_LAYOUT_FN VelScratch carve_vel_scratch(unsigned char* base, int cap, bool with_gg, bool with_xy,
                                           double** px, double** py, bool lite = false)
{
    VelScratch vs;
    double* d = reinterpret_cast<double*>(base);
    const int c1 = cap + 2;
    vs.w = d; d += c1; vs.kabs = d; d += c1; vs.el = d; d += c1;
    if (!lite) { vs.s = d; d += c1; vs.wb = d; d += c1; vs.wc = d; d += c1; }
    else { vs.s = nullptr; vs.wb = nullptr; vs.wc = nullptr; }
    if (with_gg) { vs.gax = d; d += c1; vs.gay = d; d += c1; vs.igay = d; d += c1; }
    else { vs.gax = nullptr; vs.gay = nullptr; vs.igay = nullptr; }
    if (with_xy) { *px = d; d += c1; *py = d; d += c1; }
    if (!lite) { vs.chunk = d; d += 128; } else vs.chunk = nullptr;
    vs.axm = d; d += 128;
    vs.start = reinterpret_cast<unsigned char*>(d);
    vs.cap = cap;
    vs.dbg = nullptr;
    return vs;
}

// Bytes of one wave's scratch: where the carve puts the run-start flags, the cap + 16 flag bytes behind that, rounded up to 16. The carve
// runs on a stand-in base that is never read through (not the null pointer: an offset added to it is what UBSan reports).
inline size_t vel_scratch_bytes(int cap, bool with_gg, bool with_xy, bool lite = false)
{
    unsigned char* const base = reinterpret_cast<unsigned char*>(static_cast<size_t>(4096));
    double* px; double* py;
    const VelScratch vs = carve_vel_scratch(base, cap, with_gg, with_xy, &px, &py, lite);
    return align_up((size_t)(vs.start - base) + (size_t)cap + 16, 16);
}

// Dynamic LDS of the fused tick: [the path team's block: lp4_total = vel_off][LTPL_MAX_ACTIONS x scratch(with_xy) of vel_stride bytes][flags of
// the fourth wave]. That wave computes the follow slot's unconstrained profile in wave 0's arrays and keeps run-start flags of its own.
VEL_LAYOUT_FN size_t fused_tick_flags_off(int vel_off, int vel_stride) { return (size_t)vel_off + (size_t)LTPL_MAX_ACTIONS * vel_stride; }
inline size_t fused_tick_lds(int lp4_total, int cap)
{
    return fused_tick_flags_off(lp4_total, (int)vel_scratch_bytes(cap, false, true)) + align_up((size_t)cap + 16, 16);
}

// Tiled planes of the lane kernels (vel_lanes.hpp: VelPlanes; tick_host.hpp adds the base pointer) as byte offsets into one block, in this
// order. Tile index = job index: generic jobs [0, n_slots_pad), follow jobs behind them.
struct VelPlanesLayout {
    size_t KE, P0, P1, P2, P3, XY, flags, job_slot, job_cnt, fseg;
    int n_slots_pad, n_scen_pad, plane_rows;    // slots / scenarios rounded up to 64 (whole tiles), cap_pts rounded up to 8
    size_t bytes;                               // 0, like every offset: the tick does not run as the pipeline and has no planes
};
inline VelPlanesLayout vel_planes_layout(int n_scen, int cap_pts, bool pipeline = true)
{
    VelPlanesLayout L{};
    L.n_slots_pad = (int)align_up((size_t)n_scen * LTPL_MAX_ACTIONS, 64); L.n_scen_pad = (int)align_up((size_t)n_scen, 64);
    L.plane_rows = (int)align_up((size_t)cap_pts, 8);
    if (!pipeline) return L;
    const size_t follow = (size_t)L.n_scen_pad, jobs = (size_t)L.n_slots_pad + follow;
    const size_t rec = 2 * sizeof(double) * (size_t)L.plane_rows, col = sizeof(double) * (size_t)cap_pts;      // bytes per job: operand records, a profile
    auto take = [&L](size_t n) { const size_t o = L.bytes; L.bytes += n; return o; };
    L.KE = take(rec * jobs); L.P0 = take(col * jobs);                                                            // all jobs
    L.P1 = take(col * follow); L.P2 = take(col * follow); L.P3 = take(col * follow); L.XY = take(rec * follow);   // follow jobs
    L.flags = take(sizeof(int) * jobs); L.job_slot = take(2 * sizeof(int) * jobs); L.job_cnt = take(sizeof(int) * 16); L.fseg = take(2 * sizeof(int) * follow);
    return L;
}

// Kernel variant v = 2 * EM + AXM1 (vel_variant: EM 1 / 2 = exponent 1 / 2, 0 = general pow; AXM1 = one-row machine table): f(EM, AXM1) with
// both as std::integral_constant objects, so that `em.value` / `axm1.value` are template arguments. Any other v runs as the last variant.
template <class F>
static auto with_vel_variant(int v, F&& f)
{
    using std::integral_constant; using std::false_type; using std::true_type;
    switch (v) {
        case 0: return f(integral_constant<int, 0>{}, false_type{}); case 1: return f(integral_constant<int, 0>{}, true_type{});
        case 2: return f(integral_constant<int, 1>{}, false_type{}); case 3: return f(integral_constant<int, 1>{}, true_type{});
        case 4: return f(integral_constant<int, 2>{}, false_type{}); default: return f(integral_constant<int, 2>{}, true_type{});
    }
}
