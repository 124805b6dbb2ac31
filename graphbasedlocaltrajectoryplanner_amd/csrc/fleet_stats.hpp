// fleet_stats.hpp -- campaign statistics of the fleet's closed-loop simulation (ltpl_fleet_sim_stats, include/ltpl_hip.h): one field of the
// planners' records reduced per group of planners -- counts, minimum and maximum with the planner that holds them, sum and sum of squares,
// a histogram and the K worst planners. Plain functions, host- and device-compilable, no HIP types: tests/sim_stats_shim.cpp compiles this
// file alone with the host compiler; the host mirror is sim.stats_reduce / sim.StatsModel. Measurement only: no kernel of the tick reads
// what is written here. fp64, + - * / and comparisons only, in the order written here (built with -ffp-contract=off on both sides); no
// trigonometry, no floating-point atomics: every sum has ONE order, which does not depend on the launch geometry.
//
// A GROUP is a list of members i = 0 .. n - 1, member i being planner p_i with value v_i (planners ascending in a plan's groups; any
// order in the test hook). One value:
//   NaN (v != v)    counted in n_nan, takes part in nothing else
//   +-inf           counted in n_inf; takes part in min / max / top-K and in under / over; not in n, sum, sumsq or the cells
//   finite          n += 1, sum, sumsq (v * v), min / max, one histogram cell
// MINIMUM on the key (v, p), MAXIMUM on the key (-v, p): a strict compare of the values decides, ties go to the lower planner, so a -0.0
// that ties with a +0.0 keeps the bits of the lower planner's value. Empty: min = +inf, argmin = -1, max = -inf, argmax = -1.
// HISTOGRAM: edges e_j = lo + ((hi - lo) * j) / bins, j = 0 .. bins, in exactly this order (stats_edges; the host computes them once per
// measure and the device reads them). under: v < e_0; over: v >= e_bins; cell j: e_j <= v < e_(j+1) -- the largest j < bins with e_j <= v.
// TOP-K: the K smallest keys (v, p) for top_dir = -1, (-v, p) for top_dir = +1, in order, by K rounds "the smallest key strictly above the
// last winner" (two members with the same key count once: a plan's planners are distinct). A NaN never enters, an infinity may. Unused
// entries are (NaN, -1).
// SUM ORDER (sum and sumsq), the contract between kernel and mirror:
//   1  members are cut into chunks of kStatsChunk = 1024 consecutive positions
//   2  inside a chunk lane l = i mod 64 adds its values serially in ascending i, starting from +0.0; a skipped value adds nothing
//   3  the 64 lane sums are folded by the tree t[l] = t[l] + t[l + s] for l < s, s = 32, 16, 8, 4, 2, 1
//   4  the chunk sums are added serially in ascending chunk order, starting from +0.0
// Everything else (counts, cells, extrema, top-K) is exact and order-free; the chunk partials are folded in ascending chunk order all the same.
// THE ROW, STA_DOUBLES = 27 doubles: n, n_nan, n_inf, min, argmin, max, argmax, sum, sumsq, under, over, hist[16] (unused cells 0).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FLEET_STATS_FN __host__ __device__ inline
#else
#define FLEET_STATS_FN inline
#endif

namespace fleet {

enum { STA_N = 0, STA_N_NAN, STA_N_INF, STA_MIN, STA_ARGMIN, STA_MAX, STA_ARGMAX, STA_SUM, STA_SUMSQ, STA_UNDER, STA_OVER, STA_HIST,
       STA_DOUBLES = STA_HIST + 16 };
enum { kStatsChunk = 1024, kStatsLanes = 64, kStatsBins = 16, kStatsTop = 8, kStatsNoPlanner = 0x7fffffff };
// what a value is to the histogram: a cell 0 .. 15, under, over, or nothing (a NaN)
enum { kStatsUnder = kStatsBins, kStatsOver = kStatsBins + 1, kStatsClasses = kStatsBins + 2, kStatsNoClass = -1 };
// the families of a measure: the eight records and the planner's state (column 0: failed)
enum { STA_FAM_TELEMETRY = 0, STA_FAM_VEHICLE, STA_FAM_SENSOR, STA_FAM_TRACKER, STA_FAM_PREDICTOR, STA_FAM_SELECTOR, STA_FAM_SAFETY, STA_FAM_REACT,
       STA_FAM_STATE, STA_FAMILIES, STA_FAM_RECORDS = STA_FAM_STATE };

FLEET_STATS_FN bool stats_nan(double v) { return v != v; }
FLEET_STATS_FN bool stats_finite(double v) { return v - v == 0.0; }

// e[0 .. bins]
FLEET_STATS_FN void stats_edges(double lo, double hi, int bins, double* e)
{
    for (int j = 0; j <= bins; ++j) e[j] = lo + ((hi - lo) * (double)j) / (double)bins;
}
FLEET_STATS_FN int stats_class(double v, const double* e, int bins)
{
    if (stats_nan(v)) return kStatsNoClass;
    if (v < e[0]) return kStatsUnder;
    if (v >= e[bins]) return kStatsOver;
    int cell = 0;
    for (int j = 1; j < bins; ++j) if (e[j] <= v) cell = j;
    return stats_finite(v) ? cell : kStatsNoClass;     // (an infinity between the edges: the edges themselves are not finite)
}
// key (a, pa) in front of key (b, pb)
FLEET_STATS_FN bool stats_before(double a, int pa, double b, int pb) { return a < b || (a == b && pa < pb); }
// the key of the top-K list and back
FLEET_STATS_FN double stats_top_key(double v, int top_dir) { return top_dir > 0 ? -v : v; }

// the start state of a row and of a top-K list
FLEET_STATS_FN void stats_start(double* row, double* top)
{
    for (int i = 0; i < STA_DOUBLES; ++i) row[i] = 0.0;
    row[STA_MIN] = INFINITY; row[STA_ARGMIN] = -1.0; row[STA_MAX] = -INFINITY; row[STA_ARGMAX] = -1.0;
    if (top) for (int r = 0; r < kStatsTop; ++r) { top[2 * r] = NAN; top[2 * r + 1] = -1.0; }
}

// one chunk on the host: cnt <= 1024 members -> the partial row and the partial top-K list (always kStatsTop entries, top_k of them used)
inline void stats_chunk_host(const double* v, const int* p, int cnt, const double* e, int bins, int top_dir, int top_k, double* row, double* top)
{
    stats_start(row, top);
    double t[kStatsLanes], q[kStatsLanes];
    for (int l = 0; l < kStatsLanes; ++l) { t[l] = 0.0; q[l] = 0.0; }
    double mn = INFINITY, xk = INFINITY; int mp = kStatsNoPlanner, xp = kStatsNoPlanner;
    for (int i = 0; i < cnt; ++i) {
        const double x = v[i];
        if (stats_nan(x)) { row[STA_N_NAN] += 1.0; continue; }
        if (stats_before(x, p[i], mn, mp)) { mn = x; mp = p[i]; }
        if (stats_before(-x, p[i], xk, xp)) { xk = -x; xp = p[i]; }
        const int c = stats_class(x, e, bins);
        if (c == kStatsUnder) row[STA_UNDER] += 1.0;
        else if (c == kStatsOver) row[STA_OVER] += 1.0;
        if (!stats_finite(x)) { row[STA_N_INF] += 1.0; continue; }
        row[STA_N] += 1.0;
        if (c >= 0 && c < kStatsBins) row[STA_HIST + c] += 1.0;
        const int l = i % kStatsLanes;
        t[l] = t[l] + x; q[l] = q[l] + x * x;
    }
    for (int s = kStatsLanes / 2; s >= 1; s >>= 1) for (int l = 0; l < s; ++l) { t[l] = t[l] + t[l + s]; q[l] = q[l] + q[l + s]; }
    row[STA_SUM] = t[0]; row[STA_SUMSQ] = q[0];
    if (mp != kStatsNoPlanner) { row[STA_MIN] = mn; row[STA_ARGMIN] = (double)mp; row[STA_MAX] = -xk; row[STA_ARGMAX] = (double)xp; }
    double lk = -INFINITY; int lp = -1;
    for (int r = 0; r < top_k && top_dir != 0; ++r) {
        double bk = INFINITY; int bp = kStatsNoPlanner;
        for (int i = 0; i < cnt; ++i) {
            if (stats_nan(v[i])) continue;
            const double k = stats_top_key(v[i], top_dir);
            if (stats_before(lk, lp, k, p[i]) && stats_before(k, p[i], bk, bp)) { bk = k; bp = p[i]; }
        }
        if (bp == kStatsNoPlanner) break;
        top[2 * r] = stats_top_key(bk, top_dir); top[2 * r + 1] = (double)bp;
        lk = bk; lp = bp;
    }
}

// the partials of a group's n_chunks chunks, part_row[c][27] and part_top[c][8][2], folded in ascending chunk order
inline void stats_merge_host(const double* part_row, const double* part_top, int n_chunks, int top_dir, int top_k, double* row, double* top)
{
    stats_start(row, top);
    for (int c = 0; c < n_chunks; ++c) {
        const double* pr = part_row + (size_t)c * STA_DOUBLES;
        for (int i = 0; i < STA_DOUBLES; ++i) if (i < STA_MIN || i > STA_ARGMAX) row[i] = row[i] + pr[i];
        const int pa = (int)pr[STA_ARGMIN], px = (int)pr[STA_ARGMAX];
        if (pa >= 0 && (row[STA_ARGMIN] < 0.0 || stats_before(pr[STA_MIN], pa, row[STA_MIN], (int)row[STA_ARGMIN]))) {
            row[STA_MIN] = pr[STA_MIN]; row[STA_ARGMIN] = pr[STA_ARGMIN];
        }
        if (px >= 0 && (row[STA_ARGMAX] < 0.0 || stats_before(-pr[STA_MAX], px, -row[STA_MAX], (int)row[STA_ARGMAX]))) {
            row[STA_MAX] = pr[STA_MAX]; row[STA_ARGMAX] = pr[STA_ARGMAX];
        }
    }
    double lk = -INFINITY; int lp = -1;
    for (int r = 0; r < top_k && top_dir != 0; ++r) {
        double bk = INFINITY; int bp = kStatsNoPlanner;
        for (int t = 0; t < n_chunks * kStatsTop; ++t) {
            const int p = (int)part_top[2 * (size_t)t + 1];
            if (p < 0) continue;
            const double k = stats_top_key(part_top[2 * (size_t)t], top_dir);
            if (stats_before(lk, lp, k, p) && stats_before(k, p, bk, bp)) { bk = k; bp = p; }
        }
        if (bp == kStatsNoPlanner) break;
        top[2 * r] = stats_top_key(bk, top_dir); top[2 * r + 1] = (double)bp;
        lk = bk; lp = bp;
    }
}

}  // namespace fleet
