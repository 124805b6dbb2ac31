// Host build of csrc/fleet_stats.hpp for tests/test_sim_stats_host.py: the header compiled alone with the host compiler
// (g++ -ffp-contract=off), against sim.stats_reduce.
#include "../graphbasedlocaltrajectoryplanner_amd/csrc/fleet_stats.hpp"

#include <vector>

extern "C" {

int stats_row_doubles() { return fleet::STA_DOUBLES; }
int stats_chunk_members() { return fleet::kStatsChunk; }
int stats_max_top() { return fleet::kStatsTop; }
int stats_families() { return fleet::STA_FAMILIES; }

// e[bins + 1]
void stats_edges_host(double lo, double hi, int bins, double* e) { fleet::stats_edges(lo, hi, bins, e); }

// one group and one measure: values[n] with their planners[n] -> row[27], top[8][2]; chunk after chunk, then the fold of the partials
void stats_reduce_host(const double* values, const int* planners, int n, double lo, double hi, int bins, int top_dir, int top_k, double* row, double* top)
{
    double e[fleet::kStatsBins + 1];
    fleet::stats_edges(lo, hi, bins, e);
    const int nc = (n + fleet::kStatsChunk - 1) / fleet::kStatsChunk;
    std::vector<double> pr((size_t)nc * fleet::STA_DOUBLES + 1), pt((size_t)nc * 2 * fleet::kStatsTop + 1);
    for (int c = 0; c < nc; ++c) {
        const int i0 = c * fleet::kStatsChunk, cnt = n - i0 < fleet::kStatsChunk ? n - i0 : (int)fleet::kStatsChunk;
        fleet::stats_chunk_host(values + i0, planners + i0, cnt, e, bins, top_dir, top_k, pr.data() + (size_t)c * fleet::STA_DOUBLES,
                                pt.data() + (size_t)c * 2 * fleet::kStatsTop);
    }
    fleet::stats_merge_host(pr.data(), pt.data(), nc, top_dir, top_k, row, top);
}

}
