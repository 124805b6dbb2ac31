// Host build of csrc/fleet_track.hpp for tests/test_sim_tracker_host.py: the header compiled alone with the host compiler
// (g++ -ffp-contract=off), against sim.TrackerModel. With -DSIM_TRACKER_SHIM_MAIN the file is a stand-alone program that runs seeded random
// cases at the capacity edges (built with -fsanitize=address,undefined by the test, run once, exit status 0).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../graphbasedlocaltrajectoryplanner_amd/csrc/fleet_track.hpp"

extern "C" {

// one tick of one table. params[5] = gate, w_pos, w_vel, n_confirm, n_coast; tracks: [cap][10], *n_trk rows in use (updated in place);
// dets: [K][6] = x, y, px, py, r, v (a staged object); out: [slots][6]; assign: [K]; rec: [12], accumulated
void tracker_step_host(const double* params, double adv, double tick, int cap, int slots, double* tracks, int* n_trk, double* next_id, const double* dets,
                       int K, double* out, int* n_out, int* assign, double* rec)
{
    const fleet::TrackParams P{params[0], params[1], params[2], params[3], params[4]};
    std::vector<fleet::TrackRow> rows((size_t)(cap > 0 ? cap : 1));
    std::memcpy(rows.data(), tracks, sizeof(double) * fleet::TRK_DOUBLES * (size_t)*n_trk);
    std::vector<fleet::TrackDet> det((size_t)(K > 0 ? K : 1));
    for (int k = 0; k < K; ++k) det[(size_t)k] = fleet::track_det(dets[6 * k], dets[6 * k + 1], dets[6 * k + 2], dets[6 * k + 3], dets[6 * k + 4], dets[6 * k + 5]);
    std::vector<double> o((size_t)(slots > 0 ? slots : 1) * 6);
    fleet::track_step(P, adv, tick, cap, slots, rows.data(), n_trk, next_id, det.data(), K, o.data(), n_out, assign, rec);
    std::memcpy(tracks, rows.data(), sizeof(double) * fleet::TRK_DOUBLES * (size_t)*n_trk);
    std::memcpy(out, o.data(), sizeof(double) * 6 * (size_t)*n_out);
}

}

#ifdef SIM_TRACKER_SHIM_MAIN
namespace {
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
double uni()      // xorshift64*: [0, 1)
{
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}
}

int main()
{
    static const int edges[] = {0, 1, 2, 47, 48, 63, 64, 65, 95, 96};
    long steps = 0, handed = 0;
    for (int slots : edges) {
        const int cap = 2 * slots < fleet::kTrackCap ? 2 * slots : (int)fleet::kTrackCap;
        for (int variant = 0; variant < 6; ++variant) {
            const double params[5] = {variant % 2 ? 3.0 : 60.0, 0.25 * (variant % 3), 0.4, (double)(1 + variant % 3), (double)(variant % 4)};
            std::vector<double> tracks((size_t)(cap > 0 ? cap : 1) * fleet::TRK_DOUBLES), out((size_t)(slots > 0 ? slots : 1) * 6), dets((size_t)(slots > 0 ? slots : 1) * 6);
            std::vector<int> assign((size_t)(slots > 0 ? slots : 1));
            double rec[fleet::TRS_DOUBLES] = {0.0}, next_id = 0.0;
            int n_trk = 0;
            for (int tick = 0; tick < 12; ++tick) {
                // every other tick the full list, in between a random share of it: tracks coast, die and are born at the capacity
                const int K = tick % 2 ? (int)(uni() * (slots + 1)) : slots;
                for (int k = 0; k < K; ++k) {
                    const double x = 100.0 * uni(), y = 100.0 * uni();
                    double* d = &dets[(size_t)6 * k];
                    d[0] = x; d[1] = y; d[2] = x + uni(); d[3] = y + uni(); d[4] = 1.0 + uni(); d[5] = 30.0 * uni();
                }
                int n_out = -1;
                tracker_step_host(params, 0.5, (double)tick, cap, slots, tracks.data(), &n_trk, &next_id, dets.data(), K < slots ? K : slots, out.data(),
                                  &n_out, assign.data(), rec);
                if (n_trk < 0 || n_trk > cap || n_out < 0 || n_out > slots) { std::fprintf(stderr, "tracker shim: counts out of range\n"); return 1; }
                ++steps; handed += n_out;
            }
            if (rec[fleet::TRS_TICKS] != 12.0 || rec[fleet::TRS_TRACKS_MAX] > (double)cap) { std::fprintf(stderr, "tracker shim: record\n"); return 1; }
        }
    }
    std::printf("tracker shim: %ld steps, %ld objects handed on\n", steps, handed);
    return 0;
}
#endif
