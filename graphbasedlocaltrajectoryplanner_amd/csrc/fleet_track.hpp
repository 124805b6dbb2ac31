// fleet_track.hpp -- the object tracker of the fleet's closed-loop simulation (ltpl_fleet_sim_tracker, include/ltpl_hip.h): what a planner is
// handed of the tick's detections, with memory from tick to tick. Plain functions, host- and device-compilable, no HIP types:
// tests/sim_tracker_shim.cpp compiles this file alone with the host compiler; the host mirror is sim.TrackerModel. fp64, + - * and
// comparisons only, in the order written here (built with -ffp-contract=off on both sides): no trigonometry, no division, no square root.
// The one division, adv = dt / 0.2 (the tick period over the ingestion's prediction horizon), is formed once per fleet by the caller.
//
// Per planner: a table of T <= cap tracks (x, y, ex, ey, r, v, id, hits, miss, born_tick) and the tick's detections k = 0 .. K - 1
// (x, y, e = (px - x, py - y), r, v). One tick, in this order:
//   1 predict    xp = x + adv ex, yp = y + adv ey                      (the product first, then the sum)
//   2 associate  d2(t, k) = dx dx + dy dy, dx = x_k - xp_t, dy = y_k - yp_t; candidates d2 <= gate gate in ascending (d2, t, k); a candidate
//                is accepted when neither its track nor its detection was accepted before (greedy global nearest neighbour)
//   3 update     matched: x = x_k + w_pos (xp - x_k), y likewise; ex = e_kx + w_vel (ex - e_kx), ey and v likewise; r = r_k; hits += 1;
//                miss = 0                                              (w = 0: the track is the detection)
//   4 miss       unmatched: hits < n_confirm: deleted (tentative); else miss += 1; miss > n_coast: deleted; else x = xp, y = yp (coasting)
//   5 births     unmatched detections in ascending k, behind the survivors while the table holds fewer than cap tracks: the detection's
//                values, id = next_id++, hits = 1, miss = 0, born_tick = tick; otherwise counted as overflow
//   6 order      the survivors in their previous order, then the births in detection order (a stable compaction)
//   7 hand on    the confirmed tracks (hits >= n_confirm) matched or born this tick in table order, then the confirmed coasting tracks in
//                table order until `slots` objects are handed on (the rest: withheld): x, y, x + ex, y + ey, r, v
// track_step below is the tick in serial form (the reference of the shim); k_fleet_sim_track (fleet_sim.hpp) runs the same elemental
// functions one wave per planner.
#pragma once

#include <cmath>
#include <cstdint>

#include "fleet_noise.hpp"

#define FLEET_TRACK_FN FLEET_NOISE_FN

namespace fleet {

enum { TRK_X = 0, TRK_Y, TRK_EX, TRK_EY, TRK_R, TRK_V, TRK_ID, TRK_HITS, TRK_MISS, TRK_BORN, TRK_DOUBLES };
enum { TRS_TICKS = 0, TRS_N_DET, TRS_N_MATCHED, TRS_N_BORN, TRS_N_CONFIRMED, TRS_N_DEL_TENT, TRS_N_DEL_COAST, TRS_N_OUT, TRS_N_OUT_COAST,
       TRS_N_WITHHELD, TRS_N_OVERFLOW, TRS_TRACKS_MAX, TRS_DOUBLES };
enum { kTrackCap = 96, kTrackUnmatched = -1, kTrackOverflow = -2 };

struct TrackParams { double gate, w_pos, w_vel, n_confirm, n_coast; };
struct TrackDet { double x, y, ex, ey, r, v; };
struct TrackRow { double f[TRK_DOUBLES]; };

// the detection of a staged object (g_x, g_y, g_px, g_py, g_r, g_v): e is the ingestion's displacement over its horizon
FLEET_TRACK_FN TrackDet track_det(double x, double y, double px, double py, double r, double v) { return TrackDet{x, y, px - x, py - y, r, v}; }

FLEET_TRACK_FN double track_predict(double x, double adv, double e)
{
    const double step = adv * e;
    return x + step;
}
FLEET_TRACK_FN double track_d2(double xk, double yk, double xp, double yp)
{
    const double dx = xk - xp, dy = yk - yp;
    return dx * dx + dy * dy;
}
FLEET_TRACK_FN double track_gate2(double gate) { return gate * gate; }
FLEET_TRACK_FN bool track_gated(double d2, double gate2) { return d2 <= gate2; }
// detection + w (prediction - detection)
FLEET_TRACK_FN double track_blend(double det, double w, double pred)
{
    const double diff = pred - det;
    const double part = w * diff;
    return det + part;
}

// step 3: track `r` with its prediction (xp, yp) takes detection d
FLEET_TRACK_FN void track_update(const TrackParams& P, TrackRow& r, double xp, double yp, const TrackDet& d)
{
    r.f[TRK_X] = track_blend(d.x, P.w_pos, xp); r.f[TRK_Y] = track_blend(d.y, P.w_pos, yp);
    r.f[TRK_EX] = track_blend(d.ex, P.w_vel, r.f[TRK_EX]); r.f[TRK_EY] = track_blend(d.ey, P.w_vel, r.f[TRK_EY]);
    r.f[TRK_V] = track_blend(d.v, P.w_vel, r.f[TRK_V]);
    r.f[TRK_R] = d.r; r.f[TRK_HITS] += 1.0; r.f[TRK_MISS] = 0.0;
}
// step 4: 0 the track coasts on (row updated), 1 deleted as tentative, 2 deleted after n_coast misses
FLEET_TRACK_FN int track_miss(const TrackParams& P, TrackRow& r, double xp, double yp)
{
    if (r.f[TRK_HITS] < P.n_confirm) return 1;
    r.f[TRK_MISS] += 1.0;
    if (r.f[TRK_MISS] > P.n_coast) return 2;
    r.f[TRK_X] = xp; r.f[TRK_Y] = yp;
    return 0;
}
// step 5
FLEET_TRACK_FN TrackRow track_born(const TrackDet& d, double id, double tick)
{
    return TrackRow{{d.x, d.y, d.ex, d.ey, d.r, d.v, id, 1.0, 0.0, tick}};
}
FLEET_TRACK_FN bool track_confirmed(const TrackParams& P, const TrackRow& r) { return r.f[TRK_HITS] >= P.n_confirm; }
// a track that reaches n_confirm in this tick (behind its update or its birth)
FLEET_TRACK_FN bool track_confirmed_now(const TrackParams& P, const TrackRow& r) { return r.f[TRK_HITS] == P.n_confirm; }
// step 7: out[6] = g_x, g_y, g_px, g_py, g_r, g_v
FLEET_TRACK_FN void track_out(const TrackRow& r, double* out)
{
    out[0] = r.f[TRK_X]; out[1] = r.f[TRK_Y]; out[2] = r.f[TRK_X] + r.f[TRK_EX]; out[3] = r.f[TRK_Y] + r.f[TRK_EY]; out[4] = r.f[TRK_R];
    out[5] = r.f[TRK_V];
}

// One tick in serial form. trk: [cap] rows, *n_trk of them in use; det: [K], K <= kTrackCap; out: [slots][6]; assign: [K] the id of the
// matched track, kTrackUnmatched (a track was born from it) or kTrackOverflow; rec: [TRS_DOUBLES], accumulated. Host only
inline void track_step(const TrackParams& P, double adv, double tick, int cap, int slots, TrackRow* trk, int* n_trk, double* next_id,
                               const TrackDet* det, int K, double* out, int* n_out, int* assign, double* rec)
{
    const int T = *n_trk;
    double xp[kTrackCap], yp[kTrackCap];
    int tm[kTrackCap], dm[kTrackCap];
    for (int t = 0; t < T; ++t) {
        xp[t] = track_predict(trk[t].f[TRK_X], adv, trk[t].f[TRK_EX]); yp[t] = track_predict(trk[t].f[TRK_Y], adv, trk[t].f[TRK_EY]);
        tm[t] = -1;
    }
    for (int k = 0; k < K; ++k) dm[k] = -1;
    const double g2 = track_gate2(P.gate);
    int n_matched = 0;
    for (;;) {
        double bd = 0.0; int bt = -1, bk = -1;
        for (int t = 0; t < T; ++t) {
            if (tm[t] >= 0) continue;
            for (int k = 0; k < K; ++k) {
                if (dm[k] >= 0) continue;
                const double d2 = track_d2(det[k].x, det[k].y, xp[t], yp[t]);
                if (track_gated(d2, g2) && (bt < 0 || d2 < bd)) { bd = d2; bt = t; bk = k; }
            }
        }
        if (bt < 0) break;
        tm[bt] = bk; dm[bk] = bt; ++n_matched;
    }
    // steps 3, 4 and 6: the survivors in place
    char live[kTrackCap];                  // of the NEW table: 1 matched or born this tick, 0 coasting
    int n = 0, del_tent = 0, del_coast = 0, confirmed = 0;
    for (int t = 0; t < T; ++t) {
        TrackRow r = trk[t];
        if (tm[t] >= 0) {
            track_update(P, r, xp[t], yp[t], det[tm[t]]);
            assign[tm[t]] = (int)r.f[TRK_ID];
            if (track_confirmed_now(P, r)) ++confirmed;
            live[n] = 1; trk[n++] = r;
        } else {
            const int gone = track_miss(P, r, xp[t], yp[t]);
            if (gone == 1) ++del_tent;
            else if (gone == 2) ++del_coast;
            else { live[n] = 0; trk[n++] = r; }
        }
    }
    int born = 0, overflow = 0;
    for (int k = 0; k < K; ++k) {
        if (dm[k] >= 0) continue;
        if (n < cap) {
            const TrackRow r = track_born(det[k], *next_id, tick);
            *next_id += 1.0;
            if (track_confirmed_now(P, r)) ++confirmed;
            live[n] = 1; trk[n++] = r; ++born;
            assign[k] = kTrackUnmatched;
        } else {
            ++overflow;
            assign[k] = kTrackOverflow;
        }
    }
    *n_trk = n;
    int m = 0, out_coast = 0, withheld = 0;
    for (int t = 0; t < n; ++t)
        if (live[t] && track_confirmed(P, trk[t])) track_out(trk[t], out + 6 * (m++));
    for (int t = 0; t < n; ++t)
        if (!live[t]) {                    // (a coasting track is a confirmed one)
            if (m < slots) { track_out(trk[t], out + 6 * (m++)); ++out_coast; }
            else ++withheld;
        }
    *n_out = m;
    rec[TRS_TICKS] += 1.0; rec[TRS_N_DET] += (double)K; rec[TRS_N_MATCHED] += (double)n_matched; rec[TRS_N_BORN] += (double)born;
    rec[TRS_N_CONFIRMED] += (double)confirmed; rec[TRS_N_DEL_TENT] += (double)del_tent; rec[TRS_N_DEL_COAST] += (double)del_coast;
    rec[TRS_N_OUT] += (double)m; rec[TRS_N_OUT_COAST] += (double)out_coast; rec[TRS_N_WITHHELD] += (double)withheld;
    rec[TRS_N_OVERFLOW] += (double)overflow;
    if ((double)n > rec[TRS_TRACKS_MAX]) rec[TRS_TRACKS_MAX] = (double)n;
}

}  // namespace fleet
