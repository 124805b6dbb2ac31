"""Closed-loop SIMULATION rate of a fleet (ltpl_fleet_sim_*): N planners, each with its own eight C2-style race-line opponents (SURVEY.md
section 8d: s0_k = 250 + 280 k, vel_scale_k = 0.30 + 0.05 (k mod 4), here staggered by 10 m (p mod 16) per planner), run the example
driver's loop on the device for T ticks without host work per tick.   tools/sim_rate.py [--planners 32768] [--ticks 200] [--no-tape]
[--race-size K] [--friction-map] [--telemetry] [--record M [--record-depth D]] [--events] [--noise] [--vehicle] [--sensor [keep]] [--tracker] [--predictor [K[:MODE]]] [--selector] [--safety] [--react] [--stats [demand|series]] [--lib PATH]. Prints planner-ticks per second of sim_run (device time of the run) next to tape_run on the C2 tape (recorded inputs,
tools/fleet_rate.py). --race-size K > 1: races of K consecutive planners (ltpl_fleet_sim_race) that see one another, started 30 m apart
along the race line with its heading; K = 1 (default) is the run without races. --friction-map: the same fleet on the friction grid of
tests/golden/friction_grid.npz (ltpl_fleet_friction: rows evaluated on the device, grip factors 1.0 .. 0.7 over the planners) instead of
the constant tuple. --telemetry: race telemetry on (ltpl_fleet_sim_telemetry, contact radius 2.5: k_fleet_sim_tele every tick, k_fleet_sim_rank
with races); the records of the first planners are printed after the run. --record M: the flight recorder on for M planners spread evenly
over the fleet (ltpl_fleet_sim_record, ring depth D, default: the run's ticks: k_fleet_sim_rec_paths / k_fleet_sim_rec_vel every tick on the
unfused launch sequence -- compare with LTPL_FLEET_NO_FUSE=1 and the recorder off); the bytes per record and the last record's summary are
printed. --events: scripted events on (ltpl_fleet_sim_events): per planner one timed gg_scale event at a tick of its own and one opp_within
trigger on its first opponent (it slows down; the odd planners' threshold lies above the opponent's first distance, the even planners'
below it, and the opponent drives away: theirs never fires) with a chained "after" (it speeds up again): k_fleet_sim_triggers every tick,
k_fleet_sim_events_timed in the ticks that hold a timed event; the fired events are counted after the run. --noise: seeded sensor noise on
(ltpl_fleet_sim_noise) with all five sigmas set (pos 0.1 m, vel 0.2 m/s, obj_pos 0.3 m, obj_theta 0.02 rad, obj_vel 0.5 m/s) and a seed per
planner: k_fleet_sim_step_noise (and k_fleet_sim_mates_noise with races) in place of the plain kernels; the largest distance between
estimate and true pose is printed after the run. --vehicle: every planner drives the vehicle model (ltpl_fleet_sim_vehicle,
sim.VEHICLE_DEFAULTS: k_fleet_sim_step_veh, or k_fleet_sim_step_noise_veh with --noise, in place of the step kernel); without races the
planners are put into races of one, which hands the start heading to the simulation; the tracking statistics are printed after the run.
--sensor: every planner behind the sensor model (ltpl_fleet_sim_sensor) with all four tests active -- range 300 m, a cone of 240 degrees, a
near field of 5 m, occlusion with the radius doubled, dropout 0.1, a seed per planner: k_fleet_sim_sense in front of k_fleet_sim_offsets;
like --vehicle it puts the planners into races of one for the start heading; the planner then sees fewer objects, so the rate holds the
sensor's kernel AND the changed planning work; the statistics are printed after the run. --sensor keep: every test evaluated and nothing
lost (range 10^6 m, a cone of 359.999 degrees, occlusion with the radius times 10^-6, dropout 10^-12): the planning work of the run without
a sensor plus the kernel.
--tracker: every planner behind the object tracker (ltpl_fleet_sim_tracker, sim.TRACKER_DEFAULTS: gate 5 m, weights 0.5, confirmed by the
second detection, coasted on for 3 ticks): k_fleet_sim_track in front of k_fleet_sim_offsets, behind k_fleet_sim_sense with --sensor (the
tracker then bridges the sensor's dropouts: the planner sees more objects than behind the sensor alone); the statistics are printed after
the run.
--predictor [K[:MODE]]: every planner behind the prediction model (ltpl_fleet_sim_predictor): K points per object (default 4) over 2 s in
mode MODE (default 2, along the track, relax 0.5; 0: as ingested -- the planning work of the run without a predictor on 1 + K positions
per object; 1: straight line): k_fleet_sim_predict in k_fleet_sim_compact's place, behind --sensor / --tracker when they are set; the
statistics are printed after the run.
--selector: every planner behind the behaviour selector (ltpl_fleet_sim_selector, sim.SELECTOR_DEFAULTS) on its four-entry list:
k_fleet_sim_select at the head of every tick, in front of the step kernel; the statistics are printed after the run.
--safety: every planner behind the safety monitor (ltpl_fleet_sim_safety, sim.SAFETY_DEFAULTS): k_fleet_sim_safety behind telemetry and
in front of the sensor in every tick; the first planners' records and the fleet's totals are printed after the run.
--react: the opponents of every planner react to the car ahead (ltpl_fleet_sim_react, sim.REACT_DEFAULTS): k_fleet_sim_react at the head of
every tick, in front of the step kernel; the fleet's totals and the first planners' records and scales are printed after the run.
--stats [demand|series]: a statistics plan (ltpl_fleet_sim_stats) of 12 measures over the modules that are on (the planners' failed flag
fills up) and 64 groups of planners p mod 64, lists of 8; 'demand' sets no series (nothing is launched in the tick), 'series' reduces
every 10th tick into a ring (k_fleet_sim_stats_chunk / k_fleet_sim_stats_merge at the tail of those ticks). After the last run one
sim_stats_reduce with 1 and with 64 groups is timed next to the _read calls of the families the plan uses plus the numpy mirror
(sim.StatsModel) on what they returned, and the two results are compared bit for bit.
--lib PATH: another build of
the library (A/B against the parent's)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                                            # noqa: E402
import planner_replay as pr                                                   # noqa: E402
from graphbasedlocaltrajectoryplanner_amd import _capi                        # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet                  # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.lattice import Lattice              # noqa: E402
from graphbasedlocaltrajectoryplanner_amd import sim                          # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.sim import Event, RaceLineTable     # noqa: E402


STATS_CANDIDATES = (("telemetry", "clear_min", 0.0, 40.0, 16, -1), ("telemetry", "dist", 0.0, 400.0, 16, 1), ("telemetry", "vel_max", 0.0, 60.0, 12, 1),
                    ("safety", "gap_min", -5.0, 35.0, 16, -1), ("safety", "ttc_min", 0.0, 16.0, 16, -1), ("safety", "drac_max", 0.0, 8.0, 8, 1),
                    ("vehicle", "e_max", 0.0, 2.0, 16, 1), ("vehicle", "dv_max", 0.0, 8.0, 8, 1), ("react", "gap_min", -5.0, 155.0, 16, -1),
                    ("react", "acc_min", -9.0, 3.0, 12, -1), ("sensor", "blind_clear_min", 0.0, 40.0, 8, -1), ("tracker", "tracks_max", 0.0, 16.0, 16, 1),
                    ("predictor", "d_abs_max", 0.0, 8.0, 8, 1), ("selector", "clear_min", 0.0, 40.0, 8, -1), ("state", "failed", 0.0, 2.0, 2, 1))


def stats_measures(a):
    """12 measures over the families whose module is on (the state family fills up)."""
    on = dict(telemetry=a.telemetry, safety=a.safety, vehicle=a.vehicle, react=a.react, sensor=bool(a.sensor), tracker=a.tracker,
              predictor=bool(a.predictor), selector=a.selector, state=True)
    fams = [f for f in sim.STATS_FAMILIES[:-1] if on[f]]
    m = []
    for turn in range(3):                   # every family's first field, then the second ones, ...
        m += [[c for c in STATS_CANDIDATES if c[0] == f][turn] for f in fams if len([c for c in STATS_CANDIDATES if c[0] == f]) > turn]
    m = m[:11]
    return m + [STATS_CANDIDATES[-1]] * (12 - len(m))


def stats_report(fleet, a, measures):
    """After the run: the series the run left, then one ltpl_fleet_sim_stats_reduce with 1 and with 64 groups next to reading every
    record of the modules that are on and reducing it with the numpy mirror (sim.StatsModel), best of three each."""
    n = fleet.n_scen
    if a.stats == "series":
        t, rows, total = fleet.sim_stats_series()
        d = sim.stats_dict(rows)
        print("  stats series: %d rows (ticks %d .. %d), %d written; measure 0 (%s %s) of group 0: n %s min %s" % (
            len(t), t[0] if len(t) else -1, t[-1] if len(t) else -1, total, measures[0][0], measures[0][1],
            d["n"][::5, 0, 0].tolist(), np.round(d["min"][::5, 0, 0], 3).tolist()))
    reads = dict(telemetry=lambda: stats_tele_rows(fleet), safety=lambda: fleet.sim_safety_read(raw=True)[0], vehicle=lambda: fleet.sim_vehicle_read(raw=True),
                 react=lambda: fleet.sim_react_read(raw=True)[0], sensor=lambda: fleet.sim_sensor_read(raw=True), tracker=lambda: fleet.sim_tracker_read(raw=True),
                 predictor=lambda: fleet.sim_predictor_read(raw=True), selector=lambda: fleet.sim_selector_read(raw=True)[0])
    fams = sorted(set(m[0] for m in measures) - {"state"})
    for G in (1, 64):
        groups = np.arange(n) % G
        fleet.sim_stats(groups, measures, top_k=8)
        t_dev, t_read, t_host = [], [], []
        for _ in range(3):
            t0 = time.perf_counter()
            rows, tops = fleet.sim_stats_reduce()
            t_dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            rec = {f: reads[f]() for f in fams}
            failed = fleet.digest()[:, 0] != 0
            t_read.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            want = sim.StatsModel(groups, measures, top_k=8).reduce(rec, failed)
            t_host.append(time.perf_counter() - t0)
        same = np.array_equal(rows.view(np.uint64), want[0].view(np.uint64)) and np.array_equal(tops.view(np.uint64), want[1].view(np.uint64))
        doubles = sum(sim.STATS_FAMILY_DOUBLES[f] for f in fams)
        print("  stats reduce, %d planners, G = %d, M = %d: sim_stats_reduce %.3f ms (wall, with its synchronisation and the copy of %d rows); the %d _read "
              "calls (%d doubles per planner) + digest %.3f ms, the numpy mirror on them %.1f ms; rows and lists %s" % (
                  n, G, len(measures), min(t_dev) * 1e3, G * len(measures), len(fams), doubles, min(t_read) * 1e3, min(t_host) * 1e3,
                  "bit-identical" if same else "DIFFER"))


def stats_tele_rows(fleet):
    import ctypes
    out, length = np.zeros((fleet.n_scen, sim.TELEMETRY_DOUBLES)), ctypes.c_double(0.0)
    fleet._check(fleet._fn("sim_telemetry_read")(fleet.handle, out.ctypes.data, sim.TELEMETRY_DOUBLES, ctypes.byref(length)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planners", type=int, default=32768)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-tape", action="store_true", help="skip the tape_run comparison on the C2 recording")
    ap.add_argument("--race-size", type=int, default=1, help="planners per race (1: no races)")
    ap.add_argument("--friction-map", action="store_true", help="every planner on the friction grid, own grip factor")
    ap.add_argument("--telemetry", action="store_true", help="race telemetry on (radius 2.5); prints the first planners' records")
    ap.add_argument("--record", type=int, default=0, help="flight recorder on for this many planners, spread evenly over the fleet")
    ap.add_argument("--record-depth", type=int, default=0, help="ring depth of the recorder (default: --ticks)")
    ap.add_argument("--events", action="store_true", help="scripted events on: a timed gg_scale event and an opp_within trigger with a chained after per planner")
    ap.add_argument("--noise", action="store_true", help="seeded sensor noise on, all five sigmas set, a seed per planner")
    ap.add_argument("--vehicle", action="store_true", help="every planner drives the vehicle model (sim.VEHICLE_DEFAULTS) instead of the ideal tracker")
    ap.add_argument("--sensor", nargs="?", const="lossy", default=None, choices=("lossy", "keep"),
                    help="every planner behind the sensor model: range, cone, near field, occlusion and dropout all active; 'keep': all evaluated, nothing lost")
    ap.add_argument("--tracker", action="store_true", help="every planner behind the object tracker (sim.TRACKER_DEFAULTS)")
    ap.add_argument("--predictor", nargs="?", const="4:2", default=None, metavar="K[:MODE]",
                    help="every planner behind the prediction model: K points per object over 2 s, mode 0 / 1 / 2 (default 4:2)")
    ap.add_argument("--selector", action="store_true", help="every planner behind the behaviour selector (sim.SELECTOR_DEFAULTS)")
    ap.add_argument("--safety", action="store_true", help="every planner behind the safety monitor (sim.SAFETY_DEFAULTS)")
    ap.add_argument("--react", action="store_true", help="the opponents of every planner react to the car ahead (sim.REACT_DEFAULTS)")
    ap.add_argument("--stats", nargs="?", const="demand", default=None, choices=("demand", "series"),
                    help="a statistics plan over the modules that are on: 12 measures, 64 groups; 'demand': no series, 'series': period 10")
    ap.add_argument("--lib", default=None, help="path of the library to load (default: the in-tree build)")
    a = ap.parse_args()
    lat = Lattice.load(os.path.join(ROOT, "tests", "golden", "monteblanco_lattice.npz"))
    race = RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))
    hip = _capi.HipBackend(lat, lib_path=a.lib) if a.lib else _capi.HipBackend(lat)
    grid = None
    if a.friction_map:
        from graphbasedlocaltrajectoryplanner_amd.friction import FrictionGrid
        grid = FrictionGrid.load(os.path.join(ROOT, "tests", "golden", "friction_grid.npz"))
    ticks = pr.load_ticks("c2")
    st, va = ticks[0]['start'], ticks[0]['vel_args']
    zones = pr.zone_gids_of_tick(lat, ticks[0])
    n = a.planners
    entries = [dict(opponents=[(250.0 + 280.0 * k + 10.0 * (p % 16), 0.30 + 0.05 * (k % 4), 5.0) for k in range(8)],
                    pref=("right", "left", "straight", "follow"), pos_est=st['pos'], vel_est=0.0, zone_gids=zones) for p in range(n)]
    K = a.race_size
    if K > 1:
        # slot i of a race starts 30 m ahead of slot i - 1 on the race line, with the race line's heading
        s0 = race.s_rl[int(np.argmin(np.hypot(race.x - st['pos'][0], race.y - st['pos'][1])))]
        slots = [int(np.argmin(np.abs(race.s_rl - (s0 + 30.0 * i)))) for i in range(K)]
        slot_pose = [((race.x[i], race.y[i]), race.psi[i] - 2 * np.pi if race.psi[i] > np.pi else race.psi[i]) for i in slots]
        for p in range(n):
            entries[p]['pos_est'] = slot_pose[p % K][0]
        sizes = [K] * (n // K) + ([n % K] if n % K else [])
    best = None
    for rep in range(a.reps):
        fleet = Fleet(hip, n)
        if K > 1:
            for p in range(n):
                pos, h = slot_pose[p % K]
                fleet.set_start(p, pos, h, st['vel'], st['max_heading_offset'])
        else:
            fleet.set_start_range(0, n, st['pos'], st['heading'], st['vel'], st['max_heading_offset'])
        fleet.sim_setup(race, entries)
        if K > 1:
            fleet.sim_race(sizes)
        elif a.vehicle or a.sensor:
            fleet.sim_race([1] * n)
        if grid is not None:
            fleet.friction(grid, scale=1.0 - 0.3 * (np.arange(n) % 16) / 15.0)
        fleet.sim_vel(vel_max=va['vel_max'], gg_scale=va['gg_scale'], local_gg=tuple(va['local_gg']), safety_d=va['safety_d'],
                      ax_max_machines=va['ax_max_machines'])
        if a.telemetry:
            fleet.sim_telemetry(radius=2.5)
        if a.record:
            fleet.sim_record([int(q) for q in np.linspace(0, n - 1, a.record).round()] if a.record > 1 else [0], a.record_depth or a.ticks)
        if a.events:
            ev = []
            for p in range(n):
                ev += [Event(p, when=("tick", (37 * p) % a.ticks), set=("gg_scale", 0.9 - 0.2 * (p % 8) / 7.0)),
                       Event(p, when=("opp_within", 0, 250.0 + 10.0 * (p % 16) + (5.0 if p % 2 else -20.0)), set=("opp_vel_scale", 0, 0.2)),
                       Event(p, when=("after", 1, 40), set=("opp_vel_scale", 0, 0.5))]
            fleet.sim_events(ev)
        if a.noise:
            fleet.sim_noise(seed=np.arange(n, dtype=np.uint64) + np.uint64(1), pos=0.1, vel=0.2, obj_pos=0.3, obj_theta=0.02, obj_vel=0.5)
        if a.vehicle:
            fleet.sim_vehicle(model=1)
        if a.sensor:
            par = dict(range=300.0, fov_deg=240.0, r_near=5.0, occl=2.0, p_drop=0.1) if a.sensor == "lossy" else \
                dict(range=1e6, fov_deg=359.999, r_near=0.0, occl=1e-6, p_drop=1e-12)
            fleet.sim_sensor(seed=np.arange(n, dtype=np.uint64) + np.uint64(1), **par)
        if a.tracker:
            fleet.sim_tracker()
        if a.predictor:
            kp, _, mode = a.predictor.partition(":")
            fleet.sim_predictor(n_points=int(kp), mode=int(mode or 2), horizon=2.0, relax=0.5)
        if a.selector:
            fleet.sim_selector()
        if a.safety:
            fleet.sim_safety()
        if a.react:
            fleet.sim_react()
        if a.stats:
            measures = stats_measures(a)
            fleet.sim_stats(np.arange(n) % 64, measures, top_k=8, period=10 if a.stats == "series" else 0, depth=a.ticks // 10 + 1)
        t0 = time.perf_counter()
        failed = 0
        try:
            _, ms = fleet.sim_run(a.ticks, trace=False)
        except _capi.BackendError as e:
            ms = fleet.last_ms
            failed = int(np.count_nonzero(fleet.digest()[:, 0]))
            print("  (%d planners stopped with an error: %s)" % (failed, str(e)[:160]))
        wall = time.perf_counter() - t0
        best = ms if best is None else min(best, ms)
        print("rep %d: sim_run %d planners (races of %d) x %d ticks: device %.1f ms (wall %.1f ms) = %.3f M planner-ticks/s; %.3f ms per tick of the fleet" % (
            rep, n, K, a.ticks, ms, wall * 1e3, n * a.ticks / ms / 1e3, ms / a.ticks))
        if failed == 0:
            sel = np.bincount(fleet.sim_state()['sel_action'] + 1, minlength=6)
            print("  last selected actions (none, straight, follow, left, right, emergency): %s" % sel.tolist())
        if a.noise:
            est, tru = fleet.sim_estimate(), fleet.sim_state()
            print("  noise: estimate up to %.3f m and %.3f m/s off the true state in the last tick" % (
                np.max(np.hypot(*(est["pos_est"] - tru["pos_est"]).T)), np.max(np.abs(est["vel_est"] - tru["vel_est"]))))
        if a.vehicle:
            d = fleet.sim_vehicle_read()
            print("  vehicle: e_max up to %.3f m, rms e up to %.3f m, dv_max up to %.2f m/s, %d lateral and %d longitudinal saturations in %d control "
                  "steps, %d planners left the track" % (np.max(d["e_max"]), np.sqrt(np.max(d["e2_sum"] / np.maximum(d["ctl_steps"], 1))), np.max(d["dv_max"]),
                                                         d["sat_lat"].sum(), d["sat_lon"].sum(), d["ctl_steps"].sum(), np.count_nonzero(d["off_track_ticks"])))
        if a.sensor:
            d = fleet.sim_sensor_read()
            print("  sensor: %d of %d objects seen; lost to range %d, cone %d, occlusion %d, dropout %d; %d planner-ticks with a lost object, smallest "
                  "blind clearance %.3f m" % (d["n_seen"].sum(), d["n_obj"].sum(), d["n_range"].sum(), d["n_fov"].sum(), d["n_occl"].sum(), d["n_drop"].sum(),
                                             d["blind_ticks"].sum(), np.min(d["blind_clear_min"])))
        if a.tracker:
            d = fleet.sim_tracker_read()
            print("  tracker: %d detections, %d matched, %d tracks born, %d confirmed, %d tentative and %d coasted tracks deleted; %d objects handed on, "
                  "%d of them coasting, %d withheld, %d overflows, up to %d tracks" % (
                      d["n_det"].sum(), d["n_matched"].sum(), d["n_born"].sum(), d["n_confirmed"].sum(), d["n_del_tentative"].sum(), d["n_del_coast"].sum(),
                      d["n_out"].sum(), d["n_out_coast"].sum(), d["n_withheld"].sum(), d["n_overflow"].sum(), d["tracks_max"].max()))
        if a.safety:
            d, ring = fleet.sim_safety_read()
            print("  safety: %d live ticks, %d evaluated; %d incidents in %d planners, %.1f s under the TTC threshold, %d ticks over the DRAC "
                  "threshold, %d under the headway threshold, %d overlap ticks, %d objects skipped; smallest gap %.3f m, smallest TTC %.3f s, "
                  "largest DRAC %.3f m/s^2, largest impact speed %.3f m/s" % (
                      d["ticks"].sum(), d["ticks_eval"].sum(), d["n_incidents"].sum(), np.sum(d["n_incidents"] > 0), d["tet"].sum(),
                      d["drac_ticks"].sum(), d["thw_ticks"].sum(), d["overlap_ticks"].sum(), d["n_skipped"].sum(), np.min(d["gap_min"]),
                      np.min(d["ttc_min"]), np.max(d["drac_max"]), np.max(d["impact_max"])))
            for p in range(min(3, fleet.n_scen)):
                print("    planner %d: gap_min %.3f m (tick %d, slot %d), ttc_min %.3f s (tick %d, slot %d), tet %.2f s, tit %.3f s^2, drac_max "
                      "%.3f, thw_min %.3f s, hist %s, incidents %s" % (
                          p, d["gap_min"][p], d["gap_tick"][p], d["gap_slot"][p], d["ttc_min"][p], d["ttc_tick"][p], d["ttc_slot"][p], d["tet"][p],
                          d["tit"][p], d["drac_max"][p], d["thw_min"][p], d["hist"][p].tolist(),
                          [(int(i["tick_first"]), int(i["tick_last"]), round(i["ttc_min"], 3)) for i in sim.safety_incidents(ring[p], d["n_incidents"][p])]))
        if a.react:
            d, eff = fleet.sim_react_read()
            print("  react: %d ticks, %d opponent-ticks: %d with a leader (%d behind the ego), %d clamped at -b_max, %d overlapping, %d passive; "
                  "smallest gap %.3f m, smallest acc %.3f m/s^2, smallest gap behind an ego %.3f m; %d ticks with the ego outside the gate" % (
                      d["ticks"].sum(), d["opp_ticks"].sum(), d["follow_ticks"].sum(), d["ego_lead_ticks"].sum(), d["clamped"].sum(),
                      d["overlaps"].sum(), d["passive"].sum(), np.min(d["gap_min"]), np.min(d["acc_min"]), np.min(d["ego_gap_min"]),
                      d["ego_outside"].sum()))
            no = eff.size // max(fleet.n_scen, 1)
            for p in range(min(3, fleet.n_scen)):
                print("    planner %d: follow_ticks %d, ego_lead_ticks %d, gap_min %.3f m (tick %d, opponent %d), acc_min %.3f (tick %d, opponent %d), "
                      "effective scales %s" % (p, d["follow_ticks"][p], d["ego_lead_ticks"][p], d["gap_min"][p], d["gap_tick"][p], d["gap_slot"][p],
                                               d["acc_min"][p], d["acc_tick"][p], d["acc_slot"][p], np.round(eff[p * no:(p + 1) * no], 4).tolist()))
        if a.stats and rep == a.reps - 1:
            stats_report(fleet, a, measures)
        if a.selector:
            d = fleet.sim_selector_read()[0]
            print("  selector: %d evaluations, %d actions scored; %d switches, %d overrides of the list, %d without a safe action, %d emergency; chosen "
                  "straight %d, follow %d, left %d, right %d; smallest clearance taken %.3f m" % (
                      d["ticks"].sum(), d["n_scored"].sum(), d["n_switch"].sum(), d["n_override"].sum(), d["n_unsafe"].sum(), d["n_emergency"].sum(),
                      d["chosen_straight"].sum(), d["chosen_follow"].sum(), d["chosen_left"].sum(), d["chosen_right"].sum(), np.min(d["clear_min"])))
        if a.predictor:
            d = fleet.sim_predictor_read()
            print("  predictor: %d objects predicted; as ingested %d, still %d, straight by mode %d / d_max %d / direction %d / no segment %d, along the "
                  "track %d; largest offset %.3f m, %d points wrapped" % (
                      d["n_obj"].sum(), d["n_ingested"].sum(), d["n_still"].sum(), d["n_straight_mode"].sum(), d["n_straight_dmax"].sum(),
                      d["n_straight_dir"].sum(), d["n_straight_noseg"].sum(), d["n_track"].sum(), np.max(d["d_abs_max"]), d["n_wrap"].sum()))
        if a.events:
            ft = fleet.sim_events_read()["fired_tick"].reshape(n, 3)
            print("  events: %d timed, %d opp_within and %d chained 'after' events fired of %d each (schedule tick %d)" % (
                np.count_nonzero(ft[:, 0] >= 0), np.count_nonzero(ft[:, 1] >= 0), np.count_nonzero(ft[:, 2] >= 0), n, fleet.sim_events_read()["tick"]))
        if a.record and rep == a.reps - 1:
            info = fleet.sim_record_info()
            t1 = time.perf_counter()
            last = fleet.sim_record_read(first=info["first_tick"] + info["n_ticks"] - 1, count=1)[0]
            rec_doubles = 64 + 6 * 96 + 2 * fleet.cap_rows + 7 * _capi.PLANNER_MAX_KEYS * fleet._sim_export + _capi.PLANNER_MAX_KEYS * fleet.cap_nodes
            print("  recorder: %d planners, ticks %d .. %d held, %d bytes per record (cap_rows %d, cap_nodes %d), ring copy + one tick read %.1f ms" % (
                info["n_planners"], info["first_tick"], info["first_tick"] + info["n_ticks"] - 1, (rec_doubles + 31) // 32 * 32 * 8, fleet.cap_rows,
                fleet.cap_nodes, (time.perf_counter() - t1) * 1e3))
            for r in last[:4]:
                print("    planner %d tick %d: sel %s, %d objects, paths %s (const_rows %d), trajectories %s" % (
                    r["planner"], r["tick"], r["sel"], len(r["vehicles"]), r["paths"]["keys"], r["paths"]["const_rows"],
                    {k: v[0].shape[0] for k, v in r["traj"][0].items()}))
        if a.telemetry and rep == a.reps - 1:
            d = fleet.sim_telemetry_read()
            print("  telemetry (track length %.3f m), planners 0 .. %d:" % (d["track_length"], min(n, max(K, 4)) - 1))
            for p in range(min(n, max(K, 4))):
                print("    %d: ticks %d s %.2f dist %.2f laps %d vel mean %.2f max %.2f act %s clear_min %.3f (tick %d, slot %d) contact %d "
                      "rank %d passes %d passed %d gap %.2f" % (p, d["ticks"][p], d["s"][p], d["dist"][p], d["laps"][p],
                                                                d["vel_sum"][p] / max(d["ticks"][p], 1), d["vel_max"][p], d["act"][p].tolist(),
                                                                d["clear_min"][p], d["clear_tick"][p], d["clear_slot"][p], d["contact_ticks"][p],
                                                                d["rank"][p], d["passes"][p], d["passed"][p], d["gap_ahead"][p]))
        fleet.close()
    print("closed_loop_sim_ticks_per_s %.0f" % (n * a.ticks / best * 1e3))
    if a.no_tape or grid is not None:
        return
    fleet = Fleet(hip, n)
    for k in range(a.ticks):
        t, v = ticks[k], ticks[k]['vel_args']
        fleet.tape_append_groups([(n, dict(prev_action=t['action_id_sel'], t_now=t['t'], vehicles=pr.vehicles_of_tick(t), zone_gids=zones,
                                           pos_est=t['pos_est'], vel_est=v['vel_est'], vel_max=v['vel_max'], gg_scale=v['gg_scale'],
                                           local_gg=tuple(v['local_gg']), safety_d=v['safety_d'], incl_emerg_traj=v['incl_emerg_traj']))],
                                 ax_max_machines=v['ax_max_machines'])
    fleet.set_start_range(0, n, st['pos'], st['heading'], st['vel'], st['max_heading_offset'])
    ms = fleet.tape_run(0, a.ticks)
    print("tape_run (C2 recording) %d planners x %d ticks: device %.1f ms = %.3f M planner-ticks/s" % (n, a.ticks, ms, n * a.ticks / ms / 1e3))
    print("closed_loop_device_ticks_per_s %.0f" % (n * a.ticks / ms * 1e3))


if __name__ == "__main__":
    main()
