"""
GPU: races of the fleet's closed-loop simulation (ltpl_fleet_sim_race, csrc/fleet_sim.hpp k_fleet_sim_mates) -- planners of one fleet that
see one another -- against the race recordings of the unmodified reference (tools/gen_golden_race.py: several Graph_LTPL instances in
lockstep, every car's object list holding its dummies and then the other cars at their tracked pose and heading). Every tick of every car
is checked from the run's trace like tests/test_gpu_fleet_sim.py does: selected action, clock and on-track count (mates included) exactly,
a dummy as the first vehicle to 1e-12 m and a mate to 1e-6 m, the pose to 1e-6 m, vel_est to 1e-5 relative, the digest row; the heading
of every car to 1e-6 rad after every run (runs of at most 25 ticks, so that race4's headings are checked on both sides of the +-pi wrap).
"""
import json
import os

import numpy as np
import pytest

import planner_replay as pr
from test_gpu_fleet_sim import planner_entry, segments, set_vel, start

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "race_scenarios.json")) as fh:
    SCEN = json.load(fh)


@pytest.fixture(scope="module")
def hip(monteblanco):
    from graphbasedlocaltrajectoryplanner_amd import _capi
    return _capi.HipBackend(monteblanco)


@pytest.fixture(scope="module")
def race():
    from graphbasedlocaltrajectoryplanner_amd.sim import RaceLineTable
    return RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


@pytest.fixture(scope="module")
def cars():
    return {name: [pr.load_ticks("%s_car%d" % (name, k)) for k in range(len(s["cars"]))] for name, s in SCEN.items()}


def car_entry(name, k, pref=None):
    s = SCEN[name]
    c = s["cars"][k]
    return dict(opponents=[tuple(d) for d in s["dummies"]], pref=tuple(pref or c["pref"]), pos_est=tuple(c["pos"]), vel_est=c["v0"],
                zone_gids=[])


def check_trace(trace, ticks, rows, what, nd=None):
    """``check_trace`` of tests/test_gpu_fleet_sim.py with mates: ``nd`` = the recording's dummies (None: no mates in the recording)."""
    from graphbasedlocaltrajectoryplanner_amd.planner import KEY_IDS
    from graphbasedlocaltrajectoryplanner_amd.tick_replay import check_digests
    seen, mate_first = set(), 0
    for k in range(trace.shape[0]):
        t, tr = ticks[k], trace[k, rows]
        w = "%s tick %d" % (what, k)
        assert np.all(tr[:, 0] == KEY_IDS[t['action_id_sel']]), "%s: sel action %s vs %s" % (w, tr[:, 0], t['action_id_sel'])
        assert np.all(tr[:, 1] == t['t']), "%s: t_now" % w
        n_obj = len(t['obj_radius'])
        assert np.all(tr[:, 5] == n_obj), "%s: on-track vehicles %s vs %d" % (w, tr[:, 5], n_obj)
        if n_obj:
            first = np.asarray(t['obj_pos'][0], float)
            mate = nd is not None and not any(np.array_equal(row[:2], first) for row in t['obj_in'][:nd])
            mate_first += mate
            tol = 1e-6 if mate else 1e-12
            assert np.max(np.abs(tr[:, 6:8] - first)) <= tol, "%s: first vehicle %s vs %s (%s)" % (w, tr[0, 6:8], first, "mate" if mate else "dummy")
        assert np.max(np.abs(tr[:, 2:4] - np.asarray(t['pos_est'], float))) <= 1e-6, "%s: pos_est %s vs %s" % (w, tr[0, 2:4], t['pos_est'])
        ve = t['vel_args']['vel_est']
        assert np.max(np.abs(tr[:, 4] - ve)) <= 1e-5 * max(abs(ve), 1.0), "%s: vel_est %s vs %s" % (w, tr[:, 4], ve)
        check_digests(tr[:, 8:], t, KEY_IDS, w)
        seen.update(t['vel']['keys'])
    return seen, mate_first


def check_heading(fleet, ticks, rows, what):
    th = fleet.sim_heading()[rows]
    d = np.abs(np.mod(th - ticks['theta_est'] + np.pi, 2 * np.pi) - np.pi)
    assert np.all(d <= 1e-6), "%s: heading %s vs %s" % (what, th, ticks['theta_est'])


def race_fleet(hip, race, cars, layout):
    """``layout``: [(scenario name, copies)] in planner order, 'c2' = one planner replaying the c2 recording on its own. Returns the
    fleet, the recording of every planner and [(name, copy, car, planner)]."""
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    plan, recs, sizes, entries = [], [], [], []
    for name, copies in layout:
        for c in range(copies):
            if name == "c2":
                recs.append(cars["c2"])
                entries.append(("c2", None))
                plan.append(("c2", c, 0, len(recs) - 1))
                sizes.append(1)
                continue
            for k in range(len(SCEN[name]["cars"])):
                recs.append(cars[name][k])
                entries.append((name, k))
                plan.append((name, c, k, len(recs) - 1))
            sizes.append(len(SCEN[name]["cars"]))
    fleet = Fleet(hip, len(recs))
    for p, r in enumerate(recs):
        st = r[0]['start']
        assert fleet.set_start(p, st['pos'], st['heading'], st['vel'], st['max_heading_offset']) == (st['in_track'], st['cor_heading'])
    return fleet, recs, sizes, entries, plan


def run(fleet, recs, n_ticks, every=25):
    """The planners grouped by recording (the velocity arguments are per recording), runs split where they change and every ``every``
    ticks; after each run the heading of every planner of a race recording is checked against the recording's last tick of the run.
    Returns (trace, headings checked [n_runs, n_planners] (NaN: no race recording))."""
    uniq, idx = [], []
    for p, r in enumerate(recs):
        for u, q in zip(uniq, idx):
            if u is r:
                q.append(p)
                break
        else:
            uniq.append(r)
            idx.append([p])
    cuts = sorted(set([a for a, _ in segments(uniq, n_ticks)] + list(range(0, n_ticks, every)) + [n_ticks]))
    traces, seen = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        set_vel(fleet, uniq, idx, a)
        tr, ms = fleet.sim_run(b - a)
        assert ms > 0.0
        traces.append(tr)
        th = np.full(len(recs), np.nan)
        for r, q in zip(uniq, idx):
            if 'theta_est' in r[b - 1]:
                check_heading(fleet, r[b - 1], q, "ticks %d .. %d" % (a, b - 1))
                th[q] = r[b - 1]['theta_est']
        seen.append(th)
    return np.concatenate(traces), np.array(seen)


def setup(fleet, race, monteblanco, recs, sizes, entries):
    ent = [planner_entry(monteblanco, "c2", recs[p]) if name == "c2" else car_entry(name, k) for p, (name, k) in enumerate(entries)]
    fleet.sim_setup(race, ent)
    fleet.sim_race(sizes, length=5.0)


@pytest.mark.parametrize("name,copies", [("race4", 1), ("race3_mixed", 1), ("race4", 64)])   # 64 copies: 256 planners, one-wave batch kernel
def test_race_reproduces_every_car(hip, monteblanco, race, cars, name, copies):
    fleet, recs, sizes, entries, plan = race_fleet(hip, race, cars, [(name, copies)])
    setup(fleet, race, monteblanco, recs, sizes, entries)
    T = SCEN[name]["n_ticks"]
    trace, th = run(fleet, recs, T)
    assert trace.shape[:2] == (T, len(recs))
    nd = len(SCEN[name]["dummies"])
    seen, mates = set(), 0
    for k in range(len(SCEN[name]["cars"])):
        rows = [p for (_, c, kk, p) in plan if kk == k]
        s, m = check_trace(trace, cars[name][k], rows, "%s car %d" % (name, k), nd)
        seen |= s
        mates += m
        check_heading(fleet, cars[name][k][T - 1], rows, "%s car %d" % (name, k))
    if name == "race4":
        assert mates > 0                                                   # (no dummies: every first vehicle is a mate)
        assert "follow" in seen and seen & {"left", "right"}, seen
        # device headings checked on both sides of the +-pi wrap, and a car's heading crossing it between two checks
        assert np.any(th > 2.9) and np.any(th < -2.9), th
        assert np.any(np.abs(np.diff(th, axis=0)) > np.pi), th
    else:
        n_mates = sum(len(t['obj_radius']) - sum(1 for row in t['obj_in'][:nd] if any(np.array_equal(row[:2], q) for q in t['obj_pos']))
                      for ticks in cars[name] for t in ticks)
        assert n_mates > 0                                                 # mates on the lists next to the dummies
    fleet.close()


def test_races_next_to_single_planners_each_follow_their_own_recording(hip, monteblanco, race, cars):
    cars = dict(cars, c2=pr.load_ticks("c2"))
    fleet, recs, sizes, entries, plan = race_fleet(hip, race, cars, [("race4", 1), ("c2", 2), ("race3_mixed", 2), ("c2", 1), ("race4", 1)])
    setup(fleet, race, monteblanco, recs, sizes, entries)
    T = min(SCEN["race4"]["n_ticks"], SCEN["race3_mixed"]["n_ticks"])
    trace, _ = run(fleet, recs, T)
    assert trace.shape[:2] == (T, len(recs))
    for name in ("race4", "race3_mixed", "c2"):
        for k in range(1 if name == "c2" else len(SCEN[name]["cars"])):
            rows = [p for (nm, c, kk, p) in plan if nm == name and kk == k]
            ticks = cars[name] if name == "c2" else cars[name][k]
            check_trace(trace, ticks, rows, "mixed %s car %d" % (name, k), None if name == "c2" else len(SCEN[name]["dummies"]))
            if name != "c2":
                check_heading(fleet, ticks[T - 1], rows, "mixed %s car %d" % (name, k))
    fleet.close()


def test_races_of_size_one_change_nothing(hip, monteblanco, race):
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    ticks = pr.load_ticks("c2")
    out = []
    for races in (None, [1, 1, 1]):
        fleet = Fleet(hip, 3)
        start(fleet, [(ticks, range(3))])
        fleet.sim_setup(race, [planner_entry(monteblanco, "c2", ticks)] * 3)
        if races:
            fleet.sim_race(races)
        set_vel(fleet, [ticks], [range(3)], 0)
        out.append((fleet.sim_run(120)[0], fleet.digest()))
        fleet.close()
    assert np.array_equal(out[0][0], out[1][0], equal_nan=True) and np.array_equal(out[0][1], out[1][1])


def test_a_failed_car_stays_in_its_mates_list(hip, monteblanco, race, cars):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    r4 = cars["race4"]
    fleet = Fleet(hip, 2)
    start(fleet, [(r4[0], [0]), (r4[1], [1])])
    fleet.sim_setup(race, [car_entry("race4", 0, pref=("right", "left", "follow")), car_entry("race4", 1)])
    fleet.sim_race([2])
    set_vel(fleet, [r4[0], r4[1]], [[0], [1]], 0)
    with pytest.raises(BackendError, match="planner 0: closed-loop simulation"):
        fleet.sim_run(80)
    trace = fleet.last_trace
    assert np.all(trace[:, 0, 8] != 0)                                   # error word of the failed car from the first tick on
    p0 = np.asarray(SCEN["race4"]["cars"][0]["pos"], float)
    assert np.all(trace[:, 1, 5] == 1) and np.all(trace[:, 1, 6:8] == p0), trace[:3, 1, 5:8]
    assert np.all(trace[:, 1, 8] == 0)                                   # the mate runs on
    assert np.all(np.isnan(trace[:, 0, 6])) and np.all(trace[:, 0, 5] == 0)
    fleet.close()
