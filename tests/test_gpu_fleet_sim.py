"""
GPU: the fleet's closed-loop simulation (ltpl_fleet_sim_*, csrc/fleet_sim.hpp) -- the example driver's loop (opponents on the race line,
object ingestion, ideal ego tracker) around every planner on the device -- against the tick recordings of the unmodified reference. No
run takes per-tick host input: a run is split only where the recording's velocity arguments change, and the simulation state carries
across the split. Every tick of every planner is checked from the run's trace: selected action, clock and on-track count exactly, the
first vehicle's position to 1e-12 m, the ego's pose / speed estimate, and the tick's digest row against the recording.
"""
import os

import numpy as np
import pytest

import planner_replay as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_PREF = ("right", "left", "straight", "follow")
LEFT_FIRST = ("left", "right", "straight", "follow")
C2_OPP = [(250.0 + 280.0 * k, 0.30 + 0.05 * (k % 4), 5.0) for k in range(8)]
# recording -> (opponents (s0, vel_scale, length), preference, fleet config)
SPECS = {
    "c2": (C2_OPP, DEFAULT_PREF, {}),
    "car2": ([(140.0, 0.4, 5.0)], LEFT_FIRST, {}),
    "overtake": ([(120.0, 0.5, 5.0)], LEFT_FIRST, {}),
    "c1": ([], DEFAULT_PREF, {}),
    "filt5": ([(200.0, 0.4, 5.0)], DEFAULT_PREF, {"filt_window_width": 5}),
    "zonewall": ([(180.0, 0.15, 5.0)], DEFAULT_PREF, {}),
}
VEL_KEYS = ("vel_max", "gg_scale", "local_gg", "safety_d", "ax_max_machines", "incl_emerg_traj")


@pytest.fixture(scope="module")
def hip(monteblanco):
    from graphbasedlocaltrajectoryplanner_amd import _capi
    return _capi.HipBackend(monteblanco)


@pytest.fixture(scope="module")
def race():
    from graphbasedlocaltrajectoryplanner_amd.sim import RaceLineTable
    return RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


def planner_entry(lat, name, ticks, pref=None):
    opp, dpref, _ = SPECS[name]
    t0 = ticks[0]
    static = []
    if name == "c1":    # the static objects of the recording (v = 0: the prediction is the position whatever theta)
        static = [(float(t0['obj_pos'][k][0]), float(t0['obj_pos'][k][1]), 0.0, float(t0['obj_vel'][k]), 2.0 * float(t0['obj_radius'][k]))
                  for k in range(len(t0['obj_radius']))]
    st = t0['start']
    return dict(opponents=opp, static=static, pref=pref or dpref, pos_est=st['pos'], vel_est=0.0,
                zone_gids=pr.zone_gids_of_tick(lat, t0))


def start(fleet, groups):
    """``groups``: [(recording ticks, planner indices)] -- every planner gets its recording's start pose."""
    for ticks, idx in groups:
        st = ticks[0]['start']
        for p in idx:
            assert fleet.set_start(p, st['pos'], st['heading'], st['vel'], st['max_heading_offset']) == (st['in_track'], st['cor_heading'])


def vel_of(t):
    va = t['vel_args']
    return {k: (tuple(va[k]) if k == "local_gg" else va[k]) for k in VEL_KEYS}


def same_vel(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in VEL_KEYS)


def segments(recs, n_ticks):
    """Tick ranges over which the velocity arguments of every recording stay the same."""
    cuts = [0] + [k for k in range(1, n_ticks) if any(not same_vel(vel_of(r[k - 1]), vel_of(r[k])) for r in recs)] + [n_ticks]
    return list(zip(cuts[:-1], cuts[1:]))


def set_vel(fleet, recs, groups_idx, k):
    """Velocity arguments of tick k: per planner the values of its recording (machine table per planner)."""
    n = fleet.n_scen
    cols = {key: [None] * n for key in ("vel_max", "gg_scale", "safety_d", "incl_emerg_traj")}
    gx, gy, tab_idx, tables = [0.0] * n, [0.0] * n, [0] * n, []
    for r, idx in zip(recs, groups_idx):
        v = vel_of(r[k])
        tables.append(np.asarray(v["ax_max_machines"], float).reshape(-1, 2))
        for p in idx:
            for key in cols:
                cols[key][p] = v[key]
            gx[p], gy[p] = v["local_gg"]
            tab_idx[p] = len(tables) - 1
    cols["incl_emerg_traj"] = [bool(e) for e in cols["incl_emerg_traj"]]
    fleet.sim_vel(local_gg=[(gx[p], gy[p]) for p in range(n)], ax_tables=tables, ax_table_idx=tab_idx, **cols)


def run_split(fleet, recs, groups_idx, n_ticks):
    traces = []
    for a, b in segments(recs, n_ticks):
        set_vel(fleet, recs, groups_idx, a)
        tr, ms = fleet.sim_run(b - a)
        assert ms > 0.0
        traces.append(tr)
    return np.concatenate(traces)


def check_trace(trace, ticks, rows, what):
    from graphbasedlocaltrajectoryplanner_amd.planner import KEY_IDS
    from graphbasedlocaltrajectoryplanner_amd.tick_replay import check_digests
    seen = set()
    for k in range(trace.shape[0]):
        t, tr = ticks[k], trace[k, rows]
        w = "%s tick %d" % (what, k)
        assert np.all(tr[:, 0] == KEY_IDS[t['action_id_sel']]), "%s: sel action %s vs %s" % (w, tr[:, 0], t['action_id_sel'])
        assert np.all(tr[:, 1] == t['t']), "%s: t_now" % w
        n_obj = len(t['obj_radius'])
        assert np.all(tr[:, 5] == n_obj), "%s: on-track vehicles %s vs %d" % (w, tr[:, 5], n_obj)
        if n_obj:
            assert np.max(np.abs(tr[:, 6:8] - np.asarray(t['obj_pos'][0], float))) <= 1e-12, "%s: first vehicle %s vs %s" % (w, tr[0, 6:8], t['obj_pos'][0])
        assert np.max(np.abs(tr[:, 2:4] - np.asarray(t['pos_est'], float))) <= 1e-6, "%s: pos_est %s vs %s" % (w, tr[0, 2:4], t['pos_est'])
        ve = t['vel_args']['vel_est']
        assert np.max(np.abs(tr[:, 4] - ve)) <= 1e-5 * max(abs(ve), 1.0), "%s: vel_est %s vs %s" % (w, tr[:, 4], ve)
        check_digests(tr[:, 8:], t, KEY_IDS, w)
        seen.update(t['vel']['keys'])
    return seen


@pytest.mark.parametrize("name,n,must_see", [
    ("c2", 3, {"straight", "follow", "left", "right"}),
    ("car2", 1, {"follow", "emergency"}),
    ("overtake", 64, {"follow", "left", "right", "emergency"}),        # >= 64 planners: the one-wave batch path kernel
    ("c1", 1, {"straight", "follow"}),
    ("filt5", 1, {"follow", "right"}),
    ("zonewall", 2, {"straight", "follow"}),
])
def test_closed_loop_simulation_reproduces_the_recording(hip, monteblanco, race, name, n, must_see):
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    ticks = pr.load_ticks(name)
    fleet = Fleet(hip, n, **SPECS[name][2])
    start(fleet, [(ticks, range(n))])
    fleet.sim_setup(race, [planner_entry(monteblanco, name, ticks)] * n)
    segs = segments([ticks], len(ticks))
    if name == "c2":
        assert len(segs) == 1                           # the whole recording in ONE run
    trace = run_split(fleet, [ticks], [range(n)], len(ticks))
    seen = check_trace(trace, ticks, list(range(n)), name)
    assert must_see <= seen, seen
    # the fleet's own queries see the last tick like after a tape run
    traj, ids, ref = fleet.trajectories(n - 1)
    pr.check_trajectories(traj, ids, ref, ticks[-1], "%s last tick" % name)
    st = fleet.sim_state()
    assert np.all(st['now'] == ticks[-1]['t'])
    fleet.close()


def test_mixed_fleet_each_group_follows_its_own_recording(hip, monteblanco, race):
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    recs = [pr.load_ticks("c2"), pr.load_ticks("car2")]
    T = len(recs[1])
    idx = [[0, 2, 4], [1, 3]]
    fleet = Fleet(hip, 5)
    start(fleet, list(zip(recs, idx)))
    entries = [None] * 5
    for name, r, ix in zip(("c2", "car2"), recs, idx):
        for p in ix:
            entries[p] = planner_entry(monteblanco, name, r)
    fleet.sim_setup(race, entries)
    trace = run_split(fleet, recs, idx, T)
    check_trace(trace, recs[0], idx[0], "mixed c2")
    check_trace(trace, recs[1], idx[1], "mixed car2")
    fleet.close()


def test_one_tick_runs_equal_one_long_run(hip, monteblanco, race):
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    ticks = pr.load_ticks("c2")
    K = 60
    out = []
    for split in (False, True):
        fleet = Fleet(hip, 2)
        start(fleet, [(ticks, range(2))])
        fleet.sim_setup(race, [planner_entry(monteblanco, "c2", ticks)] * 2)
        set_vel(fleet, [ticks], [range(2)], 0)
        if split:
            trace = np.concatenate([fleet.sim_run(1)[0] for _ in range(K)])
        else:
            trace = fleet.sim_run(K)[0]
        out.append((trace, fleet.digest(), fleet.sim_state()))
        fleet.close()
    (ta, da, sa), (tb, db, sb) = out
    assert np.array_equal(ta, tb, equal_nan=True) and np.array_equal(da, db)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k


def test_a_planner_without_a_matching_action_fails_alone(hip, monteblanco, race):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    ticks = pr.load_ticks("c2")
    fleet = Fleet(hip, 3)
    start(fleet, [(ticks, range(3))])
    e = planner_entry(monteblanco, "c2", ticks)
    fleet.sim_setup(race, [e, dict(e, pref=("right",)), e])
    set_vel(fleet, [ticks], [range(3)], 0)
    with pytest.raises(BackendError, match="planner 1: closed-loop simulation"):
        fleet.sim_run(40)
    trace = fleet.last_trace
    assert np.all(trace[:, 1, 8] != 0)                                   # error word of planner 1 from tick 0 on
    check_trace(trace, ticks, [0, 2], "neighbours of the failing planner")
    fleet.close()
