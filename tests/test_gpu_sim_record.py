"""
GPU: the flight recorder of the fleet's closed-loop simulation (ltpl_fleet_sim_record*, csrc/fleet_sim.hpp k_fleet_sim_rec_paths /
k_fleet_sim_rec_vel): for chosen planners a full record of every tick, taken between calc_paths and the velocity stage and behind it.

  1. against the reference's recordings (c2, overtake): paths exactly, trajectories under the rules of the replay tests, the objects, the
     constant segment on the ticks whose full arrays were recorded
  2. the records as a tick log: written by ``write_sim_record``, re-validated on the device
  3. against a second fleet in lockstep (``sim_run(1)``, ``trajectories(p)`` and the trace after every tick): bit for bit
  4. the recorder changes nothing: trace, state, heading and telemetry with and without it, on both launch sequences
  5. the ring; 6. a race; 7. the edges (96 objects, none, a failed planner, bad arguments)
"""
import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import sim_record_util as ru
import test_gpu_fleet_race as gr
import test_gpu_fleet_sim as gs
import test_gpu_sim_differential as gd
from test_gpu_fleet_sim import hip, race                                   # noqa: F401  (fixtures)
from test_gpu_fleet_race import cars                                       # noqa: F401

pytestmark = pytest.mark.gpu

RECORDED = [69, 0, 37]


def recording_fleet(hip, monteblanco, race, name, n):
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    ticks = pr.load_ticks(name)
    fleet = Fleet(hip, n, **gs.SPECS[name][2])
    gs.start(fleet, [(ticks, range(n))])
    fleet.sim_setup(race, [gs.planner_entry(monteblanco, name, ticks)] * n)
    return fleet, ticks


def run_recorded(fleet, ticks, a, b, planners, depth):
    """Ticks [a, b) of the recording (the fleet stands in front of tick a), recorded from tick a on; returns the records."""
    fleet.sim_record(planners, depth)
    n = fleet.n_scen
    for s0, s1 in gs.segments([ticks[a:b]], b - a):
        gs.set_vel(fleet, [ticks[a:b]], [range(n)], s0)
        fleet.sim_run(s1 - s0, trace=False)
    return fleet.sim_record_read()


@pytest.fixture(scope="module")
def c2_records(hip, monteblanco, race):
    fleet, ticks = recording_fleet(hip, monteblanco, race, "c2", 70)
    recs = run_recorded(fleet, ticks, 0, 300, RECORDED, 300)
    info = fleet.sim_record_info()
    fleet.close()
    assert info == dict(n_planners=3, depth=300, first_tick=0, n_ticks=300)
    return ticks, recs


def check_against_recording(recs, ticks, first, planners, name):
    full = untrimmed = 0
    for i, row in enumerate(recs):
        t = ticks[first + i]
        assert [r["planner"] for r in row] == planners and all(r["tick"] == i for r in row)
        for r in row:
            w = "%s tick %d planner %d" % (name, first + i, r["planner"])
            assert r["error"] == 0 and r["sel"] == t["action_id_sel"] and r["t_now"] == t["t"], w
            assert np.max(np.abs(np.asarray(r["pos_est"]) - np.asarray(t["pos_est"], float))) <= 1e-6, w
            full += ru.check_paths(r, t, w)
            untrimmed += ru.check_record_trajectories(r, t, 115, w)
            ru.check_vehicles(r, t, w)
    return full, untrimmed


# ---- 1. the recordings ---------------------------------------------------------------------------------------------------------------
def test_records_hold_the_c2_recording(c2_records):
    ticks, recs = c2_records
    assert len(recs) == 300
    full, untrimmed = check_against_recording(recs, ticks, 0, RECORDED, "c2")
    assert full >= 3                                                       # (c2's trajectories are all longer than the export: the lockstep test has shorter ones)


def test_records_hold_the_overtake_recording_around_its_first_emergency_profile(hip, monteblanco, race):
    ticks = pr.load_ticks("overtake")
    first_em = next(i for i, t in enumerate(ticks) if "emergency" in t["vel"]["keys"])
    a = max(0, min(first_em - 100, len(ticks) - 200))
    b = a + 200
    assert a <= first_em < b
    fleet, _ = recording_fleet(hip, monteblanco, race, "overtake", 70)
    if a:                                                                  # the ticks in front of the window, unrecorded
        for s0, s1 in gs.segments([ticks[:a]], a):
            gs.set_vel(fleet, [ticks[:a]], [range(70)], s0)
            fleet.sim_run(s1 - s0, trace=False)
    recs = run_recorded(fleet, ticks, a, b, RECORDED, 200)
    fleet.close()
    assert len(recs) == 200
    check_against_recording(recs, ticks, a, RECORDED, "overtake")
    # (four keys over the window -- follow, left, right and, on every third tick, emergency --, three of them per tick)
    seen = set(k for row in recs for r in row for k in r["traj"][0])
    assert {"follow", "emergency"} <= seen and len(seen) >= 3 and all("emergency" in r["traj"][0] for r in recs[first_em - a]), seen


# ---- 2. the log ----------------------------------------------------------------------------------------------------------------------
def test_records_write_a_log_that_revalidates_on_the_device(tmp_path, monteblanco, hip_backend, c2_records):
    from graphbasedlocaltrajectoryplanner_amd import tick_log
    ticks, recs = c2_records
    path = str(tmp_path / "ticks_data.csv")
    w = tick_log.TickLogWriter(path, graph_id="fleet-sim")
    t0 = ticks[0]
    for row in recs:
        assert w.write_sim_record(row[1], hip_backend, t0.get('zone_layers', ()), t0.get('zone_nodes', ())) is True
    _, rows = tick_log.read_log(path)
    assert len(rows) == 300
    for r, t in zip(rows, ticks):
        assert r["time"] == t["t"] and r["action_id_prev"] == t["action_id_sel"] and r["start_node"] == t["paths"]["start_node"]
        assert {k: v[0] for k, v in r["nodes_list"].items()} == t["paths"]["nodes"]
    assert tick_log.revalidate(hip_backend, monteblanco, rows, w_last_edges=(0.0, 0.5, 0.8), context=True) == []


# ---- 3. lockstep, bit for bit ----------------------------------------------------------------------------------------------------------
def lockstep_units(classes, c2_start):
    # Trajectories on Monteblanco hold 126 .. 163 rows, at standstill (emerg_first, emerg_second) as well: they are longer than the reference's
    # export of 115 rows and than 40, and every one is SHORTER than the export at the cap of 256 rows (tests/test_sim_loop_host.py asserts
    # both for these classes), which is where the record ends in front of n_export and what lies behind stays out of the view
    return [gd.single(n, classes[n], c2_start) for n in ("one", "emerg_first", "crowded", "empty", "emerg_second")]


@pytest.mark.parametrize("n_export", [115, 40, 256])
def test_records_equal_a_lockstep_fleet_bit_for_bit(hip, monteblanco, race, n_export):
    classes = sl.monteblanco_classes(race, np.load(gs.ROOT + "/tests/golden/monteblanco_track.npz"), tuple(pr.load_ticks("c2")[0]['start']['pos']))
    sc = gd.Scenario(monteblanco, race, lockstep_units(classes, pr.load_ticks("c2")[0]['start']), n_export=n_export)
    K, planners = 60, [3, 1, 4, 0, 2]
    rec_fleet = sc.fleet(hip)
    rec_fleet.sim_record(planners, K)
    rec_fleet.sim_run(K, trace=False)
    recs = rec_fleet.sim_record_read()
    rec_fleet.close()
    step = sc.fleet(hip)
    shorter = longer = 0
    for i in range(K):
        trace = step.sim_run(1)[0][0]
        for r in recs[i]:
            p, w = r["planner"], "tick %d planner %d" % (i, r["planner"])
            traj, ids, ref = step.trajectories(p)
            head = [gs_key(r["sel"]), r["t_now"], r["pos_est"][0], r["pos_est"][1], r["vel_est"], len(r["vehicles"])]
            assert np.array_equal(np.asarray(head, float), trace[p, :6]), w
            assert r["error"] == 0 and trace[p, 8] == 0, w
            rt, rids, rref = r["traj"]
            assert list(rt.keys()) == list(traj.keys()) and rids == ids, w
            assert all(rref[k] == ref[k] for k in ("cut_index_pos", "cut_layer", "vel_plan", "acc_plan")), w
            for k in traj:
                assert np.array_equal(rt[k][0], traj[k][0][:n_export]), "%s/%s" % (w, k)
                shorter += traj[k][0].shape[0] < n_export
                longer += traj[k][0].shape[0] > n_export
    step.close()
    assert (shorter > 0 and longer == 0) if n_export == 256 else (longer > 0), (shorter, longer)


def gs_key(name):
    from graphbasedlocaltrajectoryplanner_amd.planner import KEY_IDS
    return KEY_IDS[name]


def test_record_counts_equal_the_views(hip, monteblanco, race):
    """The C views of a record against ltpl_fleet_get_trajectories after the same tick: untrimmed row counts, key / trajectory ids, id pairs."""
    import ctypes as C
    from graphbasedlocaltrajectoryplanner_amd.planner import TrajView
    fleet, ticks = recording_fleet(hip, monteblanco, race, "c2", 2)
    gs.set_vel(fleet, [ticks], [range(2)], 0)
    fleet.sim_record([1], 4)
    for i in range(30):
        fleet.sim_run(1, trace=False)
        a, b = TrajView(), TrajView()
        fleet._check(fleet._fn("sim_record_get")(fleet.handle, i, 0, None, None, None, None, C.byref(a)))
        fleet._check(fleet._fn("get_trajectories")(fleet.handle, 1, C.byref(b)))
        assert a.n_keys == b.n_keys and a.n_ids == b.n_ids and a.n_vel_course == 0
        for name in ("key_id", "traj_id", "n_rows"):
            assert getattr(a, name)[:a.n_keys] == getattr(b, name)[:b.n_keys], (i, name)
        assert a.id_key[:a.n_ids] == b.id_key[:b.n_ids] and a.id_val[:a.n_ids] == b.id_val[:b.n_ids]
        assert (a.cut_index_pos, a.cut_layer, a.vel_plan, a.acc_plan) == (b.cut_index_pos, b.cut_layer, b.vel_plan, b.acc_plan)
    fleet.close()


# ---- 4. the recorder changes nothing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_fuse", [None, "1"])
def test_the_recorder_changes_nothing(hip, monteblanco, race, monkeypatch, no_fuse):
    if no_fuse:
        monkeypatch.setenv("LTPL_FLEET_NO_FUSE", no_fuse)
    else:
        monkeypatch.delenv("LTPL_FLEET_NO_FUSE", raising=False)
    out = []
    for rec in (False, True):
        fleet, ticks = recording_fleet(hip, monteblanco, race, "c2", 5)
        gs.set_vel(fleet, [ticks], [range(5)], 0)
        fleet.sim_telemetry(radius=2.5)
        if rec:
            fleet.sim_record([4, 0, 2], 50)
        trace = fleet.sim_run(200)[0]
        tele = fleet.sim_telemetry_read()
        out.append((trace, fleet.sim_state(), fleet.sim_heading(), tele, fleet.digest()))
        if rec:
            assert fleet.sim_record_info() == dict(n_planners=3, depth=50, first_tick=150, n_ticks=50)
        fleet.close()
    (ta, sa, ha, ea, da), (tb, sb, hb, eb, db) = out
    assert np.array_equal(ta, tb, equal_nan=True) and np.array_equal(ha, hb) and np.array_equal(da, db)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    for k in ea:
        assert np.array_equal(np.asarray(ea[k]), np.asarray(eb[k]), equal_nan=True), k


# ---- 5. the ring -----------------------------------------------------------------------------------------------------------------------
def test_ring_keeps_the_last_ticks(hip, monteblanco, race, c2_records):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    ticks, ref = c2_records
    fleet, _ = recording_fleet(hip, monteblanco, race, "c2", 70)
    gs.set_vel(fleet, [ticks], [range(70)], 0)
    fleet.sim_record(RECORDED, 7)
    assert fleet.sim_record_info() == dict(n_planners=3, depth=7, first_tick=0, n_ticks=0) and fleet.sim_record_read() == []
    fleet.sim_run(10, trace=False)
    assert fleet.sim_record_info()["first_tick"] == 3
    fleet.sim_run(5, trace=False)
    assert fleet.sim_record_info() == dict(n_planners=3, depth=7, first_tick=8, n_ticks=7)
    recs = fleet.sim_record_read()
    assert [row[0]["tick"] for row in recs] == list(range(8, 15))
    for row, want in zip(recs, ref[8:15]):
        for a, b in zip(row, want):
            assert a["tick"] == b["tick"] and ru.records_equal(a, b, skip=()) is None, (a["tick"], ru.records_equal(a, b, skip=()))
    assert [r["tick"] for r in fleet.sim_record_read(first=12, count=2)[1]] == [13] * 3
    for bad in (7, 15, -1):
        with pytest.raises(BackendError, match="does not hold this tick"):
            fleet.sim_record_read(first=bad, count=1)
    # depth 1 holds the last tick; setting the recorder again restarts tick 0
    fleet.sim_record([37], 1)
    assert fleet.sim_record_info() == dict(n_planners=1, depth=1, first_tick=0, n_ticks=0)
    fleet.sim_run(3, trace=False)
    assert fleet.sim_record_info() == dict(n_planners=1, depth=1, first_tick=2, n_ticks=1)
    (last,), = fleet.sim_record_read()
    assert last["tick"] == 2 and ru.records_equal(last, ref[17][2]) is None, ru.records_equal(last, ref[17][2])
    fleet.sim_record(None)
    assert fleet.sim_record_info()["n_planners"] == 0
    with pytest.raises(BackendError, match="recorder is off"):
        fleet._check(fleet._fn("sim_record_get")(fleet.handle, 0, 0, None, None, None, None, None))
    fleet.close()


# ---- 6. a race -------------------------------------------------------------------------------------------------------------------------
def test_race_records_hold_every_car(hip, monteblanco, race, cars):
    name, T = "race4", 600
    nd = len(gr.SCEN[name]["dummies"])
    out = []
    for before in (True, False):
        fleet, recs, sizes, entries, plan = gr.race_fleet(hip, race, cars, [(name, 1)])
        ent = [gr.car_entry(name, k) for k in range(4)]
        fleet.sim_setup(race, ent)
        if before:
            fleet.sim_record(range(4), T)
        fleet.sim_race(sizes, length=5.0)
        if not before:
            fleet.sim_record(range(4), T)
        trace, _ = gr.run(fleet, recs, T, every=T)
        out.append((fleet.sim_record_read(), trace))
        fleet.close()
    (ra, trace), (rb, _) = out
    assert len(ra) == T
    mates = 0
    for i in range(T):
        for k in range(4):
            r, t = ra[i][k], cars[name][k][i]
            w = "race4 car %d tick %d" % (k, i)
            assert r["planner"] == k and r["error"] == 0
            assert list(r["paths"]["start_node"]) == t["paths"]["start_node"] and r["paths"]["nodes"] == t["paths"]["nodes"], w
            assert len(r["vehicles"]) == trace[i, k, 5] == len(t["obj_radius"]), w
            for (rad, v, pos), ep in zip(r["vehicles"], t["obj_pos"]):
                assert np.max(np.abs(pos[0] - np.asarray(ep, float))) <= 1e-6, w
            # race4 has no dummies: every object is a mate, in ascending planner order, at the pose that mate's tracker wrote this tick
            assert nd == 0
            q = 0
            for rad, v, pos in r["vehicles"]:
                while q < 4 and (q == k or list(pos[0]) != ra[i][q]["pos_est"]):
                    q += 1
                assert q < 4 and v == ra[i][q]["vel_est"] and rad == 2.5, w
                q += 1
            mates += len(r["vehicles"])
            assert ru.records_equal(r, rb[i][k], skip=()) is None, w
    assert mates > 0


# ---- 7. edges --------------------------------------------------------------------------------------------------------------------------
def test_a_planner_at_the_object_cap_and_one_without_objects(hip, monteblanco, race):
    entries, poses = sl.big_race(race, sl.CAP_RACE_CARS, own=sl.cap_race_own(race))
    c2 = pr.load_ticks("c2")[0]['start']
    classes = sl.monteblanco_classes(race, np.load(gs.ROOT + "/tests/golden/monteblanco_track.npz"), tuple(c2['pos']))
    sc = gd.Scenario(monteblanco, race, [gd.race_unit("cap", entries, poses), gd.single("empty", classes["empty"], c2)])
    fleet = sc.fleet(hip)
    n = fleet.n_scen
    fleet.sim_record([n - 1, 0, sl.CAP_RACE_CARS - 1], 12)
    trace = fleet.sim_run(12)[0]
    recs = fleet.sim_record_read()
    fleet.close()
    for i, row in enumerate(recs):
        assert [len(r["vehicles"]) for r in row] == [0, 96, 96] and [r["error"] for r in row] == [0, 0, 0]
        for r in row[1:]:
            assert len(r["vehicles"]) == trace[i, r["planner"], 5]
            assert np.array_equal(r["vehicles"][0][2][0], trace[i, r["planner"], 6:8])
            assert all(np.all(np.isfinite(pos)) and rad == 2.5 for rad, v, pos in r["vehicles"])
            # the last object of car 0 is the last mate: the pose its tracker wrote this tick (the trace of that planner)
        assert np.array_equal(row[1]["vehicles"][95][2][0], trace[i, sl.CAP_RACE_CARS - 1, 2:4])
        assert np.array_equal(row[2]["vehicles"][95][2][0], trace[i, sl.CAP_RACE_CARS - 2, 2:4])


def test_a_failed_planner_is_recorded_with_its_error_word(tmp_path, hip, hip_backend, monteblanco, race, c2_records):
    from graphbasedlocaltrajectoryplanner_amd import tick_log
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    ticks, ref = c2_records
    fleet = Fleet(hip, 3)
    gs.start(fleet, [(ticks, range(3))])
    e = gs.planner_entry(monteblanco, "c2", ticks)
    fleet.sim_setup(race, [e, dict(e, pref=("right",)), e])
    gs.set_vel(fleet, [ticks], [range(3)], 0)
    fleet.sim_record([1, 2], 40)
    with pytest.raises(BackendError, match="planner 1: closed-loop simulation"):
        fleet.sim_run(40)
    trace = fleet.last_trace
    recs = fleet.sim_record_read()
    # bad arguments: refused, the recorder and its ticks stay
    for planners, depth, why in (([0, 3], 4, "out of range"), ([-1], 4, "out of range"), ([0, 2, 0], 4, "twice"), ([0], 0, "depth")):
        with pytest.raises(BackendError, match=why):
            fleet.sim_record(planners, depth)
    assert fleet.sim_record_info() == dict(n_planners=2, depth=40, first_tick=0, n_ticks=40)
    with pytest.raises(BackendError):
        fleet.sim_run(2)
    assert fleet.sim_record_info() == dict(n_planners=2, depth=40, first_tick=2, n_ticks=40)
    assert [r["tick"] for r in fleet.sim_record_read(first=41, count=1)[0]] == [41, 41]
    fleet.close()
    w = tick_log.TickLogWriter(str(tmp_path / "ticks_data.csv"))
    st = ticks[0]['start']
    for i, (bad, good) in enumerate(recs):
        assert bad["planner"] == 1 and bad["error"] == trace[i, 1, 8] != 0 and bad["tick"] == i
        assert bad["vehicles"] == [] and bad["paths"]["keys"] == [] and bad["traj"][0] == {} and bad["traj"][1] == {}
        assert bad["pos_est"] == list(map(float, st['pos'])) and bad["paths"]["const_path_seg"] is None
        assert w.write_sim_record(bad, hip_backend) is False
        assert good["planner"] == 2 and good["tick"] == i and good["error"] == 0
        ru.check_paths(good, ticks[i], "neighbour tick %d" % i)
        ru.check_record_trajectories(good, ticks[i], 115, "neighbour tick %d" % i)
        ru.check_vehicles(good, ticks[i], "neighbour tick %d" % i)
        assert w.write_sim_record(good, hip_backend) is True
    assert len(tick_log.read_log(w.path)[1]) == 40


def test_record_needs_a_simulation(hip):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    fleet = Fleet(hip, 2)
    with pytest.raises(BackendError, match="ltpl_fleet_sim_setup first"):
        fleet.sim_record([0], 3)
    with pytest.raises(BackendError, match="ltpl_fleet_sim_setup first"):
        fleet.sim_record_info()
    fleet.close()
