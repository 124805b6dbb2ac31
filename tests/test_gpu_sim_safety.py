"""
GPU: the safety monitor of the fleet's closed-loop simulation (ltpl_fleet_sim_safety / _safety_read / _safety_eval; csrc/fleet_safety.hpp,
k_fleet_sim_safety / k_fleet_sim_safety_eval in csrc/fleet_sim.hpp, k_fleet_sim_branch_safety in csrc/fleet_branch.hpp) against its host
mirror (sim.SafetyModel / sim.safety_tick) --

  1. the hook: records, rings, per-object and per-tick values bit for bit against the mirror on the case list of sim_safety_util.cases
     (0, 1, 64, 65 and 96 objects among them), in batches of 1, 63, 64 and 65 cases, and on the incident sequences with the record
     carried from tick to tick;
  2. 8 planners x 60 ticks (mixed `on` and parameters, one race of three): the mirror fed with each tick's staged objects from the flight
     recorder and the pose from sim_state; records and rings bitwise in every tick; one sim_run(60) gives the same records bit for bit;
  3. the monitor changes nothing else: trace, state, heading, digest and the telemetry record with and without it, and a cleared monitor;
  4. noise: with ego sigmas only the record equals the mirror fed with the TRUE pose; with object noise too, two planners among statics
     (true positions: the configured ones): record and ring bitwise against the mirror fed with true positions and perceived
     displacements; gap_min == clear_min - r_ego bitwise against the telemetry of the same run (both measure the true positions);
  5. snapshot, run, restore, sim_safety(keep_state, tick0), run reproduces records and rings; a branch onto a planner with other
     thresholds carries record and ring and keeps the thresholds; a source without a record leaves the start state;
  6. a planner that fails keeps its record; keep_state; every refusal.
"""
import os

import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import sim_safety_util as su
import sim_selector_util as slu
import test_gpu_sim_differential as gd
import test_gpu_sim_noise as gn
from graphbasedlocaltrajectoryplanner_amd import sim
from graphbasedlocaltrajectoryplanner_amd.sim import Event

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = su.bits
ENTRY = dict(opponents=[(250.0, 0.3, 5.0)], static=[], pref=sl.DEFAULT_PREF, pos_est=(0.0, 0.0), vel_est=0.0, zone_gids=[])
PAR = dict(r_ego=1.5, ttc_thr=8.0, drac_thr=0.5, thw_thr=3.0, margin=1.0)


@pytest.fixture(scope="module")
def hip(monteblanco):
    from graphbasedlocaltrajectoryplanner_amd import _capi
    return _capi.HipBackend(monteblanco)


@pytest.fixture(scope="module")
def table():
    return sim.RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


@pytest.fixture(scope="module")
def track():
    return np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz"))


@pytest.fixture(scope="module")
def c2_start():
    return pr.load_ticks("c2")[0]['start']


def objects_of(record):
    """[n, 5] = x, y, px, py, r of the vehicles a recorded planner was handed."""
    return np.asarray([[xy[0][0], xy[0][1], xy[1][0], xy[1][1], rad] for rad, _, xy in record["vehicles"]], np.float64).reshape(-1, 5)


def units8(table, track, start):
    s = gn.singles(table, track, start)
    units = [s[0], gn.race3(table), s[1], s[2]]
    # two flying starts at 20 m/s behind an opponent at 0.2 of the race-line speed (the CPU test's scenario: a closing phase with TTC around
    # 6 s and a positive required deceleration, then following)
    for k, gap in enumerate((60.0, 45.0)):
        entry = dict(slu.chase_entry(table, start, gap=gap, scale=0.2, pref=("follow", "straight")), vel_est=20.0)
        units.append(gd.single("chase%d" % k, dict(entry=entry, vel=sl.C2_VEL, start_vel=20.0), start))
    return units


def same(dev, model, what):
    rec, inc = dev
    assert np.array_equal(bits(rec), bits(model.rec)), "%s: records differ at %s\n%s\n%s" % (
        what, np.argwhere(bits(rec) != bits(model.rec))[:6].tolist(), rec[bits(rec) != bits(model.rec)][:6], model.rec[bits(rec) != bits(model.rec)][:6])
    assert np.array_equal(bits(inc), bits(model.inc)), "%s: incident rings differ" % what


# ---- 1. the hook --------------------------------------------------------------------------------------------------------------------------
def test_the_hook_equals_the_mirror_bit_for_bit(hip):
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    cs = su.cases()[0]
    ref = [su.mirror(c) for c in cs]
    assert {0, 1, 64, 65, 96} <= {c["objs"].shape[0] for c in cs}
    fleet = Fleet(hip, 1)
    at = 0
    for m in (1, 63, 64, 65):
        idx = [(at + k) % len(cs) for k in range(m)]
        at += m
        start = [su.start_of(cs[i]) for i in idx]
        rec, inc, po, pt = fleet.sim_safety_eval([cs[i]["pose"] for i in idx], [cs[i]["dt"] for i in idx], [cs[i]["tick"] for i in idx],
                                                 [cs[i]["par"] for i in idx], [cs[i]["objs"] for i in idx], rec=[s[0] for s in start],
                                                 inc=[s[1] for s in start])
        for j, i in enumerate(idx):
            su.compare(dict(rec=rec[j], inc=inc[j], per_obj=po[j], per_tick=pt[j]), ref[i], "batch of %d, case %d" % (m, i))
    assert at >= len(cs)                    # every case ran at least once

    def hook(c, rec, inc):
        r0, i0 = su.start_of(c)
        rec, inc, po, pt = fleet.sim_safety_eval([c["pose"]], [c["dt"]], [c["tick"]], [c["par"]], [c["objs"]], rec=[r0 if rec is None else rec],
                                                 inc=[i0 if inc is None else inc])
        return dict(rec=rec[0], inc=inc[0], per_obj=po[0], per_tick=pt[0])
    for ttcs in ([4.0, 3.0, 2.0, 2.5, 4.0, None, 1.0, 4.0], [1.0, 4.0] * 9):
        seq = su.sequence(ttcs)
        for k, (a, b) in enumerate(zip(su.run_sequence(seq, hook), su.run_sequence(seq))):
            su.compare(a, b, "sequence tick %d" % k)
    # the default start state is the mirror's
    c = cs[-1]
    rec, inc, _, _ = fleet.sim_safety_eval([c["pose"]], [c["dt"]], [c["tick"]], [c["par"]], [c["objs"]])
    su.compare(dict(rec=rec[0], inc=inc[0], per_obj=ref[-1]["per_obj"], per_tick=ref[-1]["per_tick"]), ref[-1], "default start state")
    assert len(fleet.sim_safety_eval(np.zeros((0, 2)), [], [], np.zeros((0, 5)), [])[2]) == 0
    fleet.close()


# ---- 2. the tick --------------------------------------------------------------------------------------------------------------------------
SKW = dict(on=[1, 1, 1, 1, 0, 1, 1, 1], r_ego=[1.5, 1.0, 2.0, 1.5, 1.5, 0.5, 1.5, 2.5], ttc_thr=[8.0, 3.0, 20.0, 8.0, 8.0, 5.0, 12.0, 8.0],
           drac_thr=[0.5, 0.0, 1.0, 0.5, 0.5, 3.0, 0.2, 0.5], thw_thr=[3.0, 1.0, 5.0, 3.0, 3.0, 0.0, 4.0, 3.0],
           margin=[1.0, 0.0, 2.0, 1.0, 1.0, 0.5, 3.0, 1.0])


def mirrored_ticks(fleet, model, n_ticks, dt, what, truth=None):
    """sim_run(1) n_ticks times; the mirror fed with the staged objects from the recorder and the TRUE pose from sim_state; compared in
    every tick. ``truth`` (sensor noise on): planner, staged list -> the TRUE positions [n, 2] of its objects; the mirror then gets what the
    kernel forms, true positions and perceived displacements (sim.safety_objects). Returns the traces."""
    out = []
    for k in range(n_ticks):
        tr = gd.run_one(fleet, 1)[0]
        recs = fleet.sim_record_read()[-1]
        pose = fleet.sim_state()["pos_est"]
        for p in range(model.n):
            if tr[p, 8] == 0:                # (a planner that fails here fails in the step kernel: live == not failed)
                staged = objects_of(recs[p])
                model.step(p, pose[p], staged if truth is None else sim.safety_objects(staged, truth(p, staged)), dt)
        model.advance()
        same(fleet.sim_safety_read(raw=True), model, "%s, tick %d" % (what, k))
        out.append(tr)
    return np.asarray(out)


def test_sixty_ticks_of_eight_planners_against_the_mirror(hip, monteblanco, table, track, c2_start):
    n_ticks = 60
    sc = gd.Scenario(monteblanco, table, units8(table, track, c2_start))
    assert sc.n == 8
    fleet = sc.fleet(hip)
    fleet.sim_safety(tick0=5, **SKW)
    fleet.sim_record(list(range(sc.n)), depth=1)
    model = sim.SafetyModel(sc.n, tick0=5, **SKW)
    tr = mirrored_ticks(fleet, model, n_ticks, sc.dt, "lockstep")
    assert np.all(tr[:, :, 8] == 0)
    single = fleet.sim_safety_read(raw=True)
    fleet.close()
    d = model.as_dict()
    print("safety records after %d ticks: %s" % (n_ticks, {k: v.tolist() for k, v in d.items()}))
    assert d["ticks"][4] == 0 and np.all(np.delete(d["ticks"], 4) == n_ticks) and np.all(np.delete(d["ticks_eval"], 4) == n_ticks - 1)
    assert np.all(np.delete(d["gap_tick"], 4) >= 5)              # tick0 counts
    assert np.sum(np.isfinite(d["ttc_min"])) >= 3 and np.sum(d["drac_max"] > 0) >= 3 and np.sum(np.isfinite(d["thw_min"])) >= 3
    assert d["n_incidents"].sum() >= 1 and np.array_equal(d["hist"].sum(axis=1), d["ticks_eval"])
    whole = sc.fleet(hip)
    whole.sim_safety(tick0=5, **SKW)
    whole.sim_run(n_ticks)
    rec, inc = whole.sim_safety_read(raw=True)
    whole.close()
    assert np.array_equal(bits(rec), bits(single[0])) and np.array_equal(bits(inc), bits(single[1])), "one sim_run(60) differs from 60 single ticks"


# ---- 3. no side effects -------------------------------------------------------------------------------------------------------------------
def test_the_monitor_changes_nothing_else(hip, monteblanco, table, track, c2_start):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    sc = gd.Scenario(monteblanco, table, gn.mixed(table, track, c2_start))

    def run(mode):
        fleet = sc.fleet(hip)
        fleet.sim_telemetry(radius=2.5)
        fleet.sim_record(list(range(sc.n)), depth=1)
        if mode != "never":
            fleet.sim_safety(**PAR)
        if mode == "cleared":
            fleet.sim_safety(None)
            with pytest.raises(BackendError, match="the monitor is off"):
                fleet.sim_safety_read()
        tr = fleet.sim_run(30)[0]
        st, dg, te = fleet.sim_state(), fleet.digest(), fleet.sim_telemetry_read()
        heading = [r["heading"] for r in fleet.sim_record_read()[-1]]
        saf = fleet.sim_safety_read()[0] if mode == "on" else None
        fleet.close()
        return tr, st, dg, te, heading, saf
    ref = run("never")
    for mode in ("on", "cleared"):
        got = run(mode)
        assert np.array_equal(bits(got[0]), bits(ref[0])), mode
        assert all(np.array_equal(got[1][k], ref[1][k]) for k in ref[1]) and np.array_equal(got[2], ref[2]), mode
        assert all(np.array_equal(bits(got[3][k]), bits(ref[3][k])) for k in ref[3]), mode      # (track_length, a scalar, included)
        assert np.array_equal(bits(got[4]), bits(ref[4])), mode
        if mode == "on":                    # ... while it measured: and telemetry's clearance is its gap
            assert np.all(got[5]["ticks"] == 30)
            has = got[3]["clear_tick"] >= 0
            assert np.array_equal(bits(got[5]["gap_min"][has]), bits(got[3]["clear_min"][has] - PAR["r_ego"]))
            assert np.array_equal(got[5]["gap_tick"][has], got[3]["clear_tick"][has]) and np.array_equal(got[5]["gap_slot"][has], got[3]["clear_slot"][has])
    # sim_setup switches the monitor off
    fleet = sc.fleet(hip)
    fleet.sim_safety(**PAR)
    fleet.sim_setup(sc.tab, sc.entries, dt=sc.dt, n_export=sc.n_export)
    with pytest.raises(BackendError, match="the monitor is off"):
        fleet.sim_safety_read()
    fleet.close()


# ---- 4. noise -----------------------------------------------------------------------------------------------------------------------------
def test_under_noise_the_monitor_measures_the_true_pose_and_the_true_positions(hip, monteblanco, table, track, c2_start):
    sc = gd.Scenario(monteblanco, table, gn.mixed(table, track, c2_start))
    n = sc.n
    fleet = sc.fleet(hip)
    fleet.sim_noise(seed=np.arange(n, dtype=np.uint64) + np.uint64(11), pos=0.4, vel=0.3)      # ego sigmas only: the staged objects are the true ones
    fleet.sim_safety(**PAR)
    fleet.sim_record(list(range(n)), depth=1)
    model = sim.SafetyModel(n, **PAR)
    mirrored_ticks(fleet, model, 30, sc.dt, "ego noise", truth=lambda p, staged: staged[:, :2])
    # the estimate the planner was handed is another point than the pose the monitor measured from
    assert not np.any(fleet.sim_estimate()["pos_est"] == fleet.sim_state()["pos_est"])
    fleet.close()
    assert np.all(model.rec[:, 1] == 29)
    # object noise: planners among standing and slowly moving statics, whose TRUE positions are the configured ones. The whole record and
    # the ring equal the mirror fed with true positions and perceived displacements; (Q_staged - X_true) / 0.2 as the velocity would fail
    classes = sl.monteblanco_classes(table, track, tuple(c2_start['pos']))
    st = gd.Scenario(monteblanco, table, [gd.single("statics%d" % k, classes["statics"], c2_start) for k in range(2)])
    par = dict(PAR, ttc_thr=[8.0, 20.0], margin=[1.0, 4.0])
    sigma = [0.4, 0.25]
    fleet = st.fleet(hip)
    fleet.sim_noise(seed=np.array([21, 22], np.uint64), pos=0.3, obj_pos=sigma, obj_theta=0.1, obj_vel=1.0)
    fleet.sim_safety(**par)
    fleet.sim_record([0, 1], depth=1)
    model = sim.SafetyModel(2, **par)
    moved = [0.0]

    def truth(p, staged):
        """The configured static each staged object is: the nearest one, which must be the only one within 6 sigma."""
        xy = np.asarray([r[:2] for r in st.entries[p]["static"]], np.float64)
        out = np.zeros((staged.shape[0], 2))
        for i, o in enumerate(staged):
            d = np.hypot(xy[:, 0] - o[0], xy[:, 1] - o[1])
            k = int(np.argmin(d))
            assert d[k] < 6 * sigma[p] and np.sum(d < 12 * sigma[p]) == 1, "planner %d: staged object %d at %s: distances %s" % (p, i, o[:2], np.sort(d)[:3])
            out[i] = xy[k]
            moved[0] = max(moved[0], d[k])
        return out
    n_obj = mirrored_statics(fleet, model, 40, st.dt, truth)
    fleet.close()
    d = model.as_dict()
    print("object noise, statics: %d objects mirrored, perceived up to %.3f m off; records %s" % (n_obj, moved[0], {k: v.tolist() for k, v in d.items()}))
    assert moved[0] > 0.3 and n_obj > 100 and np.all(d["ticks_eval"] == 39) and np.all(np.isfinite(d["ttc_min"])) and np.all(d["drac_max"] > 0.0)
    fleet = sc.fleet(hip)
    fleet.sim_noise(**gn.noise_args(n))
    fleet.sim_telemetry(radius=2.5)
    fleet.sim_safety(**PAR)
    fleet.sim_run(40)
    d, te = fleet.sim_safety_read()[0], fleet.sim_telemetry_read()
    fleet.close()
    has = te["clear_tick"] >= 0
    assert has.sum() >= 3
    assert np.array_equal(bits(d["gap_min"][has]), bits(te["clear_min"][has] - PAR["r_ego"])), (d["gap_min"], te["clear_min"])
    assert np.array_equal(d["gap_tick"][has], te["clear_tick"][has]) and np.array_equal(d["gap_slot"][has], te["clear_slot"][has])


def mirrored_statics(fleet, model, n_ticks, dt, truth):
    """mirrored_ticks for the planners the model has on (the others' records are not compared); returns the number of objects mirrored."""
    n_obj = 0
    for k in range(n_ticks):
        tr = gd.run_one(fleet, 1)[0]
        recs, pose = fleet.sim_record_read()[-1], fleet.sim_state()["pos_est"]
        rec, inc = fleet.sim_safety_read(raw=True)
        for p in range(model.n):
            if model.on[p] and tr[p, 8] == 0:
                staged = objects_of(recs[p])
                n_obj += staged.shape[0]
                model.step(p, pose[p], sim.safety_objects(staged, truth(p, staged)), dt)
                assert np.array_equal(bits(rec[p]), bits(model.rec[p])), "object noise, tick %d planner %d: record differs at %s\n%s\n%s" % (
                    k, p, np.nonzero(bits(rec[p]) != bits(model.rec[p]))[0].tolist(), rec[p], model.rec[p])
                assert np.array_equal(bits(inc[p]), bits(model.inc[p])), "object noise, tick %d planner %d: ring differs" % (k, p)
        model.advance()
    return n_obj


# ---- 5. snapshot and branch ---------------------------------------------------------------------------------------------------------------
def test_snapshot_restore_and_branch_carry_record_and_ring(hip, monteblanco, table, track, c2_start):
    sc = gd.Scenario(monteblanco, table, units8(table, track, c2_start))
    fleet = sc.fleet(hip)
    fleet.sim_safety(**SKW)
    fleet.sim_run(25)
    fleet.sim_snapshot(0)
    at_snapshot = fleet.sim_safety_read(raw=True)
    runs = []
    for rep in range(2):
        ticks = []
        for k in range(20):
            fleet.sim_run(1)
            ticks.append(fleet.sim_safety_read(raw=True))
        runs.append(ticks)
        if rep == 0:
            fleet.sim_restore(0)
            back = fleet.sim_safety_read(raw=True)
            assert np.array_equal(bits(back[0]), bits(at_snapshot[0])) and np.array_equal(bits(back[1]), bits(at_snapshot[1]))
            fleet.sim_safety(tick0=25, keep_state=True, **SKW)
    for k, (a, b) in enumerate(zip(*runs)):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])), "tick %d behind the restore" % k
    assert not np.array_equal(bits(runs[0][-1][0]), bits(at_snapshot[0]))
    # a branch onto a planner with other thresholds: record and ring travel, the thresholds stay -- planner 7 (ttc_thr 8) onto 6 (ttc_thr 12)
    rec, inc = fleet.sim_safety_read(raw=True)
    fleet.sim_branch(7, [6])
    rec2, inc2 = fleet.sim_safety_read(raw=True)
    assert np.array_equal(bits(rec2[6]), bits(rec[7])) and np.array_equal(bits(inc2[6]), bits(inc[7]))
    keep = [p for p in range(8) if p != 6]
    assert np.array_equal(bits(rec2[keep]), bits(rec[keep])) and np.array_equal(bits(inc2[keep]), bits(inc[keep]))
    model = sim.SafetyModel(8, tick0=45, **SKW)
    model.rec[:], model.inc[:] = rec2, inc2
    fleet.sim_record(list(range(8)), depth=1)
    mirrored_ticks(fleet, model, 5, sc.dt, "behind the branch")          # planner 6 goes on with ITS thresholds on planner 7's record
    # a source without a record: a snapshot taken with the monitor off leaves the start state, and the first tick is not evaluated
    fleet.sim_safety(None)
    fleet.sim_snapshot(1)
    fleet.sim_safety(**SKW)
    fleet.sim_run(3)
    fleet.sim_restore(1)
    rec, inc = fleet.sim_safety_read(raw=True)
    r0, i0 = sim.safety_start(8)
    assert np.array_equal(bits(rec), bits(r0)) and np.all(np.isnan(inc))
    fleet.sim_run(2)
    d = fleet.sim_safety_read()[0]
    assert np.all(np.delete(d["ticks"], 4) == 2) and np.all(np.delete(d["ticks_eval"], 4) == 1) and d["ticks"][4] == 0
    fleet.close()


# ---- 6. failure, keep_state, refusals -----------------------------------------------------------------------------------------------------
def test_a_failed_planner_keeps_its_record_and_keep_state_keeps_them_all(hip, monteblanco, table, track, c2_start):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    classes = sl.monteblanco_classes(table, track, tuple(c2_start['pos']))
    one = classes["one"]
    sc = gd.Scenario(monteblanco, table, [gd.single("fails", one, c2_start), gd.single("one", one, c2_start)])
    fleet = sc.fleet(hip)
    fleet.sim_safety(**PAR)
    # every entry of planner 0's list becomes `emergency` at tick 20, which is never exported here: the step kernel finds no action
    fleet.sim_events([Event(0, when=("tick", 20), set=("pref", e, "emergency")) for e in range(len(one["entry"]["pref"]))])
    tr = gd.run_one(fleet, 40)
    live = int(np.sum(tr[:, 0, 8] == 0))
    assert live == 20 and np.all(tr[:, 1, 8] == 0)               # planner 0 fails on the way
    rec, inc = fleet.sim_safety_read(raw=True)
    assert rec[0, 0] == live and rec[0, 1] == live - 1 and rec[1, 0] == 40
    gd.run_one(fleet, 5)
    rec2, _ = fleet.sim_safety_read(raw=True)
    assert np.array_equal(bits(rec2[0]), bits(rec[0])) and rec2[1, 0] == 45
    # keep_state: new thresholds and tick index on the old records -- the mirror goes on from them
    new = dict(PAR, ttc_thr=30.0, thw_thr=10.0, drac_thr=0.0, margin=3.0)
    fleet.sim_safety(keep_state=True, tick0=1000, **new)
    rec3, inc3 = fleet.sim_safety_read(raw=True)
    assert np.array_equal(bits(rec3), bits(rec2))
    model = sim.SafetyModel(2, tick0=1000, **new)
    model.rec[:], model.inc[:] = rec3, inc3
    fleet.sim_record([0, 1], depth=1)
    mirrored_ticks(fleet, model, 3, sc.dt, "keep_state")
    d = fleet.sim_safety_read()[0]
    assert d["ticks"][1] == 48 and d["ticks_eval"][1] == 47 and d["ticks"][0] == rec[0, 0]     # prev_valid stayed: no unevaluated tick
    # without the flag the records start anew; a refused call keeps monitor and records
    with pytest.raises(BackendError, match="planner 1: ttc_thr"):
        fleet.sim_safety(**dict(PAR, ttc_thr=[1.0, 0.0]))
    assert fleet.sim_safety_read()[0]["ticks"][1] == 48
    fleet.sim_safety(**PAR)
    assert np.all(fleet.sim_safety_read()[0]["ticks"] == 0)
    fleet.close()


def test_every_refusal(hip, table):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    fleet = Fleet(hip, 2)
    with pytest.raises(BackendError, match="ltpl_fleet_sim_setup first"):
        fleet.sim_safety(**PAR)
    fleet.sim_setup(table, [ENTRY, ENTRY])
    with pytest.raises(BackendError, match="the monitor is off"):
        fleet.sim_safety_read()
    for bad, text in ((dict(ttc_thr=0.0), "ttc_thr must be positive"), (dict(ttc_thr=[1.0, -2.0]), "planner 1: ttc_thr"), (dict(r_ego=-1.0), "r_ego"),
                      (dict(drac_thr=-0.5), "drac_thr"), (dict(thw_thr=[-1e-300, 0.0]), "planner 0: thw_thr"), (dict(margin=np.nan), "margin must be finite"),
                      (dict(ttc_thr=np.inf), "ttc_thr must be finite"), (dict(r_ego=[0.0, np.inf]), "planner 1: r_ego must be finite"),
                      (dict(on=[1, 2]), "planner 1: on must be 0 or 1"), (dict(tick0=-1), "tick0")):
        with pytest.raises(BackendError, match=text):
            fleet.sim_safety(**dict(PAR, **bad))
    with pytest.raises(ValueError):
        fleet.sim_safety(bogus=1.0)
    fleet.sim_safety(**PAR)
    d, inc = fleet.sim_safety_read()
    assert np.all(d["ticks"] == 0) and np.all(d["ttc_min"] == np.inf) and np.all(np.isnan(inc))
    one = dict(pose=[(0.0, 0.0)], dt=[0.05], tick=[0], params=[list(sim.SAFETY_DEFAULTS[k] for k in sim.SAFETY_PARAMS)], objs=[np.zeros((0, 5))])
    for kw, text in ((dict(dt=[0.0]), "dt"), (dict(tick=[-1]), "tick"), (dict(params=[[1.5, -1.0, 1.0, 1.0, 0.5]]), "ttc_thr"),
                     (dict(objs=[np.zeros((97, 5))]), "0 .. 96 objects")):
        a = dict(one, **kw)
        with pytest.raises(BackendError, match=text):
            fleet.sim_safety_eval(a["pose"], a["dt"], a["tick"], a["params"], a["objs"])
    fleet.close()
