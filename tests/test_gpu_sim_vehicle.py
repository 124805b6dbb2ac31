"""
GPU: the vehicle model of the fleet's simulation (ltpl_fleet_sim_vehicle: k_fleet_sim_step_veh / k_fleet_sim_step_noise_veh in
csrc/fleet_sim.hpp over csrc/fleet_vehicle.hpp) against its host mirror sim.VehicleModel and the host loop of
tests/sim_vehicle_util.py over the oracle's planner --

  1. the test hook (one wave per case, the tick's own device function) equals the mirror BIT FOR BIT on the CPU suite's cases and on row
     counts on both sides of every 64-lane stride with the nearest segment in the first lane, the last lane and the last partial stride,
     in batches of 1, 63, 64 and 65 cases; the heading within 1e-12 of math.atan2;
  2. seated lockstep as in tests/test_gpu_sim_differential.py: 8 planners x 80 ticks -- 'empty', 'one', 'emerg_second', a recorded race
     of 4 and a second 'one' -- with models mixed 0 / 1. Per tick the host is seated on sim_state, sim_heading and sim_vehicle_read;
     vehicle state and statistics bitwise, pose and speed of a model planner bitwise its record, theta within 1e-12, the planner's part
     within the existing tolerances, errors on the same tick on both sides; then the same scenario in ONE sim_run call, bitwise;
  3. identity: model all 0 is bitwise a fleet without the call; in a mixed fleet the planners outside any race with model 0 likewise;
  4. interplay: the noise estimate is the noise added to the model's true pose; mates see the model's pose, speed and heading; a
     branched planner continues bitwise like its source; sim_restore returns state and statistics; keep_state with a lowered grip
     continues from the same state and saturates more; every refusal of the argument check, each leaving the previous setting intact.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import sim_vehicle_util as vu
import test_gpu_sim_differential as gd
from fleet_differential import same_paths, same_trajectories

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12                     # tests/test_gpu_sim_differential.py


@pytest.fixture(scope="module")
def hip(monteblanco):
    from graphbasedlocaltrajectoryplanner_amd import _capi
    return _capi.HipBackend(monteblanco)


@pytest.fixture(scope="module")
def table():
    from graphbasedlocaltrajectoryplanner_amd.sim import RaceLineTable
    return RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


@pytest.fixture(scope="module")
def c2_start():
    return pr.load_ticks("c2")[0]['start']


@pytest.fixture(scope="module")
def classes(table, c2_start):
    return sl.monteblanco_classes(table, np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")), tuple(c2_start['pos']))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


# ---- 1. the hook ------------------------------------------------------------------------------------------------------------------------
def test_the_hook_equals_the_mirror_bit_for_bit(hip, oracle_backend):
    from graphbasedlocaltrajectoryplanner_amd import sim
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    cases = vu.cases() + vu.stride_cases()
    assert sorted(set(c["rows"].shape[0] for c in cases if "nearest" in c)) == list(vu.STRIDE_ROWS)
    for c in cases:
        if "nearest" in c:                                    # the segment the case is named after wins the first projection
            cols = sim.VehicleModel.columns(c["rows"])
            d2 = [sim.VehicleModel._seg(cols[1], cols[2], i, c["state"][0], c["state"][1])[0] for i in range(c["rows"].shape[0] - 1)]
            assert int(np.argmin(d2)) == c["nearest"], c["name"]
    assert {0, 63, 254} <= set(c["nearest"] for c in cases if "nearest" in c)
    ref = [vu.mirror_tick(c) for c in cases]
    fleet = Fleet(hip, 1)

    def run(sub):
        return fleet.sim_vehicle_step([c["state"] for c in sub], [c["par"] for c in sub], [c["rows"] for c in sub], [c["dt"] for c in sub],
                                      [c["ctl"] for c in sub])
    out, theta = run(cases)
    assert out.shape == (len(cases), sim.VEHICLE_DOUBLES) and len(cases) > 65
    for k, c in enumerate(cases):
        assert np.array_equal(bits(out[k, :14]), bits(ref[k][0])), "%s: %s vs %s" % (c["name"], out[k, :14], ref[k][0])
        assert gd.wrapped(theta[k] - ref[k][1]) <= 1e-12, "%s: heading %r vs %r" % (c["name"], theta[k], ref[k][1])
    # the track test of the pose at the end: the object ingestion's (none of these lines lies on Monteblanco but the ones through its start)
    on = oracle_backend.process_objects(out[:, 0].copy(), out[:, 1].copy(), np.zeros(len(cases)), np.zeros(len(cases)), np.zeros(len(cases)), 0.2)["on_track"]
    assert np.array_equal(out[:, 14], 1.0 - on.astype(float))
    for m in (1, 63, 64, 65):
        o, t = run(cases[:m])
        assert np.array_equal(bits(o), bits(out[:m])) and np.array_equal(bits(t), bits(theta[:m])), m
    o, t = fleet.sim_vehicle_step(np.zeros((0, 7)), np.zeros((0, 9)), [], 0.05, 10)
    assert o.shape == (0, sim.VEHICLE_DOUBLES) and t.shape == (0,)
    fleet.close()


# ---- scenarios --------------------------------------------------------------------------------------------------------------------------
def eight(classes, start):
    """'empty', 'one', 'emerg_second', the recorded race of 4 and a second 'one' (a class of its own: every planner is compared in full)."""
    return [gd.single("empty", classes["empty"], start), gd.single("one", classes["one"], start),
            gd.single("emerg_second", classes["emerg_second"], start), gd.recorded_race("race4"), gd.single("one_b", classes["one"], start)]


MODEL8 = [1, 1, 1, 1, 0, 1, 1, 0]       # the race of 4 (planners 3 .. 6) mixes both; 'one' drives the model, 'one_b' the ideal tracker


def vehicle_fleet(sc, hip, model, **par):
    fleet = sc.fleet(hip)
    if max(sc.sizes) == 1:
        fleet.sim_race([1] * sc.n)                          # (hands heading0 = the start heading to the simulation)
    if model is not None:
        fleet.sim_vehicle(model=model, **par)
    return fleet


def vehicle_host(sc, oracle, model, **par):
    """``Scenario.host`` with the vehicle loop over the scenario's host planners."""
    from oracle.planner_host import HostPlannerBackend
    backend = HostPlannerBackend(sc.lat)
    loop = vu.VehicleSimLoop(sc.lat, sc.tab, [sc.entries[p] for p in sc.hmap], [backend.planner(1, **sc.config) for _ in sc.hmap],
                             oracle=oracle, dt=sc.dt, n_export=sc.n_export)
    for h, p in enumerate(sc.hmap):
        pos, heading, vel, mho = sc.starts[p]
        assert loop.set_start(h, pos, heading, vel, mho)[0], p
        loop.sim_vel(h, **sc.vels[p])
    loop.sim_race([sc.sizes[i] for i in sc.host_units], length=5.0)
    loop.sim_vehicle(model=np.asarray(model)[sc.hmap], **par)
    return loop


# ---- 2. seated lockstep -----------------------------------------------------------------------------------------------------------------
def test_eight_planners_in_lockstep_and_in_one_call(hip, monteblanco, oracle_backend, classes, table, c2_start):
    from graphbasedlocaltrajectoryplanner_amd import sim
    from graphbasedlocaltrajectoryplanner_amd.planner import KEY_IDS, KEY_NAMES
    n_ticks, what = 80, "vehicle lockstep"
    sc = gd.Scenario(monteblanco, table, eight(classes, c2_start))
    assert sc.n == 8 and sc.hmap == list(range(8))          # every planner is compared in full
    fleet, loop = vehicle_fleet(sc, hip, MODEL8), vehicle_host(sc, oracle_backend, MODEL8)
    rec0 = fleet.sim_vehicle_read(raw=True)
    for p in range(8):                                      # the state the call set: the start pose, (c, s) of the start heading
        if MODEL8[p]:
            assert np.array_equal(bits(rec0[p]), bits(loop.veh[p].record())), p
        else:
            assert np.all(np.isnan(rec0[p])) and loop.veh[p] is None
    prev_traj = [None] * 8
    traces, worst, stats = [], dict(theta=0.0, ideal=0.0), dict(keys=set(), errors=0, sat=0)
    for k in range(n_ticks):
        st, th, vr = fleet.sim_state(), fleet.sim_heading(), fleet.sim_vehicle_read(raw=True)
        for p in range(8):
            a, b = sc.opp_off[p], sc.opp_off[p + 1]
            loop.seat(p, st['now'][p], st['pos_est'][p], st['vel_est'][p], th[p], st['opp_s'][a:b], st['opp_tic'][a:b], prev_traj[p])
            loop.seat_vehicle(p, vr[p])
        tr = gd.run_one(fleet, 1)[0]
        traces.append(tr.copy())
        st2, th2, vr2 = fleet.sim_state(), fleet.sim_heading(), fleet.sim_vehicle_read(raw=True)
        recs = loop.step_sim()
        post = {}
        for p in range(8):
            w, r = "%s tick %d planner %d" % (what, k, p), recs[p]
            dev_failed = tr[p, 8] != 0
            if r["action_failed"] or (r["failed"] and dev_failed):
                assert dev_failed, "%s: the host fails (no matching action), the device does not" % w
            else:
                assert not r["failed"], "%s: failed on the host in an earlier tick only" % w
                assert tr[p, 0] == KEY_IDS[r["sel"]] and tr[p, 1] == r["now"] == st2['now'][p], "%s: action / clock" % w
            if MODEL8[p]:
                assert np.array_equal(bits(vr2[p]), bits(loop.veh[p].record())), "%s: vehicle record %s vs %s" % (w, vr2[p], loop.veh[p].record())
                if not dev_failed and k > 0:               # pose and speed ARE the record's (the tick before the first trajectory moves nothing)
                    assert list(st2['pos_est'][p]) == [vr2[p, 0], vr2[p, 1]] and st2['vel_est'][p] == vr2[p, 4], "%s: pose vs record" % w
                d = float(gd.wrapped(th2[p] - r["theta"]))
                assert d <= TOL, "%s: heading differs by %g" % (w, d)
                worst['theta'] = max(worst['theta'], d)
                assert list(st2['pos_est'][p]) == r["pos"] and st2['vel_est'][p] == r["vel"], "%s: pose %s vs %s" % (w, st2['pos_est'][p], r["pos"])
            else:
                assert np.all(np.isnan(vr2[p])), w
                d = max(float(np.max(np.abs(st2['pos_est'][p] - r["pos"]))), abs(st2['vel_est'][p] - r["vel"]) / max(abs(r["vel"]), 1.0),
                        float(gd.wrapped(th2[p] - r["theta"])))
                assert d <= TOL, "%s: tracked state differs by %g" % (w, d)
                worst['ideal'] = max(worst['ideal'], d)
            a, b = sc.opp_off[p], sc.opp_off[p + 1]
            assert b == a or float(np.max(np.abs(st2['opp_s'][a:b] - r["opp_s"]))) <= TOL, "%s: opponents" % w
            assert np.array_equal(tr[p, 2:5], [st2['pos_est'][p, 0], st2['pos_est'][p, 1], st2['vel_est'][p]]) or dev_failed, "%s: trace vs state" % w
            post[p] = dict(sel=KEY_NAMES.get(int(st2['sel_action'][p])), now=st2['now'][p], pos=st2['pos_est'][p], vel=st2['vel_est'][p], theta=th2[p])
        recs = loop.step_plan(post=post, want_paths=True)
        for p in range(8):
            w, r = "%s tick %d planner %d" % (what, k, p), recs[p]
            dev_failed = tr[p, 8] != 0
            assert bool(r["failed"]) == bool(dev_failed), "%s: error on the %s only (%s)" % (w, "host" if r["failed"] else "device", r.get("error", tr[p, 8]))
            if r["failed"]:
                stats['errors'] += 1
                continue
            assert tr[p, 5] == r["cnt"], "%s: on-track objects %s vs %d" % (w, tr[p, 5], r["cnt"])
            if r["cnt"]:
                assert float(np.max(np.abs(tr[p, 6:8] - r["first"]))) <= TOL, "%s: first vehicle %s vs %s" % (w, tr[p, 6:8], r["first"])
            same_paths(fleet.paths(p), r["paths"], exact=False, what=w)
            dev_traj = fleet.trajectories(p)
            same_trajectories(dev_traj, r["traj"], exact=False, what=w)
            prev_traj[p] = dev_traj[0]
            stats['keys'].add(r["sel"])
    final = (fleet.sim_state(), fleet.sim_heading(), fleet.digest(), fleet.sim_vehicle_read(raw=True))
    fleet.close()
    vd = {name: final[3][:, i] for name, i, _ in sim.VEHICLE_FIELDS}
    on = np.array(MODEL8, bool)
    assert np.all(vd["ctl_steps"][on] >= (n_ticks - 2) * 5) and np.all(vd["e_max"][on] > 0.0)
    # the same scenario in one call: bitwise the single ticks, digest and vehicle records included
    fleet = vehicle_fleet(sc, hip, MODEL8)
    one = gd.run_one(fleet, n_ticks)
    assert np.array_equal(one, np.array(traces), equal_nan=True), "%s: one call differs from the single ticks" % what
    st = fleet.sim_state()
    assert all(np.array_equal(st[key], final[0][key]) for key in st) and np.array_equal(fleet.sim_heading(), final[1])
    assert np.array_equal(fleet.digest(), final[2]) and np.array_equal(bits(fleet.sim_vehicle_read(raw=True)), bits(final[3]))
    fleet.close()
    print("\n%s: %d ticks x 8 planners (models %s); actions %s, %d planner-ticks in error on both sides; largest differences %s; e_max %s m" %
          (what, n_ticks, MODEL8, sorted(stats['keys']), stats['errors'], worst, np.round(vd["e_max"][on], 3)))
    assert {"straight", "follow"} <= stats['keys'], stats


# ---- 3. identity ------------------------------------------------------------------------------------------------------------------------
def test_model_zero_is_the_fleet_without_the_call(hip, monteblanco, classes, table, c2_start):
    sc = gd.Scenario(monteblanco, table, eight(classes, c2_start))
    plain = vehicle_fleet(sc, hip, None)
    ref = gd.run_one(plain, 40)
    ref_state, ref_heading, ref_digest = plain.sim_state(), plain.sim_heading(), plain.digest()
    plain.close()
    zero = vehicle_fleet(sc, hip, 0)
    tr = gd.run_one(zero, 40)
    st = zero.sim_state()
    assert np.array_equal(tr, ref, equal_nan=True)
    assert all(np.array_equal(st[k], ref_state[k]) for k in st) and np.array_equal(zero.sim_heading(), ref_heading) and np.array_equal(zero.digest(), ref_digest)
    assert np.all(np.isnan(zero.sim_vehicle_read(raw=True)))
    zero.sim_vehicle(None)                                   # and switched off again: the plain kernels, the same ticks
    with pytest.raises(Exception, match="the model is off"):
        zero.sim_vehicle_read()
    zero.close()
    # a mixed fleet: the planners outside any race with model 0 -- here 'empty' and 'one_b' -- compute bit for bit what they compute without the call
    model = [0, 1, 1, 1, 0, 1, 1, 0]
    mixed = vehicle_fleet(sc, hip, model)
    tr = gd.run_one(mixed, 40)
    st = mixed.sim_state()
    for p in (0, 7):
        assert np.array_equal(tr[:, p], ref[:, p], equal_nan=True), p
        assert all(np.array_equal(st[k][p], ref_state[k][p]) for k in ("pos_est", "vel_est", "sel_action", "now")) and mixed.sim_heading()[p] == ref_heading[p]
    assert not np.array_equal(tr[:, 1], ref[:, 1], equal_nan=True)      # (and the model is no no-op on 'one')
    mixed.close()


# ---- 4. interplay ------------------------------------------------------------------------------------------------------------------------
def test_noise_is_added_to_the_models_true_pose(hip, monteblanco, classes, table, c2_start):
    from graphbasedlocaltrajectoryplanner_amd import sim
    sc = gd.Scenario(monteblanco, table, [gd.single("one", classes["one"], c2_start), gd.single("empty", classes["empty"], c2_start)])
    fleet = vehicle_fleet(sc, hip, 1)
    kw = dict(seed=[11, 2 ** 63 + 5], pos=0.2, vel=0.3, obj_pos=0.3, obj_theta=0.02, obj_vel=0.5)
    fleet.sim_noise(**kw)
    nm = sim.NoiseModel(2, **kw)
    for k in range(30):
        fleet.sim_run(1)
        st, est, vr = fleet.sim_state(), fleet.sim_estimate(), fleet.sim_vehicle_read(raw=True)
        for p in range(2):
            if k > 0:
                assert list(st['pos_est'][p]) == [vr[p, 0], vr[p, 1]] and st['vel_est'][p] == vr[p, 4]
            pos, vel = nm.ego(p, k, st['pos_est'][p], st['vel_est'][p])
            assert list(est['pos_est'][p]) == pos and est['vel_est'][p] == vel and pos != list(st['pos_est'][p]), (k, p)
    assert np.all(vr[:, 11] >= 29 * 5) and np.all(vr[:, 4] > 1.0)
    fleet.close()


def test_mates_see_the_models_pose_speed_and_heading(hip, monteblanco, table):
    sc = gd.Scenario(monteblanco, table, [gd.race_unit("race2", *sl.big_race(table, 2, gap=25.0))])
    fleet = vehicle_fleet(sc, hip, 1)
    fleet.sim_record([0, 1], depth=1)
    start = fleet.sim_vehicle_read(raw=True)[:, :2]
    for k in range(30):
        tr = fleet.sim_run(1)[0][0]
        vr, th, rec = fleet.sim_vehicle_read(raw=True), fleet.sim_heading(), fleet.sim_record_read()[-1]
        for p, q in ((0, 1), (1, 0)):
            assert tr[p, 5] == 1 and list(tr[p, 6:8]) == [vr[q, 0], vr[q, 1]], (k, p)
            rad, v, xy = rec[p]["vehicles"][0]
            assert v == vr[q, 4] and list(xy[0]) == [vr[q, 0], vr[q, 1]] and rad == 2.5
            pred = [vr[q, 0] - math.sin(th[q]) * v * 0.2, vr[q, 1] + math.cos(th[q]) * v * 0.2]     # ObjectListInterface.py:117-133 with the heading handed on
            assert np.max(np.abs(xy[1] - pred)) <= 1e-12 and gd.wrapped(th[q] - math.atan2(-vr[q, 2], vr[q, 3])) <= 1e-12, (k, p)
    print("\nmates: speeds %s m/s, moved %s m" % (vr[:, 4], np.hypot(vr[:, 0] - start[:, 0], vr[:, 1] - start[:, 1])))
    assert np.any(vr[:, 4] > 1.0) and np.all(vr[:, 11] >= 29 * 5)       # (the cars drive: what the mates see changes from tick to tick)
    fleet.close()


def two_ones(classes, start, v1=5.0):
    """Two planners of class 'one', the second started at another speed (its state differs, its configuration does not)."""
    b = dict(classes["one"], entry=dict(classes["one"]["entry"], vel_est=v1), start_vel=v1)
    return [gd.single("one", classes["one"], start), gd.single("one_fast", b, start)]


def test_branch_restore_and_keep_state(hip, monteblanco, classes, table, c2_start):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    sc = gd.Scenario(monteblanco, table, two_ones(classes, c2_start))
    fleet = vehicle_fleet(sc, hip, 1)
    fleet.sim_run(25)
    vr = fleet.sim_vehicle_read(raw=True)
    assert not np.array_equal(vr[0], vr[1])
    # a branched planner continues bitwise like its source
    fleet.sim_branch(0, [1])
    assert np.array_equal(bits(fleet.sim_vehicle_read(raw=True)[1]), bits(vr[0]))
    fleet.sim_snapshot(2)
    tr = fleet.sim_run(25)[0]
    assert np.array_equal(tr[:, 1], tr[:, 0], equal_nan=True)
    after = (fleet.sim_state(), fleet.sim_vehicle_read(raw=True), fleet.digest())
    assert np.array_equal(bits(after[1][0]), bits(after[1][1])) and after[1][0, 11] > vr[0, 11]
    # sim_restore returns state and statistics; the continuation repeats bit for bit
    fleet.sim_restore(2)
    back = fleet.sim_vehicle_read(raw=True)
    assert np.array_equal(bits(back[0]), bits(vr[0])) and np.array_equal(bits(back[1]), bits(vr[0]))
    tr2 = fleet.sim_run(25)[0]
    assert np.array_equal(tr2, tr, equal_nan=True) and np.array_equal(bits(fleet.sim_vehicle_read(raw=True)), bits(after[1]))
    assert np.array_equal(fleet.digest(), after[2])
    # keep_state with a lowered grip: the same state and statistics, then more saturation than the run above from the same snapshot
    fleet.sim_restore(2)
    fleet.sim_vehicle(model=1, keep_state=True, grip=0.5)
    assert np.array_equal(bits(fleet.sim_vehicle_read(raw=True)), bits(back))
    fleet.sim_run(25)
    low = fleet.sim_vehicle_read(raw=True)
    assert np.all(low[:, 12] + low[:, 13] > after[1][:, 12] + after[1][:, 13]), (low[:, 12:14], after[1][:, 12:14])
    # without keep_state the call starts from the present pose with cleared statistics
    st, th = fleet.sim_state(), fleet.sim_heading()
    fleet.sim_vehicle(model=[1, 0])
    fresh = fleet.sim_vehicle_read(raw=True)
    assert list(fresh[0, :2]) == list(st['pos_est'][0]) and fresh[0, 4] == st['vel_est'][0] and np.all(fresh[0, 5:] == 0.0) and np.all(np.isnan(fresh[1]))
    assert fresh[0, 2] == -math.sin(th[0]) and fresh[0, 3] == math.cos(th[0])
    # mixed pairs: a destination on the ideal tracker takes no vehicle record; a destination with the model needs a source that has one
    fleet.sim_branch(0, [1])
    assert np.all(np.isnan(fleet.sim_vehicle_read(raw=True)[1]))
    with pytest.raises(BackendError, match="no vehicle state"):
        fleet.sim_branch(1, [0])
    fleet.sim_snapshot(3, [1])                               # (planner 1 on the ideal tracker)
    fleet.sim_vehicle(model=1, keep_state=True)
    with pytest.raises(BackendError, match="no vehicle state"):
        fleet.sim_branch([1], [1], snapshot=3)
    assert np.array_equal(bits(fleet.sim_vehicle_read(raw=True)[0]), bits(fresh[0]))
    fleet.sim_run(3)
    fleet.close()


def test_every_refusal_leaves_the_previous_setting_intact(hip, monteblanco, classes, table, c2_start):
    from graphbasedlocaltrajectoryplanner_amd import sim
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet, SimVehicleIn
    bare = Fleet(hip, 2)
    with pytest.raises(BackendError, match="ltpl_fleet_sim_setup first"):
        bare.sim_vehicle()
    with pytest.raises(BackendError, match="ltpl_fleet_sim_setup first"):
        bare.sim_vehicle_read()
    c = vu.cases()[0]

    def step(**kw):
        a = dict(state=[c["state"]], par=[c["par"]], rows=[c["rows"]], dt=0.05, ctl=10)
        a.update(kw)
        return bare.sim_vehicle_step(a["state"], a["par"], a["rows"], a["dt"], a["ctl"])
    for kw, msg in ((dict(rows=[np.zeros((257, 5))]), "0 .. 256 rows"), (dict(dt=0.0), "dt must lie"), (dict(dt=1.5), "dt must lie"),
                    (dict(dt=float("nan")), "dt must lie"), (dict(ctl=0), "ctl_steps must be at least 1")):
        with pytest.raises(BackendError, match=msg):
            step(**kw)
    assert step()[0].shape == (1, sim.VEHICLE_DOUBLES)
    bare.close()

    sc = gd.Scenario(monteblanco, table, two_ones(classes, c2_start))
    fleet = vehicle_fleet(sc, hip, [1, 0], grip=0.9)
    fleet.sim_run(12)
    before = fleet.sim_vehicle_read(raw=True)
    refusals = [(dict(model=[1, 2]), "planner 1: model must be 0 or 1"), (dict(model=-1), "planner 0: model must be 0 or 1"),
                (dict(ctl_steps=0), "ctl_steps must be at least 1"), (dict(tau_a=0.0009), "planner 0: tau_a must be at least 0.001"),
                (dict(model=1, tau_kappa=[0.08, 0.0005]), "planner 1: tau_kappa must be at least 0.001")]
    for name in sim.VEHICLE_PARAMS:
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refusals.append(({name: bad}, "planner 0: %s must be finite and positive" % name))
        refusals.append((dict(model=1, **{name: [1.0, -2.0]}), "planner 1: %s must be finite and positive" % name))
    for kw, msg in refusals:
        with pytest.raises(BackendError, match=msg):
            fleet.sim_vehicle(**dict(dict(model=[1, 0]), **kw))
    fleet.sim_vehicle(model=[1, 0], keep_state=True, grip=0.9, **{k: [sim.VEHICLE_DEFAULTS[k], float("nan")] for k in ("ax_max", "tau_a")})    # (model 0: its parameters are not read)
    # the struct itself: an unknown flag, a missing array
    keep = [np.ascontiguousarray(np.array([1, 0], np.int32))] + [np.full(2, sim.VEHICLE_DEFAULTS[k]) for k in sim.VEHICLE_PARAMS]

    def raw(flags=1, missing=None):
        vi = SimVehicleIn()
        vi.model, vi.ctl_steps, vi.flags = keep[0].ctypes.data, 10, flags
        for a, name in zip(keep[1:], sim.VEHICLE_PARAMS):
            setattr(vi, name, None if name == missing else a.ctypes.data)
        if missing == "model":
            vi.model = None
        fleet._check(fleet._fn("sim_vehicle")(fleet.handle, C.byref(vi)))
    with pytest.raises(BackendError, match="unknown flag"):
        raw(flags=2)
    for name in ("model",) + sim.VEHICLE_PARAMS:
        with pytest.raises(BackendError, match="%s missing" % name):
            raw(missing=name)
    out = np.zeros((2, sim.VEHICLE_DOUBLES + 1))
    with pytest.raises(BackendError, match="record size mismatch"):
        fleet._check(fleet._fn("sim_vehicle_read")(fleet.handle, out.ctypes.data, sim.VEHICLE_DOUBLES + 1))
    with pytest.raises(TypeError):
        fleet.sim_vehicle(gripp=1.0)
    # nothing moved: state and statistics as before, and the next ticks are those of a fleet that never saw a refused call
    assert np.array_equal(bits(fleet.sim_vehicle_read(raw=True)), bits(before))
    tr = fleet.sim_run(12)[0]
    twin = vehicle_fleet(sc, hip, [1, 0], grip=0.9)
    ref = twin.sim_run(24)[0]
    assert np.array_equal(tr, ref[12:], equal_nan=True) and np.array_equal(bits(fleet.sim_vehicle_read(raw=True)), bits(twin.sim_vehicle_read(raw=True)))
    twin.close()
    fleet.close()
