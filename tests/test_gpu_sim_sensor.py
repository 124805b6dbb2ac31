"""
GPU: the sensor model of the fleet's closed-loop simulation (ltpl_fleet_sim_sensor / _sensor_read / _sensor_eval; csrc/fleet_sensor.hpp,
k_fleet_sim_sense / k_fleet_sim_sensor_eval in csrc/fleet_sim.hpp) against its host mirror (sim.SensorModel) and the sensing host loops of
tests/sim_sensor_util.py --

  1. the hook: causes and dropout draws bit for bit against the mirror on the cases of sim_sensor_util.cases, in batches of 1, 63, 64 and
     65 cases and all at once;
  2. seated lockstep differentials (the host loop re-seated on the device's own state every tick, as in tests/test_gpu_sim_noise.py) on
     the scenarios of sim_sensor_util.scenarios: the count handed on, the recorder's objects, trace [5] .. [7] and the statistics records,
     bitwise (the recorder's objects of the noisy run within that file's 1e-12); the same run as ONE sim_run call equals the single ticks
     bit for bit, records included. tests/test_sim_sensor_host.py asserts that no object of these scenarios comes within 1e-9 of the
     cone's boundary, so the device's sin / cos excuse nothing;
  3. identity: the open sensor, the sensor switched off again and a fresh sim_setup leave the trace bit-identical to a fleet that never
     made the call;
  4. telemetry against truth: an object the sensor never shows comes close; telemetry's clear_min and the sensor's blind_clear_min agree;
  5. layout independence: a planner alone and at index 5 of 70 computes the same records;
  6. tick0: 20 ticks in one run equal 10 ticks, sim_sensor(tick0=10), 10 ticks;
  7. snapshot, restore and branch leave configuration and statistics the destination's;
  8. every refusal, and a refused call keeps the previous sensor and its records.
"""
import os

import numpy as np
import pytest

import planner_replay as pr
import sim_sensor_util as su
import test_gpu_sim_differential as gd
import test_gpu_sim_noise as gn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12                     # tests/test_gpu_sim_noise.py: the recorder's objects of a noisy run


@pytest.fixture(scope="module")
def hip(monteblanco):
    from graphbasedlocaltrajectoryplanner_amd import _capi
    return _capi.HipBackend(monteblanco)


@pytest.fixture(scope="module")
def table():
    from graphbasedlocaltrajectoryplanner_amd.sim import RaceLineTable
    return RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


@pytest.fixture(scope="module")
def track():
    return np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz"))


@pytest.fixture(scope="module")
def c2_start():
    return pr.load_ticks("c2")[0]['start']


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


# ---- 1. the hook --------------------------------------------------------------------------------------------------------------------------
def test_the_hook_equals_the_mirror_bit_for_bit(hip):
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    cs, groups = su.cases()
    ref = [su.mirror(c) for c in cs]
    fleet = Fleet(hip, 1)

    def run(idx):
        sub = [cs[i] for i in idx]
        return fleet.sim_sensor_eval([c["pose"] for c in sub], [c["f"] for c in sub], [c["params"] for c in sub],
                                     np.array([c["seed"] for c in sub], np.uint64), np.array([c["tick"] for c in sub], np.uint32),
                                     [np.array(c["objs"], float).reshape(-1, 3) for c in sub])
    n = len(cs)
    assert n >= 1 + 63 + 64 + 65                             # (the four batches do not overlap)
    causes = [None] * n
    for idx in (list(range(n)), [0], list(range(1, 64)), list(range(64, 128)), list(range(n - 65, n))):       # all, then 1, 63, 64 and 65 cases
        got_c, got_u = run(idx)
        for i, c, u in zip(idx, got_c, got_u):
            assert c.tolist() == ref[i][0], "case %d: device %s, mirror %s" % (i, c.tolist(), ref[i][0])
            assert np.array_equal(bits(u), bits(ref[i][1])), "case %d: u" % i
            causes[i] = c.tolist()
    su.check_straddles(cs, groups, causes)
    assert fleet.sim_sensor_eval(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 5)), 0, 0, []) == ([], [])
    fleet.close()


# ---- 2. seated lockstep -------------------------------------------------------------------------------------------------------------------
def sensor_fleet(sc, hip, kw, kind="plain", tick0=0):
    fleet = sc.fleet(hip)
    if kind == "vehicle":
        if max(sc.sizes) == 1:
            fleet.sim_race([1] * sc.n)                      # (hands heading0 = the start heading to the simulation)
        fleet.sim_vehicle(model=1)
    if kind == "noise":
        fleet.sim_noise(**su.noise_args(sc.n))
    if kw is not None:
        fleet.sim_sensor(tick0=tick0, **kw)
    return fleet


def lockstep(sc, hip, oracle, n_ticks, kw, kind, what):
    from graphbasedlocaltrajectoryplanner_amd.planner import KEY_IDS, KEY_NAMES
    fleet, loop = sensor_fleet(sc, hip, kw, kind), su.host_loop(sc, oracle, kw, kind)
    fleet.sim_record(list(range(sc.n)), depth=1)
    prev_traj = [None] * sc.n
    traces, stats = [], dict(max_all=0, max_cnt=0, lost=np.zeros(5, int), lost_low=0, lost_high=0, worst_obj=0.0)
    for k in range(n_ticks):
        st, th = fleet.sim_state(), fleet.sim_heading()
        vr = fleet.sim_vehicle_read(raw=True) if kind == "vehicle" else None
        for p in range(sc.n):
            a, b = sc.opp_off[p], sc.opp_off[p + 1]
            loop.seat(p, st['now'][p], st['pos_est'][p], st['vel_est'][p], th[p], st['opp_s'][a:b], st['opp_tic'][a:b], prev_traj[p])
            if vr is not None:
                loop.seat_vehicle(p, vr[p])
        tr = fleet.sim_run(1)[0][0]
        traces.append(tr.copy())
        st2, th2 = fleet.sim_state(), fleet.sim_heading()
        rec_dev, dev_stats = fleet.sim_record_read()[-1], fleet.sim_sensor_read(raw=True)
        recs = loop.step_sim()
        post = {}
        for p in range(sc.n):
            w, r = "%s tick %d planner %d" % (what, k, p), recs[p]
            assert tr[p, 8] == 0 and not r["failed"], w
            assert tr[p, 0] == KEY_IDS[r["sel"]] and tr[p, 1] == r["now"] == st2['now'][p], "%s: action / clock" % w
            post[p] = dict(sel=KEY_NAMES.get(int(st2['sel_action'][p])), now=st2['now'][p], pos=st2['pos_est'][p], vel=st2['vel_est'][p], theta=th2[p])
        recs = loop.step_plan(post=post)
        for p in range(sc.n):
            w, r = "%s tick %d planner %d" % (what, k, p), recs[p]
            assert not r["failed"], "%s: %s" % (w, r.get("error"))
            dev_veh = rec_dev[p]["vehicles"]
            assert tr[p, 5] == r["cnt"] == len(dev_veh), "%s: objects handed on: trace %s, recorder %d, host %d of %d (causes %s)" % (
                w, tr[p, 5], len(dev_veh), r["cnt"], len(r["veh_all"]), r["causes"])
            for i, ((rad, v, xy), (hrad, hv, hxy)) in enumerate(zip(dev_veh, r["veh"])):
                if kind == "noise":
                    d = max(abs(rad - hrad), abs(v - hv), float(np.max(np.abs(xy - hxy))))
                    assert d <= TOL, "%s: object %d differs by %g" % (w, i, d)
                    stats['worst_obj'] = max(stats['worst_obj'], d)
                else:
                    assert rad == hrad and v == hv and np.array_equal(xy, hxy), "%s: object %d: %s %s %s vs %s %s %s" % (w, i, rad, v, xy, hrad, hv, hxy)
            if r["cnt"]:
                assert np.array_equal(tr[p, 6:8], dev_veh[0][2][0]), "%s: first vehicle of the trace vs the recorder" % w
                if kind == "noise":
                    assert float(np.max(np.abs(tr[p, 6:8] - r["first"]))) <= TOL, "%s: first vehicle %s vs %s" % (w, tr[p, 6:8], r["first"])
                else:
                    assert np.array_equal(tr[p, 6:8], r["first"]), "%s: first vehicle %s vs %s" % (w, tr[p, 6:8], r["first"])
            else:
                assert np.all(np.isnan(tr[p, 6:8])), w
            assert np.array_equal(bits(dev_stats[p]), bits(loop.sensor.rec[p])), "%s: statistics: device %s, mirror %s" % (w, dev_stats[p], loop.sensor.rec[p])
            prev_traj[p] = fleet.trajectories(p)[0]
            c = np.asarray(r["causes"], int)
            stats['lost'] += np.bincount(c, minlength=5)
            stats['lost_low'] += int(np.sum(c[:64] != 0))
            stats['lost_high'] += int(np.sum(c[64:] != 0))
            stats['max_all'], stats['max_cnt'] = max(stats['max_all'], len(c)), max(stats['max_cnt'], r["cnt"])
    final = (fleet.sim_state(), fleet.sim_heading(), fleet.digest(), fleet.sim_sensor_read(raw=True))
    fleet.close()
    # the same scenario in one call: bitwise the single ticks, digest and records included
    fleet = sensor_fleet(sc, hip, kw, kind)
    one = fleet.sim_run(n_ticks)[0]
    assert np.array_equal(one, np.array(traces), equal_nan=True), "%s: one call differs from the single ticks" % what
    st = fleet.sim_state()
    assert all(np.array_equal(st[key], final[0][key]) for key in st) and np.array_equal(fleet.sim_heading(), final[1])
    assert np.array_equal(fleet.digest(), final[2]) and np.array_equal(bits(fleet.sim_sensor_read(raw=True)), bits(final[3]))
    fleet.close()
    print("\n%s: %d ticks x %d planners against the sensing host loop; up to %d objects on the track, up to %d handed on; seen / range / cone / "
          "occlusion / dropout %s; lost below / from slot 64: %d / %d; records %s" % (
              what, n_ticks, sc.n, stats['max_all'], stats['max_cnt'], stats['lost'].tolist(), stats['lost_low'], stats['lost_high'], final[3].tolist()))
    return stats


@pytest.mark.parametrize("index", range(5))
def test_lockstep_against_the_sensing_host_loop(hip, monteblanco, oracle_backend, table, track, c2_start, index):
    name, units, kw, ticks, kind = su.scenarios(table, track, c2_start)[index]
    sc = gd.Scenario(monteblanco, table, units)
    assert sc.n <= 8 and ticks <= 80
    stats = lockstep(sc, hip, oracle_backend, ticks, kw, kind, name)
    assert stats['lost'][0] > 0 and np.sum(stats['lost'][1:]) > 0, stats
    if name == "crowd":
        assert stats['max_all'] >= 70 and stats['lost_low'] > 0 and stats['lost_high'] > 0, stats
    if name == "three singles":                              # far opponents and statics beyond the ranges; the draws
        assert np.all(stats['lost'][[1, 4]] > 0), stats
    if name == "race of 3":                                  # the mates behind a car are outside its cone, the far mate stands behind the near one
        assert np.all(stats['lost'][[2, 3]] > 0), stats


# ---- 3. identity --------------------------------------------------------------------------------------------------------------------------
def test_open_cleared_and_fresh_setup_leave_the_trace_untouched(hip, monteblanco, table, track, c2_start):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    sc = gd.Scenario(monteblanco, table, gn.mixed(table, track, c2_start))
    plain = sc.fleet(hip)
    ref = plain.sim_run(30)[0]
    ref_state, ref_digest = plain.sim_state(), plain.digest()
    plain.close()
    kw = su.sensor_args(sc.n)
    opened = sc.fleet(hip)
    opened.sim_sensor()                                      # the open sensor: every object kept
    cleared = sensor_fleet(sc, hip, kw)
    cleared.sim_sensor(None)
    for what, fleet in (("open", opened), ("set, then cleared", cleared)):
        tr = fleet.sim_run(30)[0]
        assert np.array_equal(tr, ref, equal_nan=True), what
        st = fleet.sim_state()
        assert all(np.array_equal(st[k], ref_state[k]) for k in st) and np.array_equal(fleet.digest(), ref_digest), what
    d = opened.sim_sensor_read()
    assert np.all(d["ticks"] == 30) and np.array_equal(d["n_obj"], d["n_seen"]) and np.all(d["blind_ticks"] == 0) and np.all(np.isinf(d["blind_clear_min"]))
    assert np.array_equal(d["n_obj"], ref[:, :, 5].sum(axis=0).astype(np.int64))
    with pytest.raises(BackendError, match="the sensor is off"):
        cleared.sim_sensor_read()
    # sim_setup switches the sensor off
    opened.sim_sensor(**kw)
    opened.sim_setup(sc.tab, sc.entries, dt=sc.dt, n_export=sc.n_export)
    with pytest.raises(BackendError, match="the sensor is off"):
        opened.sim_sensor_read()
    opened.close()
    cleared.close()
    # and the sensor is not a no-op on this scenario
    sensed = sensor_fleet(sc, hip, kw)
    assert not np.array_equal(sensed.sim_run(30)[0], ref, equal_nan=True)
    sensed.close()


# ---- 4. telemetry against truth -----------------------------------------------------------------------------------------------------------
def test_telemetry_and_the_sensor_agree_on_an_object_that_is_never_shown(hip, monteblanco, table, c2_start):
    sc = gd.Scenario(monteblanco, table, [gn.tele_unit(table, c2_start)])
    fleet = sc.fleet(hip)
    fleet.sim_telemetry(radius=gn.TELE_RADIUS)
    fleet.sim_sensor(range=1.0)                              # the only object stands 14 m ahead: never shown
    trace = fleet.sim_run(30)[0]
    tele, sens = fleet.sim_telemetry_read(), fleet.sim_sensor_read()
    fleet.close()
    print("telemetry clear_min %r at tick %d, contacts %d; sensor blind_clear_min %r at tick %d; lost to range %d" % (
        tele["clear_min"][0], tele["clear_tick"][0], tele["contact_ticks"][0], sens["blind_clear_min"][0], sens["blind_clear_tick"][0], sens["n_range"][0]))
    assert np.all(trace[:, 0, 8] == 0) and np.all(trace[:, 0, 5] == 0) and np.all(np.isnan(trace[:, 0, 6:8]))
    assert sens["n_obj"][0] == sens["n_range"][0] >= 25 and sens["n_seen"][0] == 0 and sens["blind_ticks"][0] == sens["n_obj"][0]
    assert np.isfinite(sens["blind_clear_min"][0]) and bits(tele["clear_min"])[0] == bits(sens["blind_clear_min"])[0]
    assert tele["clear_tick"][0] == sens["blind_clear_tick"][0] and tele["contact_ticks"][0] > 0


# ---- 5. layout independence ---------------------------------------------------------------------------------------------------------------
def test_a_planner_computes_the_same_alone_and_at_index_5_of_70(hip, monteblanco, table, track, c2_start):
    s = gn.singles(table, track, c2_start)
    one = dict(range=200.0, fov_deg=220.0, r_near=0.0, occl=2.0, p_drop=0.25, seed=0xC0FFEE0123456789)
    alone = sensor_fleet(gd.Scenario(monteblanco, table, [s[0]]), hip, one)
    ref = alone.sim_run(30)[0]
    ref_rec = alone.sim_sensor_read(raw=True)
    alone.close()
    units = [s[k % 3] for k in (1, 2, 1, 2, 1)] + [s[0]] + [s[k % 3] for k in range(64)]
    sc = gd.Scenario(monteblanco, table, units)
    assert sc.n == 70
    kw = su.sensor_args(70)
    for k, v in one.items():
        kw[k] = np.array(np.broadcast_to(kw[k], (70,)))
        kw[k][5] = v
    fleet = sensor_fleet(sc, hip, kw)
    tr = fleet.sim_run(30)[0]
    rec = fleet.sim_sensor_read(raw=True)
    fleet.close()
    assert np.array_equal(tr[:, 5], ref[:, 0], equal_nan=True) and np.array_equal(bits(rec[5]), bits(ref_rec[0]))
    assert ref_rec[0, 2] < ref_rec[0, 1] and not np.array_equal(rec[6], rec[5])          # objects were lost; planner 6 (the same unit) has other parameters
    two = sensor_fleet(gd.Scenario(monteblanco, table, [s[1], s[0]]), hip, {k: np.array([kw[k][4], v], dtype=kw[k].dtype) for k, v in one.items()})
    tr2 = two.sim_run(30)[0]
    assert np.array_equal(tr2[:, 1], ref[:, 0], equal_nan=True) and np.array_equal(bits(two.sim_sensor_read(raw=True)[1]), bits(ref_rec[0]))
    two.close()


# ---- 6. tick0 -----------------------------------------------------------------------------------------------------------------------------
def test_tick0_continues_the_dropout_decisions(hip, monteblanco, table, track, c2_start):
    sc = gd.Scenario(monteblanco, table, gn.mixed(table, track, c2_start))
    kw = dict(su.sensor_args(sc.n, seed0=31), p_drop=0.3)
    whole = sensor_fleet(sc, hip, kw)
    ref = whole.sim_run(20)[0]
    ref_rec = whole.sim_sensor_read()
    whole.close()
    assert np.sum(ref_rec["n_drop"]) > 0
    fleet = sensor_fleet(sc, hip, kw)
    a = fleet.sim_run(10)[0]
    first = fleet.sim_sensor_read()
    fleet.sim_snapshot(0)
    fleet.sim_sensor(tick0=10, **kw)
    assert np.all(fleet.sim_sensor_read()["ticks"] == 0)     # a successful call starts the statistics anew
    b = fleet.sim_run(10)[0]
    second = fleet.sim_sensor_read()
    assert np.array_equal(np.concatenate((a, b)), ref, equal_nan=True)
    for key in ("ticks", "n_obj", "n_seen", "n_range", "n_fov", "n_occl", "n_drop", "blind_ticks"):
        assert np.array_equal(first[key] + second[key], ref_rec[key]), key
    assert np.array_equal(np.minimum(first["blind_clear_min"], second["blind_clear_min"]), ref_rec["blind_clear_min"])
    assert np.all((second["blind_clear_tick"] >= 10) | (second["blind_clear_tick"] == -1))
    # without tick0 the second half is another one
    fleet.sim_restore(0)
    fleet.sim_sensor(**kw)
    assert not np.array_equal(fleet.sim_run(10)[0], ref[10:], equal_nan=True)
    fleet.close()


# ---- 7. snapshot, restore, branch ---------------------------------------------------------------------------------------------------------
def test_snapshot_and_branch_leave_configuration_and_statistics_alone(hip, monteblanco, table, track, c2_start):
    s = gn.singles(table, track, c2_start)
    sc = gd.Scenario(monteblanco, table, [s[0], s[0], s[1]])
    kw = dict(range=[150.0, 0.0, 150.0], fov_deg=220.0, occl=2.0, p_drop=[0.2, 0.0, 0.2], seed=[11, 12, 13])
    fleet = sensor_fleet(sc, hip, kw)
    fleet.sim_run(10)
    fleet.sim_snapshot(0)
    after10 = fleet.sim_sensor_read(raw=True)
    ref = fleet.sim_run(10)[0]
    after20 = fleet.sim_sensor_read(raw=True)
    assert np.all(after20[:, 0] == 20)
    fleet.sim_restore(0)
    assert np.array_equal(bits(fleet.sim_sensor_read(raw=True)), bits(after20))          # the statistics are not rolled back
    fleet.sim_sensor(tick0=10, **kw)
    again = fleet.sim_run(10)[0]
    assert np.array_equal(again, ref, equal_nan=True)        # the restored state under the same sensor ticks: the same second half
    assert np.array_equal(bits(fleet.sim_sensor_read(raw=True)[:, 1:8]), bits((after20 - after10)[:, 1:8]))
    # planner 1 (range 0: blind) takes planner 0's state: it stays blind, and its record goes on counting its own
    before = fleet.sim_sensor_read(raw=True)
    fleet.sim_branch([0], [1])
    assert np.array_equal(bits(fleet.sim_sensor_read(raw=True)), bits(before))
    tr = fleet.sim_run(5)[0]
    rec = fleet.sim_sensor_read()
    assert np.all(tr[:, 1, 5] == 0) and rec["ticks"][1] == 15 and rec["n_seen"][1] == 0 and rec["n_range"][1] == rec["n_obj"][1] > 0
    assert rec["n_seen"][0] > 0
    fleet.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_keep_the_previous_sensor_and_its_records(hip, monteblanco, table, track, c2_start):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    bare = Fleet(hip, 2)
    for call in (lambda: bare.sim_sensor(range=10.0), lambda: bare.sim_sensor(None), lambda: bare.sim_sensor_read()):
        with pytest.raises(BackendError, match="sim_setup first"):
            call()
    with pytest.raises(BackendError, match="0 .. 96 objects"):
        bare.sim_sensor_eval([(0.0, 0.0)], [(0.0, 1.0)], [[1.0, 0.0, -1.0, 0.0, 0.0]], 0, 0, [np.zeros((97, 3))])
    bare.close()
    sc = gd.Scenario(monteblanco, table, gn.singles(table, track, c2_start)[:2])
    kw = dict(su.sensor_args(2, seed0=5), range=[0.0, 150.0])
    fleet = sensor_fleet(sc, hip, kw)
    ticks = 0

    def still_in_force():
        nonlocal ticks
        before = fleet.sim_sensor_read(raw=True)
        tr = fleet.sim_run(1)[0][0]
        ticks += 1
        rec = fleet.sim_sensor_read()
        assert np.all(rec["ticks"] == ticks) and np.all(before[:, 0] == ticks - 1)
        assert tr[0, 5] == 0 and rec["n_seen"][0] == 0 and rec["n_range"][0] == rec["n_obj"][0] > 0       # planner 0 has range 0
    still_in_force()
    nan, inf = float("nan"), float("inf")
    bad = [(dict(range=nan), "range"), (dict(range=-1.0), "range"), (dict(range=[150.0, -inf]), "range"),
           (dict(r_near=-0.1), "r_near"), (dict(r_near=[0.0, 150.5]), "r_near"), (dict(r_near=nan), "r_near"),
           (dict(fov_deg=nan), "fov_cos"), (dict(occl=-1.0), "occl"), (dict(occl=inf), "occl"), (dict(occl=nan), "occl"),
           (dict(p_drop=1.0), "p_drop"), (dict(p_drop=-0.01), "p_drop"), (dict(p_drop=nan), "p_drop"), (dict(tick0=-1), "tick0")]
    for args, msg in bad:
        with pytest.raises(BackendError, match=msg):
            fleet.sim_sensor(**dict(dict(range=150.0, r_near=0.0), **args))
        still_in_force()
    fleet.close()
