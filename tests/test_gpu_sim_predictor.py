"""
GPU: the prediction model of the fleet's closed-loop simulation (ltpl_fleet_sim_predictor / _predictor_read / _predictor_eval;
csrc/fleet_predict.hpp, k_fleet_sim_predict / k_fleet_sim_predictor_eval in csrc/fleet_sim.hpp) against its host mirror
(sim.PredictorModel) and the predicting host loop of tests/sim_predictor_util.py --

  1. the hook: positions, outcomes and counters bit for bit against the mirror on the whole case list of sim_predictor_util.cases (the
     boundaries of the rule, K = 1 .. 8, the object counts at which cnt K crosses a pass of 64 pairs, the capacity edge cnt (1 + K) = 192)
     and, through a second fleet, on a table with a duplicated row;
  2. equivalence: K = 1 and K = 4 with every planner in mode 0, a predictor set and cleared, and a fleet that never had one give
     bit-identical traces, digests included;
  3. seated lockstep (the host loop re-seated on the device's own state every tick) on the scenarios of sim_predictor_util.scenarios:
     counts, the recorder's objects (own position and point 1), trace [5] .. [7], tracker tables where a tracker runs, bitwise; the discrete
     fields of the planners' digests; the statistics records equal the mirror's (6.); the same run as ONE sim_run call equals the single
     ticks bit for bit;
  4. the prediction matters: scenario A in mode 0 and in mode 2 over 2 s differ in trace and in recorded paths;
  5. a planner computes the same alone and at index 5 of 70;
  7. snapshot, restore and branch leave configuration and records alone;
  8. with K = 4 a recorded tick's objects show own position and point 1;
  and every refusal keeps the previous predictor.
"""
import os

import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import sim_predictor_util as pu
import sim_tracker_util as tu
import test_gpu_sim_differential as gd
import test_gpu_sim_noise as gn
from graphbasedlocaltrajectoryplanner_amd import sim

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


ENTRY = dict(opponents=[(250.0, 0.3, 5.0)], static=[], pref=sl.DEFAULT_PREF, pos_est=(0.0, 0.0), vel_est=0.0, zone_gids=[])


# ---- 1. the hook --------------------------------------------------------------------------------------------------------------------------
def hook_against_mirror(fleet, tab, cs, what):
    done = 0
    for K in sorted({c["K"] for c in cs}):
        idx = [i for i, c in enumerate(cs) if c["K"] == K]
        pos, oc, rec = fleet.sim_predictor_eval(K, [cs[i]["params"] for i in idx], [cs[i]["objs"] for i in idx])
        for j, i in enumerate(idx):
            pu.compare(dict(pos=pos[j], outcome=oc[j], rec=rec[j]), pu.mirror(tab, cs[i]), "%s case %d (K = %d, %d objects)" % (what, i, K, len(cs[i]["objs"])))
            done += 1
    return done


def test_the_hook_equals_the_mirror_bit_for_bit(hip, table):
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    cs, groups = pu.cases(table)
    assert {c["K"] for c in cs} == set(range(1, 9))
    assert {(13, 5), (16, 8), (43, 3), (0, 4), (1, 4), (96, 1), (64, 2)} <= {(len(c["objs"]), c["K"]) for c in cs}
    fleet = Fleet(hip, 1)
    fleet.sim_setup(table, [ENTRY])
    assert hook_against_mirror(fleet, table, cs, "Monteblanco") == len(cs)
    pos, oc, rec = fleet.sim_predictor_eval(3, np.zeros((0, 4)), [])
    assert pos == [] and oc == [] and rec.shape[0] == 0
    fleet.close()
    # a table with a duplicated row: a second small fleet set up on it
    dtab = pu.dup_table(table)
    small = Fleet(hip, 1)
    small.sim_setup(dtab, [ENTRY])
    dc = pu.dup_cases(dtab)
    assert hook_against_mirror(small, dtab, dc, "duplicated row") == len(dc)
    small.close()


# ---- 2. equivalence -----------------------------------------------------------------------------------------------------------------------
def test_mode_0_and_a_cleared_predictor_equal_a_fleet_without_one(hip, monteblanco, table, track, c2_start):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    sc = gd.Scenario(monteblanco, table, gn.mixed(table, track, c2_start))
    plain = sc.fleet(hip)
    ref = plain.sim_run(20)[0]
    ref_state, ref_digest = plain.sim_state(), plain.digest()
    plain.close()
    for what, K in (("K = 1, mode 0", 1), ("K = 4, mode 0", 4), ("set, then cleared", None)):
        fleet = sc.fleet(hip)
        fleet.sim_predictor(n_points=K or 3, mode=0 if K else 2, horizon=2.5)
        if K is None:
            fleet.sim_predictor(None)
        tr = fleet.sim_run(20)[0]
        st = fleet.sim_state()
        assert np.array_equal(bits(tr), bits(ref)), what
        assert all(np.array_equal(st[k], ref_state[k]) for k in st) and np.array_equal(fleet.digest(), ref_digest), what
        if K is None:
            with pytest.raises(BackendError, match="the predictor is off"):
                fleet.sim_predictor_read()
        else:
            d = fleet.sim_predictor_read()
            assert np.all(d["ticks"] == 20) and np.array_equal(d["n_ingested"], d["n_obj"]) and np.array_equal(d["n_obj"], ref[:, :, 5].sum(axis=0))
        fleet.close()
    # sim_setup switches the predictor off; sim_race keeps it
    fleet = sc.fleet(hip)
    fleet.sim_predictor(n_points=2)
    fleet.sim_setup(sc.tab, sc.entries, dt=sc.dt, n_export=sc.n_export)
    with pytest.raises(BackendError, match="the predictor is off"):
        fleet.sim_predictor_read()
    fleet.sim_predictor(n_points=2)
    fleet.sim_race(sc.sizes, length=5.0)
    assert np.all(fleet.sim_predictor_read()["ticks"] == 0)
    fleet.close()


# ---- 3. and 6. seated lockstep, the records ---------------------------------------------------------------------------------------------------
def predictor_fleet(sc, hip, skw, tkw, pkw):
    fleet = sc.fleet(hip)
    if skw is not None:
        fleet.sim_sensor(**skw)
    if tkw is not None:
        fleet.sim_tracker(**tkw)
    if pkw is not None:
        fleet.sim_predictor(**pkw)
    return fleet


def lockstep(sc, hip, oracle, n_ticks, skw, tkw, pkw, what):
    from graphbasedlocaltrajectoryplanner_amd.planner import KEY_IDS, KEY_NAMES
    fleet, loop = predictor_fleet(sc, hip, skw, tkw, pkw), pu.host_loop(sc, oracle, skw, tkw, pkw)
    fleet.sim_record(list(range(sc.n)), depth=1)
    prev_traj = [None] * sc.n
    traces, worst, n_obj = [], 0.0, 0

    def same(a, b, w):
        nonlocal worst
        a, b = np.asarray(a, float), np.asarray(b, float)
        assert a.shape == b.shape, "%s: shapes %s, %s" % (w, a.shape, b.shape)
        if a.size:
            worst = max(worst, float(np.nanmax(np.abs(a - b))))
        assert np.array_equal(bits(a), bits(b)), "%s: device %s, host %s" % (w, a, b)
    for k in range(n_ticks):
        st, th = fleet.sim_state(), fleet.sim_heading()
        for p in range(sc.n):
            a, b = sc.opp_off[p], sc.opp_off[p + 1]
            loop.seat(p, st['now'][p], st['pos_est'][p], st['vel_est'][p], th[p], st['opp_s'][a:b], st['opp_tic'][a:b], prev_traj[p])
        tr = fleet.sim_run(1)[0][0]
        traces.append(tr.copy())
        st2, th2 = fleet.sim_state(), fleet.sim_heading()
        rec_dev = fleet.sim_record_read()[-1]
        dev_rec = fleet.sim_predictor_read(raw=True)
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
            assert tr[p, 5] == r["cnt"] == len(dev_veh), "%s: objects handed on: trace %s, recorder %d, host %d" % (w, tr[p, 5], len(dev_veh), r["cnt"])
            for i, ((rad, v, xy), (hrad, hv, hxy)) in enumerate(zip(dev_veh, r["veh"])):
                assert np.asarray(hxy).shape == (1 + pkw["n_points"], 2), w
                same([rad, v] + list(np.ravel(xy)), [hrad, hv] + list(np.ravel(np.asarray(hxy)[:2])), "%s: object %d (own position and point 1)" % (w, i))
            n_obj += r["cnt"]
            if r["cnt"]:
                assert np.array_equal(tr[p, 6:8], dev_veh[0][2][0]), "%s: first vehicle of the trace vs the recorder" % w
            else:
                assert np.all(np.isnan(tr[p, 6:8])), w
            assert np.array_equal(bits(dev_rec[p]), bits(loop.predictor.rec[p])), "%s: statistics: device %s, mirror %s" % (w, dev_rec[p], loop.predictor.rec[p])
            dg = sl.digest_row(dict(r, failed=False))
            assert np.array_equal(tr[p, 8:][[0, 3, 4]], dg[[0, 3, 4]]), "%s: digest %s vs %s" % (w, tr[p, 8:16], dg[:8])
            prev_traj[p] = fleet.trajectories(p)[0]
        if tkw is not None:
            dev_stats, dev_tabs, dev_cnt = fleet.sim_tracker_read(planners=list(range(sc.n)), raw=True)
            for p in range(sc.n):
                m = loop.trackers[p]
                assert dev_cnt[p] == len(m.tracks) and np.array_equal(bits(dev_tabs[p]), bits(m.table())) and np.array_equal(bits(dev_stats[p]), bits(m.rec)), \
                    "%s tick %d planner %d: tracker table" % (what, k, p)
    final = (fleet.sim_state(), fleet.sim_heading(), fleet.digest(), fleet.sim_predictor_read(raw=True))
    fleet.close()
    # the same scenario in one call: bitwise the single ticks, digest and records included
    fleet = predictor_fleet(sc, hip, skw, tkw, pkw)
    one = fleet.sim_run(n_ticks)[0]
    assert np.array_equal(one, np.array(traces), equal_nan=True), "%s: one call differs from the single ticks" % what
    st = fleet.sim_state()
    assert all(np.array_equal(st[key], final[0][key]) for key in st) and np.array_equal(fleet.sim_heading(), final[1])
    assert np.array_equal(fleet.digest(), final[2]) and np.array_equal(bits(fleet.sim_predictor_read(raw=True)), bits(final[3]))
    fleet.close()
    rec = sim.predictor_dict(final[3])
    print("\n%s: %d ticks x %d planners against the predicting host loop, %d objects; largest deviation %.3g; records %s" % (
        what, n_ticks, sc.n, n_obj, worst, {k: v.tolist() for k, v in rec.items()}))
    return rec, worst, np.array(traces)


@pytest.mark.parametrize("index", range(3))
def test_lockstep_against_the_predicting_host_loop(hip, monteblanco, oracle_backend, table, track, c2_start, index):
    name, units, skw, tkw, pkw, ticks = pu.scenarios(table, track, c2_start)[index]
    sc = gd.Scenario(monteblanco, table, units)
    assert sc.n <= 4 and ticks <= 30
    rec, worst, _ = lockstep(sc, hip, oracle_backend, ticks, skw, tkw, pkw, name)
    assert worst == 0.0
    assert np.all(rec["ticks"] == ticks) and rec["n_obj"].sum() > 0
    assert np.array_equal(rec["n_obj"], sum(rec[k] for k in ("n_ingested", "n_still", "n_straight_mode", "n_straight_dmax", "n_straight_dir",
                                                              "n_straight_noseg", "n_track")))
    if index == 0:
        assert rec["n_track"][0] > 0 and rec["d_abs_max"][0] > 3.0            # the car beside the race line
    if index == 1:
        assert rec["n_straight_dmax"].sum() > 0 and rec["n_track"].sum() > 0, rec
    if index == 2:
        assert rec["n_ingested"][0] > 0 and rec["n_straight_mode"][1] > 0 and rec["n_track"][2] + rec["n_straight_dmax"][2] > 0
        assert rec["n_ingested"][1] == rec["n_ingested"][2] == 0


# ---- 4. the prediction matters ------------------------------------------------------------------------------------------------------------
def test_the_prediction_changes_trace_and_paths(hip, monteblanco, table, c2_start):
    sc = gd.Scenario(monteblanco, table, [pu.bend_unit(table, c2_start)])
    out = {}
    for mode in (0, 2):
        fleet = predictor_fleet(sc, hip, None, None, dict(pu.A_PRED, mode=mode))
        fleet.sim_record([0], depth=25)
        tr = fleet.sim_run(25)[0]
        assert np.all(tr[:, 0, 8] == 0)
        out[mode] = (tr, [r[0] for r in fleet.sim_record_read()], fleet.sim_predictor_read())
        fleet.close()
    (tr0, rec0, d0), (tr2, rec2, d2) = out[0], out[2]
    trace_differs = [k for k in range(25) if not np.array_equal(bits(tr0[k]), bits(tr2[k]))]
    paths_differ = [k for k in range(25) if (rec0[k]["paths"]["keys"], rec0[k]["paths"]["nodes"]) != (rec2[k]["paths"]["keys"], rec2[k]["paths"]["nodes"])]
    print("ticks whose trace differs: %s; whose paths differ: %s; actions as ingested %s, along the track %s" % (
        trace_differs, paths_differ, [r["sel"] for r in rec0][::4], [r["sel"] for r in rec2][::4]))
    assert trace_differs and paths_differ
    # as ingested the planner finds a way past the car beside the race line; its prediction onto the race line takes that way
    assert any("right" in r["paths"]["keys"] for r in rec0) and not any("right" in r["paths"]["keys"] for r in rec2[:5])
    assert d0["n_ingested"][0] == d0["n_obj"][0] > 0 and d2["n_track"][0] > 0 and d2["n_ingested"][0] == 0


# ---- 5. independence ----------------------------------------------------------------------------------------------------------------------
def test_a_planner_computes_the_same_alone_and_at_index_5_of_70(hip, monteblanco, table, track, c2_start):
    singles = gn.singles(table, track, c2_start)
    unit = pu.bend_unit(table, c2_start)
    units = [singles[i % 3] for i in range(70)]
    units[5] = unit
    n_ticks = 10
    par = dict(n_points=4, horizon=2.0, relax=0.5, d_max=pu.INF)
    alone = predictor_fleet(gd.Scenario(monteblanco, table, [unit]), hip, None, None, dict(par, mode=2))
    a = alone.sim_run(n_ticks)[0][:, 0]
    ra = alone.sim_predictor_read(raw=True)[0]
    alone.close()
    mode = np.arange(70) % 3
    mode[5] = 2
    crowd = predictor_fleet(gd.Scenario(monteblanco, table, units), hip, None, None, dict(par, mode=mode))
    b = crowd.sim_run(n_ticks)[0][:, 5]
    rb = crowd.sim_predictor_read(raw=True)
    crowd.close()
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(ra), bits(rb[5]))
    assert np.all(rb[:, 0] == n_ticks) and rb[5, 8] > 0


# ---- 7. snapshot, restore, branch ---------------------------------------------------------------------------------------------------------
def test_snapshot_restore_and_branch_leave_configuration_and_records_alone(hip, monteblanco, table, track, c2_start):
    sc = gd.Scenario(monteblanco, table, gn.singles(table, track, c2_start)[:2])
    pkw = dict(n_points=3, mode=[2, 1], horizon=[2.0, 1.0], relax=0.25, d_max=pu.INF)
    fleet = predictor_fleet(sc, hip, None, None, pkw)
    fleet.sim_run(5)
    fleet.sim_snapshot(0)
    rec5 = fleet.sim_predictor_read(raw=True)
    ref = fleet.sim_run(5)[0]
    rec10 = fleet.sim_predictor_read(raw=True)
    fleet.sim_restore(0)
    assert np.array_equal(bits(fleet.sim_predictor_read(raw=True)), bits(rec10))          # not rolled back
    again = fleet.sim_run(5)[0]
    assert np.array_equal(again, ref, equal_nan=True)                                       # the same configuration: the run repeats
    rec15 = fleet.sim_predictor_read(raw=True)
    cnt = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10]
    assert np.array_equal(bits((rec15 - rec10)[:, cnt]), bits((rec10 - rec5)[:, cnt])) and np.all(rec15[:, 0] == 15)
    fleet.sim_branch([0], [1])
    assert np.array_equal(bits(fleet.sim_predictor_read(raw=True)), bits(rec15))
    fleet.sim_run(3)
    d = fleet.sim_predictor_read()
    assert np.all(d["ticks"] == 18) and d["n_straight_mode"][1] > 0 and d["n_track"][1] == 0 and d["n_straight_mode"][0] == 0    # each keeps its own mode
    fleet.close()


# ---- 8. the recorder ----------------------------------------------------------------------------------------------------------------------
def test_a_recorded_tick_shows_own_position_and_point_1(hip, monteblanco, table, c2_start):
    sc = gd.Scenario(monteblanco, table, [pu.bend_unit(table, c2_start)])
    shown = {}
    for mode in (0, 2):
        fleet = predictor_fleet(sc, hip, None, None, dict(pu.A_PRED, mode=mode))
        fleet.sim_record([0], depth=2)
        fleet.sim_run(1)
        shown[mode] = fleet.sim_record_read()[-1][0]["vehicles"]
        fleet.close()
    # the first tick's objects are the same in both fleets; mode 0 shows own position and the ingestion's point
    assert len(shown[0]) == len(shown[2]) == 3
    objs = [(xy[0, 0], xy[0, 1], xy[1, 0], xy[1, 1], v) for _, v, xy in shown[0]]
    pts, ocs = sim.PredictorModel(1, table, **pu.A_PRED).predict(0, objs)
    assert sim.PRED_TRACK in ocs
    for i, (rad, v, xy) in enumerate(shown[2]):
        assert xy.shape == (2, 2) and (rad, v) == (shown[0][i][0], shown[0][i][1])
        assert np.array_equal(bits(xy[0]), bits(objs[i][:2])) and np.array_equal(bits(xy[1]), bits(pts[i, 0])), i


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_keep_the_previous_predictor(hip, monteblanco, table, track, c2_start):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    bare = Fleet(hip, 2)
    for call in (lambda: bare.sim_predictor(), lambda: bare.sim_predictor(None), lambda: bare.sim_predictor_read(),
                 lambda: bare.sim_predictor_eval(2, [[2.0, 1.0, 0.0, 1.0]], [np.zeros((1, 5))])):
        with pytest.raises(BackendError, match="sim_setup first"):
            call()
    bare.close()
    sc = gd.Scenario(monteblanco, table, gn.singles(table, track, c2_start)[:2])
    fleet = predictor_fleet(sc, hip, None, None, dict(n_points=2, mode=[0, 2], horizon=1.0))
    ticks = 0

    def still_in_force():
        nonlocal ticks
        fleet.sim_run(1)
        ticks += 1
        d = fleet.sim_predictor_read()
        assert np.all(d["ticks"] == ticks) and d["n_ingested"][0] == d["n_obj"][0] > 0 and d["n_ingested"][1] == 0
    still_in_force()
    nan, inf = float("nan"), float("inf")
    bad = [(dict(n_points=0), "n_points"), (dict(n_points=9), "n_points"), (dict(mode=3), "mode"), (dict(mode=[0, -1]), "mode"),
           (dict(horizon=0.0), "horizon"), (dict(horizon=nan), "horizon"), (dict(horizon=[1.0, inf]), "horizon"),
           (dict(relax=-0.1), "relax"), (dict(relax=1.5), "relax"), (dict(relax=nan), "relax"), (dict(d_max=-1.0), "d_max"), (dict(d_max=nan), "d_max")]
    for args, msg in bad:
        with pytest.raises(BackendError, match=msg):
            fleet.sim_predictor(**args)
        still_in_force()
    for kw, msg in ((dict(n_points=0, params=[[2.0, 1.0, 0.0, 1.0]], objs=[np.zeros((1, 5))]), "n_points"),
                    (dict(n_points=2, params=[[2.0, 1.0, 0.0, 1.0]], objs=[np.zeros((97, 5))]), "0 .. 96 objects"),
                    (dict(n_points=2, params=[[5.0, 1.0, 0.0, 1.0]], objs=[np.zeros((1, 5))]), "mode")):
        with pytest.raises(BackendError, match=msg):
            fleet.sim_predictor_eval(**kw)
    fleet.close()
    # the capacity bound: 3 slots each; K = 8 gives 27 positions -- far from 192: only a crowded planner reaches it
    crowd = gd.Scenario(monteblanco, table, [tu.su.crowd(table, track, c2_start)])
    fleet = crowd.fleet(hip)
    fleet.sim_predictor(n_points=1, mode=2)                                    # 96 x 2 = 192
    with pytest.raises(BackendError, match="above 192"):
        fleet.sim_predictor(n_points=2)
    tr = fleet.sim_run(2)[0]
    d = fleet.sim_predictor_read()
    assert np.all(tr[:, 0, 8] == 0) and d["ticks"][0] == 2 and d["n_obj"][0] == tr[:, 0, 5].sum() > 128
    fleet.close()
