"""
GPU: the object tracker of the fleet's closed-loop simulation (ltpl_fleet_sim_tracker / _tracker_read / _tracker_eval; csrc/fleet_track.hpp,
k_fleet_sim_track / k_fleet_sim_tracker_eval in csrc/fleet_sim.hpp) against its host mirror (sim.TrackerModel) and the tracking host loops of
tests/sim_tracker_util.py --

  1. the hook: tables, lists handed on, assignments, counters and next_id bit for bit against the mirror on the whole case table of
     sim_tracker_util.cases, all at once and in batches of 1, 63, 64 and 65 cases;
  2. seated lockstep differentials (the host loop re-seated on the device's own state every tick) on the scenarios of
     sim_tracker_util.scenarios: the count handed on, the recorder's objects, trace [5] .. [7], the tables and the statistics records,
     bitwise; the discrete fields of the planners' digests; the same run as ONE sim_run call equals the single ticks bit for bit. The noisy
     scenario: discrete outputs (counts, ids, hits, misses, born ticks, records) exactly, values within NOISE_TOL (measured, see there);
  3. telemetry keeps measuring truth behind a tracker that hands on nothing;
  4. tick0 is the born_tick of the first tracks;
  5. a planner that is not live keeps its table while the tracker tick advances;
  6. snapshot / restore / branch carry table and next_id: a restored run repeats bitwise; a source without tracker state empties the table;
     a source with more tracks than the destination's capacity is refused;
  7. every refusal; a refused call keeps the previous tracker and its tables;
  8. sim_tracker(gate=None) followed by a run, and a fresh sim_setup, equal a fleet that never had a tracker, bitwise.
"""
import os

import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import sim_tracker_util as tu
import test_gpu_sim_differential as gd
import test_gpu_sim_noise as gn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENSOR_TOL = 1e-12              # tests/test_gpu_sim_sensor.py: the recorder's objects of a noisy run
# The noisy scenario's values against the host loop: the largest deviation measured on an MI355X is NOISE_MEASURED (printed by the test;
# DESIGN.md 4.5c); the bound is four times the larger of that and SENSOR_TOL
NOISE_MEASURED = 0.0
NOISE_TOL = 4.0 * max(NOISE_MEASURED, SENSOR_TOL)


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
    cs, groups = tu.cases()
    ref = [tu.mirror(c) for c in cs]
    fleet = Fleet(hip, 1)
    n = len(cs)
    assert n >= 1 + 63 + 64 + 65                             # (the four batches do not overlap)
    done = np.zeros(n, int)
    for idx in (list(range(n)), [0], list(range(1, 64)), list(range(64, 128)), list(range(n - 65, n))):       # all, then 1, 63, 64 and 65 cases
        sub = [cs[i] for i in idx]
        got = fleet.sim_tracker_eval([c["params"] for c in sub], [c["adv"] for c in sub], [c["tick"] for c in sub], [c["cap"] for c in sub],
                                     [c["slots"] for c in sub], [c["tracks"] for c in sub], [c["next_id"] for c in sub], [c["dets"] for c in sub])
        for j, i in enumerate(idx):
            dev = dict(table=got["tables"][j], n_tracks=int(got["n_tracks"][j]), next_id=float(got["next_id"][j]), out=got["out"][j],
                       assign=got["assign"][j].tolist(), rec=got["rec"][j])
            tu.compare(dev, ref[i], "case %d (batch of %d)" % (i, len(idx)))
            done[i] += 1
    assert np.all(done >= 1)
    empty = fleet.sim_tracker_eval(np.zeros((0, 5)), [], [], [], [], [], [], [])
    assert empty["out"] == [] and empty["tables"].shape[0] == 0
    fleet.close()


# ---- 2. seated lockstep -------------------------------------------------------------------------------------------------------------------
def tracker_fleet(sc, hip, skw, tkw, kind="plain", tick0=0):
    fleet = sc.fleet(hip)
    if kind == "vehicle":
        if max(sc.sizes) == 1:
            fleet.sim_race([1] * sc.n)                      # (hands heading0 = the start heading to the simulation)
        fleet.sim_vehicle(model=1)
    if kind == "noise":
        fleet.sim_noise(**tu.su.noise_args(sc.n))
    if skw is not None:
        fleet.sim_sensor(**skw)
    if tkw is not None:
        fleet.sim_tracker(tick0=tick0, **tkw)
    return fleet


DISCRETE = [6, 7, 8, 9]         # id, hits, miss, born_tick of a table row


def lockstep(sc, hip, oracle, n_ticks, skw, tkw, kind, what):
    from graphbasedlocaltrajectoryplanner_amd.planner import KEY_IDS, KEY_NAMES
    fleet, loop = tracker_fleet(sc, hip, skw, tkw, kind), tu.host_loop(sc, oracle, skw, tkw, kind)
    fleet.sim_record(list(range(sc.n)), depth=1)
    prev_traj = [None] * sc.n
    traces = []
    stats = dict(max_det=0, max_out=0, match_low=0, match_high=0, worst=0.0, coast_out=0)
    noisy = kind == "noise"

    def close(a, b, w):
        a, b = np.asarray(a, float), np.asarray(b, float)
        assert a.shape == b.shape, "%s: shapes %s, %s" % (w, a.shape, b.shape)
        if noisy:
            d = float(np.max(np.abs(a - b))) if a.size else 0.0
            stats['worst'] = max(stats['worst'], d)
            assert d <= NOISE_TOL, "%s differs by %g" % (w, d)
        else:
            assert np.array_equal(bits(a), bits(b)), "%s: device %s, host %s" % (w, a, b)
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
        rec_dev = fleet.sim_record_read()[-1]
        dev_stats, dev_tabs, dev_cnt = fleet.sim_tracker_read(planners=list(range(sc.n)), raw=True)
        recs = loop.step_sim()
        post = {}
        for p in range(sc.n):
            w, r = "%s tick %d planner %d" % (what, k, p), recs[p]
            assert tr[p, 8] == 0 and not r["failed"], w
            assert tr[p, 0] == KEY_IDS[r["sel"]] and tr[p, 1] == r["now"] == st2['now'][p], "%s: action / clock" % w
            post[p] = dict(sel=KEY_NAMES.get(int(st2['sel_action'][p])), now=st2['now'][p], pos=st2['pos_est'][p], vel=st2['vel_est'][p], theta=th2[p])
        recs = loop.step_plan(post=post)
        for p in range(sc.n):
            w, r, m = "%s tick %d planner %d" % (what, k, p), recs[p], loop.trackers[p]
            assert not r["failed"], "%s: %s" % (w, r.get("error"))
            dev_veh = rec_dev[p]["vehicles"]
            assert tr[p, 5] == r["cnt"] == len(dev_veh), "%s: objects handed on: trace %s, recorder %d, host %d of %d detections" % (
                w, tr[p, 5], len(dev_veh), r["cnt"], len(r["dets"]))
            for i, ((rad, v, xy), (hrad, hv, hxy)) in enumerate(zip(dev_veh, r["veh"])):
                close([rad, v] + list(np.ravel(xy)), [hrad, hv] + list(np.ravel(hxy)), "%s: object %d" % (w, i))
            if r["cnt"]:
                assert np.array_equal(tr[p, 6:8], dev_veh[0][2][0]), "%s: first vehicle of the trace vs the recorder" % w
                close(tr[p, 6:8], r["first"], "%s: first vehicle" % w)
            else:
                assert np.all(np.isnan(tr[p, 6:8])), w
            # the table: the discrete columns exactly, the values bitwise (with noise: within the bound)
            assert dev_cnt[p] == len(m.tracks), "%s: %d tracks, mirror %d" % (w, dev_cnt[p], len(m.tracks))
            host_tab = m.table()
            assert np.array_equal(bits(dev_tabs[p][:, DISCRETE]), bits(host_tab[:, DISCRETE])), "%s: ids / hits / misses / born ticks" % w
            close(dev_tabs[p][:dev_cnt[p], :6], host_tab[:dev_cnt[p], :6], "%s: table" % w)
            assert np.array_equal(bits(dev_stats[p]), bits(m.rec)), "%s: statistics: device %s, mirror %s" % (w, dev_stats[p], m.rec)
            # the planner's digest: error word, number of trajectories and of ids
            dg = sl.digest_row(dict(r, failed=False))
            assert np.array_equal(tr[p, 8:][[0, 3, 4]], dg[[0, 3, 4]]), "%s: digest %s vs %s" % (w, tr[p, 8:16], dg[:8])
            prev_traj[p] = fleet.trajectories(p)[0]
            a = np.asarray(r["assign"], int)
            stats['match_low'] += int(np.sum(a[:64] >= 0))
            stats['match_high'] += int(np.sum(a[64:] >= 0))
            stats['max_det'], stats['max_out'] = max(stats['max_det'], len(a)), max(stats['max_out'], r["cnt"])
            stats['coast_out'] += r["cnt"] - r["out_live"]
    final = (fleet.sim_state(), fleet.sim_heading(), fleet.digest(), fleet.sim_tracker_read(planners=list(range(sc.n)), raw=True))
    fleet.close()
    # the same scenario in one call: bitwise the single ticks, digest, tables and records included
    fleet = tracker_fleet(sc, hip, skw, tkw, kind)
    one = fleet.sim_run(n_ticks)[0]
    assert np.array_equal(one, np.array(traces), equal_nan=True), "%s: one call differs from the single ticks" % what
    st = fleet.sim_state()
    assert all(np.array_equal(st[key], final[0][key]) for key in st) and np.array_equal(fleet.sim_heading(), final[1])
    assert np.array_equal(fleet.digest(), final[2])
    again = fleet.sim_tracker_read(planners=list(range(sc.n)), raw=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again[:2], final[3][:2])) and np.array_equal(again[2], final[3][2])
    fleet.close()
    stats['rec'] = np.sum(final[3][0], axis=0)
    print("\n%s: %d ticks x %d planners against the tracking host loop; up to %d detections, up to %d handed on (%d coasting in all); matched "
          "below / from slot 64: %d / %d; largest deviation %.3g; counters %s" % (
              what, n_ticks, sc.n, stats['max_det'], stats['max_out'], stats['coast_out'], stats['match_low'], stats['match_high'], stats['worst'],
              stats['rec'].astype(int).tolist()))
    return stats


@pytest.mark.parametrize("index", range(5))
def test_lockstep_against_the_tracking_host_loop(hip, monteblanco, oracle_backend, table, track, c2_start, index):
    name, units, skw, tkw, ticks, kind = tu.scenarios(table, track, c2_start)[index]
    sc = gd.Scenario(monteblanco, table, units)
    assert sc.n <= 8 and ticks <= 60
    stats = lockstep(sc, hip, oracle_backend, ticks, skw, tkw, kind, name)
    rec = stats['rec']
    assert rec[2] > 0 and rec[3] > 0 and rec[8] > 0 and stats['coast_out'] == rec[8], stats     # matches, births, coasting objects handed on
    if name == "crowd":
        assert stats['max_det'] > 64 and stats['match_low'] > 0 and stats['match_high'] > 0, stats
    if kind == "noise":
        print("noisy run: largest deviation from the host loop %.3g (the sensor tests hold %.3g); bound %.3g" % (stats['worst'], SENSOR_TOL, NOISE_TOL))
        assert stats['worst'] <= NOISE_TOL
    else:
        assert stats['worst'] == 0.0


# ---- 3. telemetry against truth -----------------------------------------------------------------------------------------------------------
def test_telemetry_measures_truth_behind_a_tracker_that_hands_on_nothing(hip, monteblanco, table, c2_start):
    sc = gd.Scenario(monteblanco, table, [gn.tele_unit(table, c2_start)])
    blind = sc.fleet(hip)
    blind.sim_telemetry(radius=gn.TELE_RADIUS)
    blind.sim_sensor(range=1.0)                              # the only object stands 14 m ahead: never shown
    ref = blind.sim_run(30)[0]
    ref_tele = blind.sim_telemetry_read()
    blind.close()
    fleet = sc.fleet(hip)
    fleet.sim_telemetry(radius=gn.TELE_RADIUS)
    fleet.sim_tracker(n_confirm=255)                         # seen in every tick, never confirmed within the run
    trace = fleet.sim_run(30)[0]
    tele, d = fleet.sim_telemetry_read(), fleet.sim_tracker_read()
    assert all(np.array_equal(np.asarray(tele[key]), np.asarray(ref_tele[key]), equal_nan=True) for key in ref_tele), "telemetry records"
    assert np.array_equal(trace, ref, equal_nan=True)
    fleet.close()
    assert np.all(trace[:, 0, 5] == 0) and np.all(np.isnan(trace[:, 0, 6:8]))
    assert d["n_det"][0] == 30 and d["n_matched"][0] == 29 and d["n_born"][0] == 1 and d["n_out"][0] == 0 and d["n_confirmed"][0] == 0
    assert np.isfinite(tele["clear_min"][0]) and tele["contact_ticks"][0] > 0


# ---- 4. tick0 -----------------------------------------------------------------------------------------------------------------------------
def test_tick0_is_the_born_tick_of_the_first_tracks(hip, monteblanco, table, track, c2_start):
    sc = gd.Scenario(monteblanco, table, gn.singles(table, track, c2_start)[:2])
    kw = dict(gate=6.0, w_pos=0.5, w_vel=0.5, n_confirm=2, n_coast=3)
    fleet = tracker_fleet(sc, hip, None, kw, tick0=1000)
    a = fleet.sim_run(5)[0]
    _, tabs, cnt = fleet.sim_tracker_read(planners=[0, 1])
    assert np.all(cnt > 0) and all(np.all(tabs[p, :cnt[p], 9] == 1000.0) for p in range(2)) and np.all(np.isnan(tabs[0, cnt[0]:]))
    fleet.close()
    plain = tracker_fleet(sc, hip, None, kw)
    assert np.array_equal(plain.sim_run(5)[0], a, equal_nan=True)          # the tick labels the tracks, it decides nothing
    _, tabs0, cnt0 = plain.sim_tracker_read(planners=[0, 1])
    assert np.array_equal(cnt0, cnt) and np.array_equal(bits(tabs0[:, :, :9]), bits(tabs[:, :, :9])) and np.all(tabs0[0, :cnt0[0], 9] == 0.0)
    plain.close()


# ---- 5. a planner that is not live --------------------------------------------------------------------------------------------------------
def test_a_planner_that_is_not_live_keeps_its_table(hip, monteblanco, table, track, c2_start):
    classes = sl.monteblanco_classes(table, track, tuple(c2_start['pos']))
    # (the velocity arguments carry no emergency trajectory: a preference list of 'emergency' alone never finds its action)
    dead = dict(classes["failing"], entry=dict(classes["failing"]["entry"], pref=("emergency",)))
    sc = gd.Scenario(monteblanco, table, [gd.single("one", classes["one"], c2_start), gd.single("failing", dead, c2_start)])
    fleet = tracker_fleet(sc, hip, None, dict(gate=6.0, n_confirm=1, n_coast=2))
    tr = gd.run_one(fleet, 10)
    assert np.all(tr[:, 0, 8] == 0) and np.all(tr[:, 1, 8] != 0)             # planner 1 finds no action in its first tick
    rec, tabs, cnt = fleet.sim_tracker_read(planners=[0, 1], raw=True)
    assert rec[0, 0] == 10 and cnt[0] == 1 and np.all(rec[1] == 0) and cnt[1] == 0
    # planner 1 takes planner 0's state, its table with it; its own preference list finds no action again: the table stays as it is
    fleet.sim_branch([0], [1])
    _, tabs_b, cnt_b = fleet.sim_tracker_read(planners=[0, 1], raw=True)
    assert cnt_b[1] == 1 and np.array_equal(bits(tabs_b[1]), bits(tabs[0])) and np.array_equal(bits(tabs_b[0]), bits(tabs[0]))
    tr = gd.run_one(fleet, 5)
    assert np.all(tr[:, 0, 8] == 0) and np.all(tr[:, 1, 8] != 0)
    rec2, tabs2, cnt2 = fleet.sim_tracker_read(planners=[0, 1], raw=True)
    assert cnt2[1] == 1 and np.array_equal(bits(tabs2[1]), bits(tabs_b[1])) and np.all(rec2[1] == 0)
    assert rec2[0, 0] == 15 and tabs2[0, 0, 7] == 15.0 and not np.array_equal(bits(tabs2[0]), bits(tabs_b[0]))
    fleet.close()


# ---- 6. snapshot, restore, branch ---------------------------------------------------------------------------------------------------------
def test_snapshot_restore_and_branch_carry_table_and_next_id(hip, monteblanco, table, track, c2_start):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    s = gn.singles(table, track, c2_start)
    bare = dict(s[0]["entries"][0], static=[])               # the opponents of s[0] without its static object: 2 slots, capacity 4 ...
    small = gd.single("small", dict(entry=bare, vel=sl.C2_VEL), c2_start)
    many = dict(s[0]["entries"][0], static=sl.crowded_statics(track, 12, 5, first_row=150, every=4, off_every=100, off_phase=99))
    big = gd.single("big", dict(entry=many, vel=sl.C2_VEL), c2_start)      # ... and with 12 statics on the track: 14 slots, capacity 28
    sc = gd.Scenario(monteblanco, table, [s[0], s[0], small, big])
    skw = dict(range=float("inf"), p_drop=0.3, seed=[11, 12, 13, 14])
    tkw = dict(gate=6.0, w_pos=0.5, w_vel=0.5, n_confirm=[2, 1, 1, 1], n_coast=[3, 0, 3, 3])
    fleet = tracker_fleet(sc, hip, skw, tkw)
    every = list(range(sc.n))
    fleet.sim_run(10)
    fleet.sim_snapshot(0)
    rec10, tabs10, cnt10 = fleet.sim_tracker_read(planners=every, raw=True)
    ref = fleet.sim_run(10)[0]
    rec20, tabs20, cnt20 = fleet.sim_tracker_read(planners=every, raw=True)
    assert np.all(cnt10[:2] > 0) and cnt20[3] > 4
    # restore: the tables and next_id come back, the statistics are not rolled back; under the same sensor ticks the run repeats bitwise
    fleet.sim_restore(0)
    rec_r, tabs_r, cnt_r = fleet.sim_tracker_read(planners=every, raw=True)
    assert np.array_equal(cnt_r, cnt10) and np.array_equal(bits(tabs_r), bits(tabs10)) and np.array_equal(bits(rec_r), bits(rec20))
    fleet.sim_sensor(tick0=10, **skw)
    again = fleet.sim_run(10)[0]
    assert np.array_equal(again, ref, equal_nan=True)
    rec30, tabs30, cnt30 = fleet.sim_tracker_read(planners=every, raw=True)
    # (the tracker tick went on: tracks born in the repeated half carry later born ticks; everything else, the ids included, repeats)
    assert np.array_equal(cnt30, cnt20) and np.array_equal(bits(tabs30[:, :, :9]), bits(tabs20[:, :, :9]))
    assert np.array_equal(bits((rec30 - rec20)[:, :11]), bits((rec20 - rec10)[:, :11]))
    # branch live -> live: planner 1 takes planner 0's table and next_id; configuration and statistics stay its own
    fleet.sim_branch([0], [1])
    rec_b, tabs_b, cnt_b = fleet.sim_tracker_read(planners=every, raw=True)
    assert cnt_b[1] == cnt30[0] and np.array_equal(bits(tabs_b[1]), bits(tabs30[0])) and np.array_equal(bits(rec_b), bits(rec30))
    ids_before = set(tabs_b[1, :cnt_b[1], 6].astype(int).tolist())
    top = max(int(np.nanmax(tabs30[0, :, 6])), -1)
    fleet.sim_run(12)
    _, tabs_c, cnt_c = fleet.sim_tracker_read(planners=every, raw=True)
    new1 = [i for i in tabs_c[1, :cnt_c[1], 6].astype(int).tolist() if i not in ids_before]
    assert all(i > top for i in new1), (new1, top)           # planner 1 goes on counting from planner 0's next_id: no id is reused
    # a source without tracker state empties the destination's table: a snapshot taken with the tracker off
    fleet.sim_tracker(None)
    fleet.sim_snapshot(1)
    fleet.sim_tracker(**tkw)
    fleet.sim_run(5)
    _, tabs_d, cnt_d = fleet.sim_tracker_read(planners=every, raw=True)
    assert np.all(cnt_d[[0, 3]] > 0)
    fleet.sim_restore(1)
    _, tabs_e, cnt_e = fleet.sim_tracker_read(planners=every, raw=True)
    assert np.all(cnt_e == 0) and np.all(np.isnan(tabs_e))
    fleet.sim_run(3)
    _, tabs_f, cnt_f = fleet.sim_tracker_read(planners=every, raw=True)
    assert cnt_f[3] > 4 and np.nanmin(tabs_f[3, :, 6]) == 0.0               # ids start at 0 again: the tracker's start state
    # more tracks than the destination's table holds: planner 3 (capacity 28) onto planner 2 (capacity 4), live and from a snapshot
    fleet.sim_snapshot(2)
    for call in (lambda: fleet.sim_branch([3], [2]), lambda: fleet.sim_branch([3], [2], snapshot=2)):
        with pytest.raises(BackendError, match="tracks, the destination's table 4"):
            call()
    _, tabs_g, cnt_g = fleet.sim_tracker_read(planners=every, raw=True)
    assert np.array_equal(cnt_g, cnt_f) and np.array_equal(bits(tabs_g), bits(tabs_f))      # a refused branch copies nothing
    fleet.sim_branch([2], [3])                               # the other way round fits
    assert fleet.sim_tracker_read(planners=[3], raw=True)[2][0] == cnt_f[2]
    fleet.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_keep_the_previous_tracker_and_its_tables(hip, monteblanco, table, track, c2_start):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    bare = Fleet(hip, 2)
    for call in (lambda: bare.sim_tracker(), lambda: bare.sim_tracker(None), lambda: bare.sim_tracker_read()):
        with pytest.raises(BackendError, match="sim_setup first"):
            call()
    one = dict(params=[[5.0, 0.0, 0.0, 1.0, 0.0]], adv=0.25, tick=0, next_id=0.0)
    for kw, msg in ((dict(cap=96, slots=96, tracks=[np.zeros((0, 10))], dets=[np.zeros((97, 6))]), "slots detections"),
                    (dict(cap=4, slots=2, tracks=[np.zeros((5, 10))], dets=[np.zeros((1, 6))]), "capacity tracks"),
                    (dict(cap=97, slots=2, tracks=[np.zeros((0, 10))], dets=[np.zeros((1, 6))]), "0 .. 96"),
                    (dict(cap=4, slots=2, tracks=[np.zeros((0, 10))], dets=[np.zeros((1, 6))], params=[[0.0, 0.0, 0.0, 1.0, 0.0]]), "parameters")):
        with pytest.raises(BackendError, match=msg):
            bare.sim_tracker_eval(**dict(one, **kw))
    bare.close()
    sc = gd.Scenario(monteblanco, table, gn.singles(table, track, c2_start)[:2])
    fleet = tracker_fleet(sc, hip, None, dict(gate=6.0, n_confirm=[1, 255], n_coast=2))
    ticks = 0

    def still_in_force():
        nonlocal ticks
        tr = fleet.sim_run(1)[0][0]
        ticks += 1
        rec, tabs, cnt = fleet.sim_tracker_read(planners=[0, 1])
        assert np.all(rec["ticks"] == ticks) and tr[0, 5] > 0 and tr[1, 5] == 0 and rec["n_out"][1] == 0       # planner 1 never confirms
        assert np.all(cnt > 0) and np.all(tabs[0, :cnt[0], 7] <= ticks) and np.max(tabs[0, :cnt[0], 7]) == ticks      # the tables were kept
    still_in_force()
    nan, inf = float("nan"), float("inf")
    bad = [(dict(gate=nan), "gate"), (dict(gate=0.0), "gate"), (dict(gate=-1.0), "gate"), (dict(gate=[6.0, inf]), "gate"),
           (dict(w_pos=1.0), "w_pos"), (dict(w_pos=-0.1), "w_pos"), (dict(w_pos=nan), "w_pos"),
           (dict(w_vel=1.0), "w_vel"), (dict(w_vel=[0.0, -1.0]), "w_vel"), (dict(w_vel=nan), "w_vel"),
           (dict(n_confirm=0), "n_confirm"), (dict(n_confirm=256), "n_confirm"), (dict(n_coast=-1), "n_coast"), (dict(n_coast=[0, 256]), "n_coast"),
           (dict(tick0=-1), "tick0")]
    for args, msg in bad:
        with pytest.raises(BackendError, match=msg):
            fleet.sim_tracker(**args)
        still_in_force()
    with pytest.raises(BackendError, match="out of range"):
        fleet.sim_tracker_read(planners=[2])
    fleet.close()


# ---- 8. identity --------------------------------------------------------------------------------------------------------------------------
def test_cleared_tracker_and_fresh_setup_leave_the_trace_untouched(hip, monteblanco, table, track, c2_start):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    sc = gd.Scenario(monteblanco, table, gn.mixed(table, track, c2_start))
    plain = sc.fleet(hip)
    ref = plain.sim_run(30)[0]
    ref_state, ref_digest = plain.sim_state(), plain.digest()
    plain.close()
    kw = tu.tracker_args(sc.n)
    cleared = tracker_fleet(sc, hip, None, kw)
    cleared.sim_tracker(gate=None)
    tr = cleared.sim_run(30)[0]
    st = cleared.sim_state()
    assert np.array_equal(tr, ref, equal_nan=True)
    assert all(np.array_equal(st[k], ref_state[k]) for k in st) and np.array_equal(cleared.digest(), ref_digest)
    with pytest.raises(BackendError, match="the tracker is off"):
        cleared.sim_tracker_read()
    # sim_setup switches the tracker off; sim_race keeps it
    cleared.sim_tracker(**kw)
    cleared.sim_setup(sc.tab, sc.entries, dt=sc.dt, n_export=sc.n_export)
    with pytest.raises(BackendError, match="the tracker is off"):
        cleared.sim_tracker_read()
    cleared.sim_tracker(**kw)
    cleared.sim_race(sc.sizes, length=5.0)
    assert np.all(cleared.sim_tracker_read()["ticks"] == 0)
    cleared.close()
    # the pass-through tracker (w = 0, confirmed at once, no coasting) hands on the detections: the same counts
    through = tracker_fleet(sc, hip, None, dict(gate=6.0, w_pos=0.0, w_vel=0.0, n_confirm=1, n_coast=0))
    tr = through.sim_run(30)[0]
    assert np.array_equal(tr[:, :, 5], ref[:, :, 5])
    through.close()
    # and the tracker is not a no-op on this scenario
    tracked = tracker_fleet(sc, hip, None, kw)
    assert not np.array_equal(tracked.sim_run(30)[0], ref, equal_nan=True)
    tracked.close()
