"""
GPU: the campaign statistics of the fleet's closed-loop simulation (ltpl_fleet_sim_stats / _stats_reduce / _stats_series / _stats_eval;
csrc/fleet_stats.hpp, k_fleet_sim_stats_chunk / k_fleet_sim_stats_merge / k_fleet_sim_stats_eval in csrc/fleet_sim.hpp) against the host
mirror (sim.stats_reduce / sim.StatsModel), bit for bit throughout --

  1. the hook on the case list of sim_stats_util.cases (0, 1, 63, 64, 65, 1023, 1024, 1025 and 2049 members among them, the sum-order
     cases too), in batches of 1, 63, 64 and 65 cases;
  2. 8 planners x 40 ticks with telemetry, safety monitor, vehicle model and reactive opponents: two groups of three (one of them a
     race), one planner in no group, one on the ideal tracker (its vehicle record is NaN), one that fails at tick 20 (STATE / failed);
     after every tick ltpl_fleet_sim_stats_reduce against sim.StatsModel fed from the _read calls, rows and lists;
  3. the series: one sim_run(40) with period 4 and depth 6 holds rows 5 .. 10 of the 10 written, ticks and rows equal to reductions
     taken by hand in a twin run cut into pieces;
  4. 1 025 planners in one group, the smallest fleet with two chunks, 20 ticks with telemetry only;
  5. measurement only: trace, state, digest, telemetry and safety records with a plan, without one and with a cleared one;
  6. the plan's lifetime: keep_series, snapshot / restore / branch, a module switched off under the plan, sim_setup, the refusals.
"""
import ctypes
import os

import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import sim_stats_util as xu
import test_gpu_sim_differential as gd
import test_gpu_sim_noise as gn
import test_gpu_sim_safety as gsf
from graphbasedlocaltrajectoryplanner_amd import sim
from graphbasedlocaltrajectoryplanner_amd.sim import Event

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = xu.bits
F = xu.F
GROUPS8 = [1, 0, 0, 0, 1, 1, -1, 2]       # planners 1 .. 3 are the race; planner 6 is in no group
MODEL8 = [1, 1, 1, 1, 0, 1, 1, 1]         # planner 4 drives on the ideal tracker: its vehicle record is NaN
FAILS = 5                                 # the planner whose preference list becomes unusable at tick 20
MEASURES = [("telemetry", "clear_min", 0.0, 40.0, 8, -1), ("telemetry", "dist", 0.0, 30.0, 16, 1), ("telemetry", "act[1]", 0.0, 40.0, 4, 1),
            ("safety", "gap_min", -2.0, 30.0, 16, -1), ("safety", "ttc_min", 0.0, 20.0, 5, -1), ("safety", "hist[7]", 0.0, 40.0, 1, 0),
            ("vehicle", "e_max", 0.0, 0.5, 10, 1), ("vehicle", "v", 0.0, 30.0, 3, -1), ("react", "gap_min", 0.0, 100.0, 7, -1),
            ("react", "follow_ticks", 0.0, 80.0, 2, 1), ("state", "failed", 0.0, 2.0, 2, 1)]


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


def tele_rows(fleet):
    out, length = np.zeros((fleet.n_scen, sim.TELEMETRY_DOUBLES)), ctypes.c_double(0.0)
    fleet._check(fleet._fn("sim_telemetry_read")(fleet.handle, out.ctypes.data, sim.TELEMETRY_DOUBLES, ctypes.byref(length)))
    return out


def records_of(fleet, families):
    read = dict(telemetry=lambda: tele_rows(fleet), safety=lambda: fleet.sim_safety_read(raw=True)[0], vehicle=lambda: fleet.sim_vehicle_read(raw=True),
                react=lambda: fleet.sim_react_read(raw=True)[0])
    return {f: read[f]() for f in families}


def same(dev, want, what):
    for name, a, b in (("rows", dev[0], want[0]), ("tops", dev[1], want[1])):
        assert a.shape == b.shape, "%s: %s of shape %s, the mirror's %s" % (what, name, a.shape, b.shape)
        ne = bits(a) != bits(b)
        assert not ne.any(), "%s: %s differ at %s: %s against the mirror's %s" % (what, name, np.argwhere(ne)[:6].tolist(), a[ne][:6], b[ne][:6])


def fleet8(hip, monteblanco, table, track, c2_start):
    """The eight planners of the safety monitor's test with every recording module on and planner FAILS failing at tick 20."""
    sc = gd.Scenario(monteblanco, table, gsf.units8(table, track, c2_start))
    assert sc.n == 8 and sc.sizes == [1, 3, 1, 1, 1, 1]
    fleet = sc.fleet(hip)
    fleet.sim_telemetry(radius=2.5)
    fleet.sim_safety(**gsf.PAR)
    fleet.sim_vehicle(model=MODEL8)
    fleet.sim_react()
    # every entry of the planner's list becomes `emergency`, which is never exported here: the step kernel finds no action
    fleet.sim_events([Event(FAILS, when=("tick", 20), set=("pref", e, "emergency")) for e in range(len(sc.entries[FAILS]["pref"]))])
    return sc, fleet


# ---- 1. the hook --------------------------------------------------------------------------------------------------------------------------
def test_the_hook_equals_the_mirror_bit_for_bit(hip):
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    cs = xu.cases()[0]
    ref = [xu.mirror(c) for c in cs]
    assert set(xu.COUNTS) <= {c["values"].size for c in cs} and max(c["values"].size for c in cs) <= 3000
    fleet = Fleet(hip, 1)
    at = 0
    for m in (1, 63, 64, 65):
        idx = [(at + k) % len(cs) for k in range(m)]
        at += m
        # (a batch is one planner_idx array or none: the cases without planners get their positions, which is what None means)
        planners = [np.arange(cs[i]["values"].size) if cs[i]["planners"] is None else cs[i]["planners"] for i in idx]
        rows, tops = fleet.sim_stats_eval([cs[i]["values"] for i in idx], [xu.spec_of(cs[i]) for i in idx], planners)
        for j, i in enumerate(idx):
            xu.compare(dict(row=rows[j], top=tops[j]), ref[i], "batch of %d, case %d" % (m, i))
    assert at >= len(cs)                    # every case ran at least once
    plain = [i for i, c in enumerate(cs) if c["planners"] is None][:70]              # planner_idx == NULL: the positions
    rows, tops = fleet.sim_stats_eval([cs[i]["values"] for i in plain], [xu.spec_of(cs[i]) for i in plain])
    for j, i in enumerate(plain):
        xu.compare(dict(row=rows[j], top=tops[j]), ref[i], "without planner_idx, case %d" % i)
    assert len(fleet.sim_stats_eval([], np.zeros((0, 5)))[0]) == 0
    fleet.close()


# ---- 2. the tick --------------------------------------------------------------------------------------------------------------------------
def test_forty_ticks_of_eight_planners_against_the_mirror(hip, monteblanco, table, track, c2_start):
    sc, fleet = fleet8(hip, monteblanco, table, track, c2_start)
    fleet.sim_stats(GROUPS8, MEASURES, top_k=3)
    model = sim.StatsModel(GROUPS8, MEASURES, top_k=3)
    families = ("telemetry", "safety", "vehicle", "react")
    failed = np.zeros(8, bool)
    seen_nan = seen_inf = 0
    for k in range(40):
        tr = gd.run_one(fleet, 1)[0]
        failed = failed | (tr[:, 8] != 0)   # the error word stays
        rec = records_of(fleet, families)
        dev = fleet.sim_stats_reduce()
        same(dev, model.reduce(rec, failed), "tick %d" % k)
        seen_nan += int(dev[0][..., F["n_nan"]].sum())
        seen_inf += int(dev[0][..., F["n_inf"]].sum())
        assert (k < 20 and not failed.any()) or (k >= 20 and failed.tolist() == [p == FAILS for p in range(8)]), (k, failed)
    rows, tops = dev
    d = sim.stats_dict(rows)
    print("statistics after 40 ticks: n %s, min %s, argmin %s" % (d["n"].tolist(), d["min"].tolist(), d["argmin"].tolist()))
    m_fail, m_veh = len(MEASURES) - 1, 6
    assert rows[1, m_fail, F["sum"]] == 1 and rows[1, m_fail, F["argmax"]] == FAILS and rows[0, m_fail, F["sum"]] == 0 and tops[1, m_fail, 0].tolist() == [1.0, FAILS]
    assert rows[1, m_veh, F["n_nan"]] == 1 and rows[1, m_veh, F["n"]] == 2 and rows[0, m_veh, F["n"]] == 3 and rows[2, m_veh, F["n"]] == 1
    assert seen_nan >= 40 and seen_inf > 0 and np.all(np.isin(rows[0, :, F["argmin"]], [1, 2, 3])) and 6 not in rows[..., F["argmin"]]
    assert np.all(rows[..., F["hist"]:].sum(axis=-1) + rows[..., F["under"]] + rows[..., F["over"]] + rows[..., F["n_nan"]] ==
                  np.array([3, 3, 1])[:, None])
    fleet.close()


# ---- 3. the series ------------------------------------------------------------------------------------------------------------------------
def test_the_series_holds_the_last_rows_of_a_run(hip, monteblanco, table, track, c2_start):
    _, whole = fleet8(hip, monteblanco, table, track, c2_start)
    whole.sim_stats(GROUPS8, MEASURES, top_k=2, period=4, depth=6)
    gd.run_one(whole, 40)
    ticks, ring, total = whole.sim_stats_series()
    final = whole.sim_stats_reduce()[0]
    whole.close()
    assert total == 10 and ticks.tolist() == [19, 23, 27, 31, 35, 39] and ring.shape == (6, 3, len(MEASURES), 27)
    _, twin = fleet8(hip, monteblanco, table, track, c2_start)
    twin.sim_stats(GROUPS8, MEASURES, top_k=2)                   # on demand only
    by_hand = []
    for k in range(10):
        gd.run_one(twin, 4)
        by_hand.append(twin.sim_stats_reduce()[0])
    twin.close()
    for j in range(6):
        assert np.array_equal(bits(ring[j]), bits(by_hand[4 + j])), "row %d of the ring (tick %d)" % (j, ticks[j])
    assert np.array_equal(bits(final), bits(by_hand[-1])) and not np.array_equal(bits(ring[0]), bits(ring[5]))


# ---- 4. two chunks on a real fleet --------------------------------------------------------------------------------------------------------
def test_a_plan_spanning_two_chunks(hip, monteblanco, table, c2_start):
    classes = sl.monteblanco_classes(table, np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")), tuple(c2_start['pos']))
    n = sim.STATS_CHUNK + 1
    sc = gd.Scenario(monteblanco, table, gd.dealt_units(classes, c2_start, n, seed=n))
    fleet = sc.fleet(hip)
    fleet.sim_telemetry(radius=2.5)
    measures = [("telemetry", "clear_min", 0.0, 40.0, 16, -1), ("telemetry", "dist", 0.0, 20.0, 8, 1), ("telemetry", "vel_sum", 0.0, 300.0, 12, 1),
                ("telemetry", "rank", 0.0, 5.0, 5, 0), ("state", "failed", 0.0, 2.0, 2, 1)]
    groups = [np.zeros(n, int), np.arange(n) % 3 - 1]            # everyone in one group of two chunks; three thirds, one of them in no group
    tr = gd.run_one(fleet, 20)
    failed = (tr[:, :, 8] != 0).any(axis=0)
    rec = dict(telemetry=tele_rows(fleet))
    for g in groups:
        fleet.sim_stats(g, measures, top_k=8)
        dev = fleet.sim_stats_reduce()
        same(dev, sim.StatsModel(g, measures, top_k=8).reduce(rec, failed), "%d groups" % (g.max() + 1))
    fleet.sim_stats(groups[0], measures, top_k=8)
    rows = fleet.sim_stats_reduce()[0]
    fleet.close()
    r = rows[0, 1]
    assert r[F["n"]] + r[F["n_nan"]] + r[F["n_inf"]] == n and rows[0, 4, F["sum"]] == failed.sum() > 0
    # the sum of the 1 025 distances is the specified order's (the hook's order cases tell it from the other orders)
    v = rec["telemetry"][:, 2]
    print("sum of dist: %r; left to right %r, numpy %r" % (r[F["sum"]], xu.sum_plain(v), xu.sum_numpy(v)))
    assert bits(r[F["sum"]]) == bits(sim.stats_sum(v))


# ---- 5. no side effects -------------------------------------------------------------------------------------------------------------------
def test_the_plan_changes_nothing_else(hip, monteblanco, table, track, c2_start):
    sc = gd.Scenario(monteblanco, table, gn.mixed(table, track, c2_start))
    measures = [("telemetry", "clear_min", 0.0, 40.0, 8, -1), ("safety", "gap_min", -2.0, 30.0, 16, -1), ("state", "failed", 0.0, 2.0, 2, 1)]

    def run(mode):
        fleet = sc.fleet(hip)
        fleet.sim_telemetry(radius=2.5)
        fleet.sim_safety(**gsf.PAR)
        if mode != "never":
            fleet.sim_stats(np.arange(sc.n) % 2, measures, top_k=4, period=3, depth=4)
        if mode == "cleared":
            fleet.sim_stats(None)
        tr = gd.run_one(fleet, 30)
        if mode == "on":
            assert fleet.sim_stats_series()[2] == 10 and fleet.sim_stats_reduce()[0][..., F["n"]].sum() > 0
        out = (tr, fleet.sim_state(), fleet.digest(), tele_rows(fleet), fleet.sim_safety_read(raw=True))
        fleet.close()
        return out
    ref = run("never")
    for mode in ("on", "cleared"):
        got = run(mode)
        assert np.array_equal(bits(got[0]), bits(ref[0])), mode
        assert all(np.array_equal(got[1][k], ref[1][k]) for k in ref[1]) and np.array_equal(bits(got[2]), bits(ref[2])), mode
        assert np.array_equal(bits(got[3]), bits(ref[3])), mode
        assert np.array_equal(bits(got[4][0]), bits(ref[4][0])) and np.array_equal(bits(got[4][1]), bits(ref[4][1])), mode


# ---- 6. the plan's lifetime ---------------------------------------------------------------------------------------------------------------
def test_plan_lifetime_and_refusals(hip, monteblanco, table, track, c2_start):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    sc = gd.Scenario(monteblanco, table, gn.singles(table, track, c2_start))
    assert sc.n == 3
    fleet = sc.fleet(hip)
    with pytest.raises(BackendError, match="no plan"):
        fleet.sim_stats_reduce()
    measures = [("telemetry", "dist", 0.0, 30.0, 6, 1), ("state", "failed", 0.0, 2.0, 2, 1)]
    with pytest.raises(BackendError, match="measure 0: family telemetry is off"):
        fleet.sim_stats([0, 0, 1], measures)
    fleet.sim_telemetry(radius=2.5)
    for bad, text in ((dict(groups=[0, 0, 5], n_groups=2), "planner 2: group"), (dict(groups=[-2, 0, 1]), "planner 0: group"), (dict(top_k=9), "top_k"), (dict(period=2), "depth"), (dict(tick0=-1), "tick0"),
                      (dict(measures=[("telemetry", 22, 0.0, 1.0, 4, 0)]), "column outside the 22 doubles"),
                      (dict(measures=[("telemetry", "dist", 1.0, 1.0, 4, 0)]), "lo must be below hi"),
                      (dict(measures=[("telemetry", "dist", 0.0, 1.0, 17, 0)]), "bins"), (dict(measures=[("telemetry", "dist", 0.0, 1.0, 4, 2)]), "top_dir"),
                      (dict(period=1, depth=2 ** 31 - 1), "256 MiB")):
        with pytest.raises(BackendError, match=text):
            fleet.sim_stats(**dict(dict(groups=[0, 0, 1], measures=measures), **bad))
    fleet.sim_stats([0, 0, 1], measures, top_k=2, period=2, depth=3, tick0=1)
    with pytest.raises(BackendError, match="planner 1: group"):                      # a refused call keeps the plan
        fleet.sim_stats([0, 7, 1], measures, n_groups=2)
    model = sim.StatsModel([0, 0, 1], measures, top_k=2, period=2, depth=3, tick0=1)

    def ticks(n):
        for _ in range(n):
            gd.run_one(fleet, 1)
            model.tick(dict(telemetry=tele_rows(fleet)), np.zeros(3))
    ticks(5)                                # indices 1 .. 5: rows at the ticks 1, 3, 5
    t, rows, total = fleet.sim_stats_series()
    assert t.tolist() == [1, 3, 5] and total == 3 and np.array_equal(bits(rows), bits(model.series()[1]))
    # snapshot, restore and branch leave plan and series alone
    fleet.sim_snapshot(0)
    ticks(2)
    fleet.sim_restore(0)
    fleet.sim_branch(0, [1])
    t, rows, total = fleet.sim_stats_series()
    assert t.tolist() == [3, 5, 7] and total == 4 and np.array_equal(bits(rows), bits(model.series()[1]))
    same(fleet.sim_stats_reduce(), model.reduce(dict(telemetry=tele_rows(fleet)), np.zeros(3)), "behind restore and branch")
    # keep_series: other ranges, period and tick0 on the same ring; another shape is refused and keeps everything
    measures2 = [("telemetry", "dist", 0.0, 60.0, 3, -1), ("state", "failed", 0.0, 2.0, 2, 1)]
    for bad in (dict(depth=4), dict(groups=[0, 1, 2]), dict(period=0, depth=0)):
        with pytest.raises(BackendError, match="KEEP_SERIES"):
            fleet.sim_stats(**dict(dict(groups=[0, 0, 1], measures=measures2, period=1, depth=3, keep_series=True), **bad))
    fleet.sim_stats([1, 0, 0], measures2, top_k=1, period=1, depth=3, tick0=100, keep_series=True)
    assert fleet.sim_stats_series()[2] == 4
    gd.run_one(fleet, 1)
    t, rows, total = fleet.sim_stats_series()
    assert t.tolist() == [5, 7, 100] and total == 5 and np.array_equal(bits(rows[:2]), bits(model.series()[1][1:]))
    now = sim.StatsModel([1, 0, 0], measures2, top_k=1).reduce(dict(telemetry=tele_rows(fleet)), np.zeros(3))
    assert np.array_equal(bits(rows[2]), bits(now[0]))
    same(fleet.sim_stats_reduce(), now, "the new plan")
    fleet.sim_stats([1, 0, 0], measures2, period=1, depth=3)    # without the flag the series starts anew
    assert fleet.sim_stats_series()[2] == 0
    # telemetry set again re-allocates its records: the plan follows
    fleet.sim_telemetry(radius=1.0)
    gd.run_one(fleet, 2)
    assert np.array_equal(bits(fleet.sim_stats_reduce()[0]), bits(sim.StatsModel([1, 0, 0], measures2).reduce(dict(telemetry=tele_rows(fleet)), np.zeros(3))[0]))
    # a module switched off under the plan: reduce and a periodic run refuse, the fleet runs on once the plan is cleared
    fleet.sim_telemetry(None)
    with pytest.raises(BackendError, match="family telemetry is off"):
        fleet.sim_stats_reduce()
    before = fleet.sim_state()
    with pytest.raises(BackendError, match="family telemetry is off"):
        fleet.sim_run(1)
    after = fleet.sim_state()
    assert all(np.array_equal(before[k], after[k]) for k in before)                  # refused before its first tick
    fleet.sim_stats(None)
    with pytest.raises(BackendError, match="no series"):
        fleet.sim_stats_series()
    fleet.sim_run(1)
    # sim_setup clears the plan
    fleet.sim_telemetry(radius=2.5)
    fleet.sim_stats([0, 0, 0], measures)
    fleet.sim_stats_reduce()
    fleet.sim_setup(table, sc.entries)
    with pytest.raises(BackendError, match="no plan"):
        fleet.sim_stats_reduce()
    for kw, text in ((dict(spec=[[0.0, 1.0, 0.0, 0.0, 0.0]]), "bins"), (dict(spec=[[1.0, 0.0, 4.0, 0.0, 0.0]]), "lo must be below hi"),
                     (dict(spec=[[0.0, 1.0, 4.0, 0.0, 9.0]]), "top_k"), (dict(planners=[[0, -1, 2]]), "planner index")):
        a = dict(dict(values=[[1.0, 2.0, 3.0]], spec=[[0.0, 1.0, 4.0, 0.0, 0.0]], planners=None), **kw)
        with pytest.raises(BackendError, match=text):
            fleet.sim_stats_eval(a["values"], a["spec"], a["planners"])
    fleet.close()
