"""
GPU: the behaviour selector of the fleet's closed-loop simulation (ltpl_fleet_sim_selector / _selector_read / _selector_eval;
csrc/fleet_select.hpp, k_fleet_sim_select / k_fleet_sim_selector_eval in csrc/fleet_sim.hpp) against its host mirror (sim.SelectorModel)
and the selecting host loop of tests/sim_selector_util.py --

  1. the hook: ordered lists, vbar / clear / clear_obj / J / flags and records bit for bit against the mirror on the case list of
     sim_selector_util.cases and on the size cases (rows 2, 63, 64, 65, 115, 256; objects 0, 1, 63, 64, 65, 96), in batches of 1, 63, 64
     and 65 cases;
  2. lockstep: 8 planners x 60 ticks (selector on and off, lists of 1 .. 5 entries, one race of three), the host loop re-seated on the
     device's own state every tick: chosen actions exact, pose / speed / heading within the differential test's 1e-12, ordered lists and
     records bitwise in every tick; the same 60 ticks in ONE sim_run call equal the single ticks bit for bit;
  3. no side effects: one-entry lists with the selector on, and a selector set and cleared, give the trace of a fleet without one;
  4. events: a rewritten preference entry changes the allowed set from the event's own tick on; the user's list, read through a planner
     whose selector is off, is what the event wrote, entry by entry;
  5. branch: a branch onto a planner with the same parameters computes what its source computes bit for bit (the staged list travels),
     branches with different w_switch diverge, parameters and records stay with their destinations; snapshot, run, restore, run with the
     selector on reproduces trace and ordered lists bit for bit;
  6. noise, sensor and tracker on: the rule scores the perceived list -- the mirror fed with the recorder's objects of the tick before;
  7. every refusal.
"""
import os

import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import sim_selector_util as su
import test_gpu_sim_differential as gd
import test_gpu_sim_noise as gn
from graphbasedlocaltrajectoryplanner_amd import sim
from graphbasedlocaltrajectoryplanner_amd.sim import Event

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = {n: i for i, n in enumerate(su.NAMES)}


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
PAR = dict(horizon=2.0, r_ego=1.0, c_hard=0.0, c_soft=1.0, w_clear=1.0, w_switch=2.0)


def pref_ids(entries):
    return [[IDS[a] if isinstance(a, str) else int(a) for a in e["pref"]] for e in entries]


def lists(order):
    return [o.tolist() for o in order]


# ---- 1. the hook --------------------------------------------------------------------------------------------------------------------------
def test_the_hook_equals_the_mirror_bit_for_bit(hip):
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    cs = su.cases()[0] + su.size_cases()
    ref = [su.mirror(c) for c in cs]
    assert {2, 63, 64, 65, 115, 256} <= {a.shape[0] for c in cs for a in c["actions"] if a is not None}
    assert {0, 1, 63, 64, 65, 96} <= {c["objs"].shape[0] for c in cs}
    fleet = Fleet(hip, 1)
    at = 0
    for m in (1, 63, 64, 65):
        idx = [(at + k) % len(cs) for k in range(m)]
        at += m
        order, act_d, act_i, rec = fleet.sim_selector_eval([cs[i]["params"] for i in idx], [cs[i]["user"] for i in idx], [cs[i]["sel_prev"] for i in idx],
                                                           [cs[i]["actions"] for i in idx], [cs[i]["objs"] for i in idx], [cs[i]["emergency"] for i in idx])
        for j, i in enumerate(idx):
            su.compare(dict(order=order[j], act_d=act_d[j], act_i=act_i[j], rec=rec[j]), ref[i], "batch of %d, case %d" % (m, i))
    assert at >= len(cs)                    # every case ran at least once
    # a record handed in is carried on
    c = cs[-1]
    before = su.mirror(cs[0])["rec"]
    got = fleet.sim_selector_eval([c["params"]], [c["user"]], [c["sel_prev"]], [c["actions"]], [c["objs"]], [c["emergency"]], rec=[before])
    assert np.array_equal(bits(got[3][0]), bits(su.mirror(c, before)["rec"]))
    assert fleet.sim_selector_eval(np.zeros((0, 6)), [], [], [], [])[0] == []
    fleet.close()


# ---- 2. lockstep --------------------------------------------------------------------------------------------------------------------------
class Loop(su.Selecting, sl.HostSimLoop):
    def step_sim(self):
        recs = super(Loop, self).step_sim()
        self.log.append(([[IDS[a] for a in o] for o in self.ordered], self.selector.rec.copy()))
        return recs


class SelScenario(gd.Scenario):
    """gd.Scenario with a selector on both sides; every sim_run of the device fleet and every step_sim of the host loop logs the ordered
    lists and the records."""

    def __init__(self, *a, **kw):
        self.skw = kw.pop("selector")
        gd.Scenario.__init__(self, *a, **kw)
        self.users = pref_ids(self.entries)
        self.dev_logs, self.loop = [], None

    def fleet(self, hip):
        fleet = gd.Scenario.fleet(self, hip)
        fleet.sim_selector(**self.skw)
        log, run = [], fleet.sim_run

        def sim_run(n, *a, **kw):
            try:
                return run(n, *a, **kw)
            finally:
                rec, order = fleet.sim_selector_read(raw=True)
                log.append((lists(order), rec))
        fleet.sim_run = sim_run
        self.dev_logs.append(log)
        return fleet

    def host(self, oracle):
        from oracle.planner_host import HostPlannerBackend
        assert self.hmap == list(range(self.n))
        backend = HostPlannerBackend(self.lat)
        loop = Loop(self.lat, self.tab, self.entries, [backend.planner(1, **self.config) for _ in range(self.n)], oracle=oracle, dt=self.dt,
                    n_export=self.n_export)
        for p in range(self.n):
            pos, heading, vel, mho = self.starts[p]
            assert loop.set_start(p, pos, heading, vel, mho)[0], p
            loop.sim_vel(p, **self.vels[p])
        if max(self.sizes) > 1:
            loop.sim_race(self.sizes, length=5.0)
        loop.set_selector(sim.SelectorModel(self.n, **self.skw))
        loop.log = []
        self.loop = loop
        return loop


def lockstep_units(table, track, start):
    s = gn.singles(table, track, start)
    units = [s[0], gn.race3(table), s[1], s[2]]
    for k, (pref, gap) in enumerate(((("follow", "straight"), 60.0), (("straight",), 600.0))):
        units.append(gd.single("chase%d" % k, dict(entry=su.chase_entry(table, start, gap=gap, pref=pref), vel=sl.C2_VEL), start))
    units[2]["entries"][0] = dict(units[2]["entries"][0], pref=("follow", "emergency", "straight", "left", "right"))
    units[3]["entries"][0] = dict(units[3]["entries"][0], pref=("left", "straight", "follow"))
    return units


def test_lockstep_with_the_selecting_host_loop(hip, monteblanco, oracle_backend, table, track, c2_start):
    n_ticks = 60
    skw = dict(PAR, on=[1, 1, 1, 0, 1, 1, 1, 1], w_switch=[2.0, 0.0, 0.5, 0.5, 1.0, 0.2, 0.5, 0.5], horizon=[2.0, 3.0, 1.0, 2.0, 2.5, 2.0, 4.0, 2.0])
    sc = SelScenario(monteblanco, table, lockstep_units(table, track, c2_start), selector=skw)
    assert sc.n == 8 and sorted(len(u) for u in sc.users) == [1, 2, 3, 4, 4, 4, 4, 5]
    worst, stats = gd.both(sc, hip, oracle_backend, n_ticks, "selector")
    single, whole = sc.dev_logs
    assert len(single) == n_ticks == len(sc.loop.log) and len(whole) == 1
    for k, ((d_ord, d_rec), (h_ord, h_rec)) in enumerate(zip(single, sc.loop.log)):
        assert d_ord == h_ord, "tick %d: ordered lists: device %s, host %s" % (k, d_ord, h_ord)
        assert np.array_equal(bits(d_rec), bits(h_rec)), "tick %d: records\n%s\n%s" % (k, d_rec, h_rec)
    assert whole[0][0] == single[-1][0] and np.array_equal(bits(whole[0][1]), bits(single[-1][1]))
    d = sim.selector_dict(single[-1][1])
    print("selector records after %d ticks: %s" % (n_ticks, {k: v.tolist() for k, v in d.items()}))
    assert d["ticks"][3] == 0 and d["ticks"][7] == 0 and np.all(d["ticks"][[0, 1, 2, 4, 5, 6]] == n_ticks - 1)      # off; one entry; the first tick copies
    assert np.any(d["n_scored"] > d["ticks"]) and d["n_switch"].sum() > 0        # the scenario: several actions to rank, actions left


# ---- 3. no side effects -------------------------------------------------------------------------------------------------------------------
def test_one_entry_lists_and_a_cleared_selector_change_nothing(hip, monteblanco, table, track, c2_start):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    units = gn.mixed(table, track, c2_start)
    for u in units:
        u["entries"] = [dict(e, pref=("straight",)) for e in u["entries"]]
    one = gd.Scenario(monteblanco, table, units)
    mixed = gd.Scenario(monteblanco, table, gn.mixed(table, track, c2_start))
    for sc, what in ((one, "one-entry lists, selector on"), (mixed, "set, then cleared")):
        plain = sc.fleet(hip)
        ref = gd.run_one(plain, 20)             # (a planner whose one action is not exported fails alone, on both fleets alike)
        ref_state, ref_digest = plain.sim_state(), plain.digest()
        plain.close()
        fleet = sc.fleet(hip)
        fleet.sim_selector(**PAR)
        if sc is mixed:
            fleet.sim_selector(None)
        tr = gd.run_one(fleet, 20)
        st = fleet.sim_state()
        assert np.array_equal(bits(tr), bits(ref)), what
        assert all(np.array_equal(st[k], ref_state[k]) for k in st) and np.array_equal(fleet.digest(), ref_digest), what
        if sc is mixed:
            with pytest.raises(BackendError, match="the selector is off"):
                fleet.sim_selector_read()
        else:
            d, order = fleet.sim_selector_read()
            assert np.all(d["ticks"] == 0) and lists(order) == [[0]] * sc.n
        fleet.close()
    # sim_setup switches the selector off
    fleet = mixed.fleet(hip)
    fleet.sim_selector(**PAR)
    fleet.sim_setup(mixed.tab, mixed.entries, dt=mixed.dt, n_export=mixed.n_export)
    with pytest.raises(BackendError, match="the selector is off"):
        fleet.sim_selector_read()
    fleet.close()


# ---- 4. events ----------------------------------------------------------------------------------------------------------------------------
def test_an_event_rewrites_the_users_list_and_the_selector_follows(hip, monteblanco, table, c2_start):
    """Two planners with the same list and the same event, the second with the selector off: its "ordered" list is the user's list copied
    entry by entry, so it shows the list as the event wrote it -- the entry, its place, and the tick. The events kernels run in front of the
    selector, so the write counts in the event's own tick (the issue's text says from the next tick on: DESIGN states the deviation)."""
    units = [gd.single("chase%d" % k, dict(entry=su.chase_entry(table, c2_start, pref=("follow", "straight", "straight")), vel=sl.C2_VEL), c2_start)
             for k in range(2)]
    sc = gd.Scenario(monteblanco, table, units)
    fleet = sc.fleet(hip)
    fleet.sim_selector(**dict(PAR, on=[1, 0]))
    fleet.sim_events([Event(p, when=("tick", 10), set=("pref", 2, "right")) for p in range(2)])
    before, after = [su.FOLLOW, su.STRAIGHT, su.STRAIGHT], [su.FOLLOW, su.STRAIGHT, su.RIGHT]
    for k in range(14):
        tr = fleet.sim_run(1)[0][0]
        on, off = lists(fleet.sim_selector_read()[1])
        want = before if k < 10 else after                   # run k is the fleet's tick k
        assert off == want, "run %d: the user's list reads %s, expected %s" % (k, off, want)
        assert sorted(on) == sorted(want), "run %d: the ordered list %s is no permutation of %s" % (k, on, want)
        assert tr[0, 8] == 0 and tr[1, 8] == 0
    fleet.close()


# ---- 5. branch ----------------------------------------------------------------------------------------------------------------------------
def test_branches_with_different_w_switch_diverge(hip, monteblanco, table, c2_start):
    """Planner 0 branched onto three others. Planner 1 has planner 0's parameters and a history of its own (another gap): behind the branch
    it computes what planner 0 computes, bit for bit -- sel, the exported set AND the staged list travelled. Planners 2 and 3 have other
    w_switch and diverge. Records stay with their destinations."""
    units = [gd.single("chase%d" % k, dict(entry=su.chase_entry(table, c2_start, gap=(100.0, 40.0, 100.0, 100.0)[k]), vel=sl.C2_VEL), c2_start)
             for k in range(4)]
    sc = gd.Scenario(monteblanco, table, units)
    fleet = sc.fleet(hip)
    fleet.sim_selector(**dict(PAR, c_soft=8.0, w_switch=[2.0, 2.0, 0.0, 1000.0]))
    tr0 = fleet.sim_run(60)[0]
    assert not np.array_equal(tr0[-1, 0, 5:8], tr0[-1, 1, 5:8])          # planner 1 staged another list than planner 0
    before = fleet.sim_selector_read(raw=True)[0]
    fleet.sim_branch(0, [1, 2, 3])
    st = fleet.sim_state()
    assert all(np.array_equal(st['pos_est'][p], st['pos_est'][0]) for p in (1, 2, 3))
    assert np.array_equal(bits(fleet.sim_selector_read(raw=True)[0]), bits(before))               # the records stay with their destinations
    orders = []
    for k in range(140):
        tr = fleet.sim_run(1)[0][0]
        orders.append(lists(fleet.sim_selector_read()[1]))
        assert np.array_equal(bits(tr[1]), bits(tr[0])) and orders[-1][1] == orders[-1][0], "tick %d behind the branch: planner 1 left planner 0" % k
    d = fleet.sim_selector_read()[0]
    acts = [sorted(set(o[p][0] for o in orders)) for p in range(4)]
    print("first ordered entries behind the branch: %s; n_switch %s, n_override %s" % (acts, d["n_switch"].tolist(), d["n_override"].tolist()))
    assert any(o[2] != o[3] for o in orders), "the branches with w_switch 0 and 1000 did not diverge"
    assert np.all(d["ticks"] == 199)
    fleet.close()


def test_a_restored_snapshot_reproduces_the_run_with_the_selector_on(hip, monteblanco, table, track, c2_start):
    """Snapshot, run, restore, run: trace and ordered lists of the second run equal the first bit for bit. The selector reads the staged
    list of the tick before, so the list is state and travels with the snapshot; behind the first run the live list is a later tick's."""
    sc = gd.Scenario(monteblanco, table, gn.mixed(table, track, c2_start))
    fleet = sc.fleet(hip)
    fleet.sim_selector(**dict(PAR, c_soft=8.0, w_switch=0.2))
    fleet.sim_run(50)
    fleet.sim_snapshot(0)
    runs = []
    for rep in range(2):
        ticks = []
        for k in range(30):
            tr = fleet.sim_run(1)[0][0]
            ticks.append((tr.copy(), lists(fleet.sim_selector_read()[1])))
        runs.append(ticks)
        cnt_end = ticks[-1][0][:, 5].copy()
        if rep == 0:
            fleet.sim_restore(0)
    for k, ((ta, oa), (tb, ob)) in enumerate(zip(*runs)):
        assert oa == ob, "tick %d behind the restore: ordered lists %s, first run %s" % (k, ob, oa)
        assert np.array_equal(bits(ta), bits(tb)), "tick %d behind the restore: the trace differs" % k
    assert cnt_end.sum() > 0                                  # objects were staged and scored
    # a snapshot taken without a selector holds no list: the restored planners start from empty lists, and say so in their records
    fleet.sim_selector(None)
    fleet.sim_snapshot(1)
    fleet.sim_selector(**dict(PAR, c_soft=8.0, w_switch=0.2))
    fleet.sim_restore(1)
    fleet.sim_run(1)
    d = fleet.sim_selector_read()[0]
    assert np.all(d["ticks"] == 1) and np.all(d["clear_min"] == np.inf)
    fleet.close()


# ---- 6. the perceived list ----------------------------------------------------------------------------------------------------------------
def test_the_selector_scores_what_noise_sensor_and_tracker_hand_on(hip, monteblanco, table, track, c2_start):
    from graphbasedlocaltrajectoryplanner_amd.planner import KEY_IDS
    sc = gd.Scenario(monteblanco, table, gn.mixed(table, track, c2_start))
    users = pref_ids(sc.entries)
    skw = dict(PAR, c_soft=6.0, w_switch=0.3)
    fleet = sc.fleet(hip)
    fleet.sim_noise(**gn.noise_args(sc.n))
    fleet.sim_sensor(range=150.0, fov_deg=200.0, occl=1.0, p_drop=0.15, seed=np.arange(sc.n, dtype=np.uint64) + np.uint64(3))
    fleet.sim_tracker()
    fleet.sim_selector(**skw)
    fleet.sim_record(list(range(sc.n)), depth=1)
    model = sim.SelectorModel(sc.n, **skw)
    prev, scored_objs = None, 0
    for k in range(40):
        tr = fleet.sim_run(1)[0][0]
        rec, order = fleet.sim_selector_read(raw=True)
        order = lists(order)
        for p in range(sc.n):
            w = "tick %d planner %d" % (k, p)
            if prev is None:
                exp, keys = users[p], {su.STRAIGHT}
            else:
                traj = prev[p]["traj"][0]
                actions, objs, emergency = su.tick_inputs(traj, prev[p]["vehicles"], sc.n_export)
                exp = model.select(p, users[p], KEY_IDS[prev[p]["sel"]], actions, objs, emergency)
                keys = {KEY_IDS[key] for key in traj}
                scored_objs += len(objs)
            assert order[p] == exp, "%s: ordered list %s, mirror %s" % (w, order[p], exp)
            assert np.array_equal(bits(rec[p]), bits(model.rec[p])), "%s: record\n%s\n%s" % (w, rec[p], model.rec[p])
            assert tr[p, 8] == 0 and tr[p, 0] == sim.selector_first(exp, keys), "%s: action %s of %s" % (w, tr[p, 0], exp)
        prev = fleet.sim_record_read()[-1]
    print("perceived objects scored: %d; records %s" % (scored_objs, {k: v.tolist() for k, v in model.as_dict().items()}))
    assert scored_objs > 0 and model.rec[:, 0].min() == 39
    fleet.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_every_refusal(hip, table):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    fleet = Fleet(hip, 2)
    with pytest.raises(BackendError, match="ltpl_fleet_sim_setup first"):
        fleet.sim_selector(**PAR)
    fleet.sim_setup(table, [ENTRY, ENTRY])
    with pytest.raises(BackendError, match="the selector is off"):
        fleet.sim_selector_read()
    for bad, text in ((dict(horizon=0.0), "horizon"), (dict(horizon=[1.0, -2.0]), "planner 1: horizon"), (dict(r_ego=-1.0), "r_ego"),
                      (dict(w_clear=-0.5), "w_clear"), (dict(w_switch=[-1e-300, 0.0]), "planner 0: w_switch"), (dict(c_hard=np.nan), "NaN"),
                      (dict(c_soft=[0.0, np.nan]), "planner 1: a parameter is NaN"), (dict(horizon=np.nan), "NaN")):
        with pytest.raises(BackendError, match=text):
            fleet.sim_selector(**dict(PAR, **bad))
    with pytest.raises(ValueError):
        fleet.sim_selector(bogus=1.0)
    fleet.sim_selector(**dict(PAR, c_hard=-np.inf))
    with pytest.raises(BackendError, match="horizon"):           # a refused call keeps the previous selector
        fleet.sim_selector(**dict(PAR, horizon=-1.0))
    d, order = fleet.sim_selector_read()
    assert np.all(d["ticks"] == 0) and np.all(d["clear_min"] == np.inf) and lists(order) == pref_ids([ENTRY, ENTRY])
    line = su.line(5)
    for kw, text in ((dict(params=[su.params(horizon=-1.0)]), "horizon"), (dict(users=[[0, 7]]), "unknown action"), (dict(users=[[0] * 6]), "1 .. 5 entries"),
                     (dict(objs=[np.zeros((97, 5))]), "0 .. 96 objects")):
        a = dict(dict(params=[su.params()], users=[[0, 2]], sel_prev=[0], actions=[[line, None, line, None]], objs=[np.zeros((0, 5))]), **kw)
        with pytest.raises(BackendError, match=text):
            fleet.sim_selector_eval(a["params"], a["users"], a["sel_prev"], a["actions"], a["objs"])
    fleet.close()
