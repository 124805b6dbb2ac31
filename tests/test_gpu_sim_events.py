"""
GPU: scripted events of the fleet simulation (ltpl_fleet_sim_events / _events_read, include/ltpl_hip.h; csrc/fleet_events.hpp:
k_fleet_sim_events_timed, k_fleet_sim_triggers at the head of every tick of ltpl_fleet_sim_run).

  5. Recordings in ONE call: car2, overtake (64 planners) and filt5 with the changes of the recording's velocity arguments as timed events:
     the trace equals the split run's (test_gpu_fleet_sim.run_split) bit for bit and passes check_trace; the fired ticks are the change ticks.
  6. The other timed kinds against the existing entry points, bitwise: the grip factor against ltpl_fleet_friction_scale between two
     runs, vel_max / safety_d at per-planner DIFFERENT ticks against a fleet split at every distinct tick with ltpl_fleet_sim_vel.
  7. Differential against the host loop (tests/sim_loop.py driven by sim.EventScript, tests/sim_events_util.py) in the lockstep of
     tests/test_gpu_sim_differential.py, with that module's bounds: opponent, static and preference events, every trigger kind, fleets of
     1, 64 and 65 planners whose neighbours carry different opponent counts, a trigger on opponent 66 of 70, planners with 0 and 16
     triggers, 65 timed events in one tick, events at tick 0 and in every tick's own call; then the same in one call, bit for bit,
     fired ticks included.
  8. Decision boundaries of the three state conditions, from the device's own state.
  9. A list that never fires changes nothing; a failed planner fires nothing; snapshot / branch leave the list alone and the written
     configuration with the destination; a later sim_vel overwrites an event's value; two fleets on one handle.
tests/test_sim_events_host.py shows on the CPU that the scenarios of 7 are not vacuous.
"""
import math
import os

import numpy as np
import pytest

import planner_replay as pr
import sim_events_util as eu
import sim_loop as sl
import test_gpu_fleet_sim as gs
import test_gpu_sim_differential as gd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip(monteblanco):
    from graphbasedlocaltrajectoryplanner_amd import _capi
    return _capi.HipBackend(monteblanco)


@pytest.fixture(scope="module")
def track():
    return np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz"))


@pytest.fixture(scope="module")
def race(track):
    from graphbasedlocaltrajectoryplanner_amd.sim import RaceLineTable
    return RaceLineTable.from_track(track)


@pytest.fixture(scope="module")
def c2():
    return pr.load_ticks("c2")


def c2_fleet(hip, monteblanco, race, ticks, n, entries=None):
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    fleet = Fleet(hip, n)
    gs.start(fleet, [(ticks, range(n))])
    fleet.sim_setup(race, entries or [gs.planner_entry(monteblanco, "c2", ticks)] * n)
    return fleet


def same_bits(a, b, what):
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: first difference at (tick, planner, field) %s" % (
        what, np.argwhere((a != b) & ~(np.isnan(a) & np.isnan(b)))[:1])


def same_state(a, b, what):
    sa, sb = a.sim_state(), b.sim_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), "%s: %s" % (what, k)
    assert np.array_equal(a.sim_heading(), b.sim_heading()) and np.array_equal(a.digest(), b.digest()), what


# ---- 5. recordings in one call -------------------------------------------------------------------------------------------------------
def vel_events(ticks, planners):
    """The changes of a recording's velocity arguments as timed events of every planner; returns (events, {tick: events per planner})."""
    from graphbasedlocaltrajectoryplanner_amd.sim import Event
    events, per_tick = [], {}
    for k in range(1, len(ticks)):
        a, b = gs.vel_of(ticks[k - 1]), gs.vel_of(ticks[k])
        assert np.array_equal(np.asarray(a["ax_max_machines"]), np.asarray(b["ax_max_machines"]))       # (no event kind: machine tables do not change)
        sets = [(key, float(b[key])) for key in ("vel_max", "gg_scale", "safety_d") if a[key] != b[key]]
        sets += [(key, float(b["local_gg"][i])) for i, key in enumerate(("gg_ax", "gg_ay")) if a["local_gg"][i] != b["local_gg"][i]]
        if bool(a["incl_emerg_traj"]) != bool(b["incl_emerg_traj"]):
            sets.append(("incl_emerg", bool(b["incl_emerg_traj"])))
        for p in planners:
            events += [Event(p, when=("tick", k), set=s) for s in sets]
        if sets:
            per_tick[k] = len(sets)
    return events, per_tick


@pytest.mark.parametrize("name,n", [("car2", 1), ("overtake", 64), ("filt5", 1)])
def test_recording_in_one_call_equals_the_split_run(hip, monteblanco, race, name, n):
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    ticks = pr.load_ticks(name)
    T = len(ticks)
    traces = []
    for scripted in (False, True):
        fleet = Fleet(hip, n, **gs.SPECS[name][2])
        gs.start(fleet, [(ticks, range(n))])
        fleet.sim_setup(race, [gs.planner_entry(monteblanco, name, ticks)] * n)
        if not scripted:
            traces.append(gs.run_split(fleet, [ticks], [range(n)], T))
        else:
            events, per_tick = vel_events(ticks, range(n))
            assert len(per_tick) == len(gs.segments([ticks], T)) - 1 > 0
            gs.set_vel(fleet, [ticks], [range(n)], 0)
            fleet.sim_events(events)
            traces.append(fleet.sim_run(T)[0])                                  # ONE call
            rd = fleet.sim_events_read()
            assert rd["tick"] == T and rd["fired_tick"].tolist() == [e.when_index for e in events]
            print("\n%s: %d planners x %d ticks in one call, %d timed events in %d ticks (the split run: %d calls)" % (
                name, n, T, len(events), len(per_tick), len(per_tick) + 1))
        fleet.close()
    same_bits(traces[1], traces[0], name)
    gs.check_trace(traces[1], ticks, list(range(n)), name)


# ---- 6. the other timed kinds against the existing entry points -----------------------------------------------------------------------
def test_friction_scale_event_equals_friction_scale_between_two_runs(hip, monteblanco, race, c2):
    from graphbasedlocaltrajectoryplanner_amd.friction import FrictionGrid
    from graphbasedlocaltrajectoryplanner_amd.sim import Event
    grid = FrictionGrid.load(os.path.join(ROOT, "tests", "golden", "friction_grid.npz"))
    n, K, T = 3, 9, 30
    s0, s1 = [0.9, 0.9, 0.8], [0.7, 0.9, 1.0]                                   # planners 0 and 1: the same until the event
    out = []
    for scripted in (False, True):
        fleet = c2_fleet(hip, monteblanco, race, c2, n)
        fleet.friction(grid, scale=s0)
        gs.set_vel(fleet, [c2], [range(n)], 0)
        if scripted:
            fleet.sim_events([Event(p, when=("tick", K), set=("friction_scale", s1[p])) for p in (0, 2)])
            tr = fleet.sim_run(T)[0]
            assert fleet.sim_events_read()["fired_tick"].tolist() == [K, K]
        else:
            a = fleet.sim_run(K)[0]
            fleet.friction_scale(s1)
            tr = np.concatenate([a, fleet.sim_run(T - K)[0]])
        out.append((tr, fleet))
    same_bits(out[1][0], out[0][0], "friction scale event")
    same_state(out[1][1], out[0][1], "friction scale event")
    tr = out[1][0]
    assert np.array_equal(tr[:K, 0], tr[:K, 1], equal_nan=True) and not np.array_equal(tr[K:, 0], tr[K:, 1], equal_nan=True)   # (the event matters)
    for _, fleet in out:
        fleet.close()


def test_per_planner_ticks_equal_a_fleet_split_at_every_distinct_tick(hip, monteblanco, race, c2):
    from graphbasedlocaltrajectoryplanner_amd.sim import Event
    n, T = 5, 30
    base = gs.vel_of(c2[0])
    # planner p: vel_max at a tick of its own, safety_d at another (planner 4: both in one tick, planner 3: none)
    # (vel_max stays above the planned speed of the start phase, 5 m/s: below it the planner stops with the reference's ValueError)
    plan = {0: [(4, "vel_max", 30.0), (11, "safety_d", 12.0)], 1: [(7, "vel_max", 25.0), (13, "safety_d", 45.0)],
            2: [(4, "safety_d", 20.0), (19, "vel_max", 35.0)], 4: [(16, "vel_max", 40.0), (16, "safety_d", 10.0)]}
    events = [Event(p, when=("tick", k), set=(key, v)) for p, rows in plan.items() for k, key, v in rows]
    cuts = sorted(set(k for rows in plan.values() for k, _, _ in rows))
    assert len(cuts) == 6
    ref = c2_fleet(hip, monteblanco, race, c2, n)
    cur = dict(vel_max=[base["vel_max"]] * n, safety_d=[base["safety_d"]] * n)
    parts, a = [], 0
    for b in cuts + [T]:
        ref.sim_vel(local_gg=tuple(base["local_gg"]), gg_scale=base["gg_scale"], ax_max_machines=base["ax_max_machines"],
                    incl_emerg_traj=bool(base["incl_emerg_traj"]), **cur)
        parts.append(ref.sim_run(b - a)[0])
        for p, rows in plan.items():
            for k, key, v in rows:
                if k == b:
                    cur[key] = list(cur[key])
                    cur[key][p] = v
        a = b
    fleet = c2_fleet(hip, monteblanco, race, c2, n)
    fleet.sim_vel(local_gg=tuple(base["local_gg"]), gg_scale=base["gg_scale"], ax_max_machines=base["ax_max_machines"],
                  incl_emerg_traj=bool(base["incl_emerg_traj"]), vel_max=base["vel_max"], safety_d=base["safety_d"])
    fleet.sim_events(events)
    tr = fleet.sim_run(T)[0]
    assert fleet.sim_events_read()["fired_tick"].tolist() == [e.when_index for e in events]
    same_bits(tr, np.concatenate(parts), "per-planner ticks")
    same_state(fleet, ref, "per-planner ticks")
    assert not np.array_equal(tr[-1, 0], tr[-1, 3])                              # (the limits matter: planner 3 keeps the recording's)
    fleet.close()
    ref.close()


# ---- 7. differential against the host loop ---------------------------------------------------------------------------------------------
class EventScenario(gd.Scenario):
    """A fleet of sim_events_util.scenario with its event list; the host loop applies the writes sim.EventScript decides, from the state
    the lockstep seated it on. Fired ticks are read when a fleet is closed."""

    def __init__(self, lat, tab, track, start, n):
        entries, events, classes, start_vel = eu.scenario(tuple(start['pos']), track, n)
        units = [dict(cls=c, entries=[e], vels=[sl.C2_VEL], starts=[(start['pos'], start['heading'], v, start['max_heading_offset'])])
                 for c, e, v in zip(classes, entries, start_vel)]
        gd.Scenario.__init__(self, lat, tab, units)
        self.events, self.classes, self.read, self.script = events, classes, [], None

    def fleet(self, hip):
        fleet = gd.Scenario.fleet(self, hip)
        fleet.sim_events(self.events)
        close = fleet.close

        def read_and_close():
            self.read.append(fleet.sim_events_read())
            close()
        fleet.close = read_and_close
        return fleet

    def host(self, oracle):
        from graphbasedlocaltrajectoryplanner_amd.sim import Event, EventScript
        loop = gd.Scenario.host(self, oracle)
        host_of = {p: h for h, p in enumerate(self.hmap)}
        self.host_events = [i for i, e in enumerate(self.events) if e.planner in host_of]
        self.script = EventScript([Event(host_of[self.events[i].planner], self.events[i].when, self.events[i].set) for i in self.host_events],
                                  len(self.hmap), race=self.tab)
        step_sim = loop.step_sim

        def events_then_step():
            eu.apply_writes(loop, self.script.before_tick(eu.loop_state(loop)))
            return step_sim()
        loop.step_sim = events_then_step
        return loop


@pytest.mark.parametrize("n", [1, 64, 65])
def test_events_against_the_host_loop(hip, monteblanco, oracle_backend, race, track, c2, n):
    sc = EventScenario(monteblanco, race, track, c2[0]['start'], n)
    cnt = np.diff(sc.opp_off)
    if n > 1:
        assert np.all(cnt[1:n - 1] != cnt[:n - 2]) and cnt.max() == 70 and cnt.min() == 0          # neighbours carry different opponent counts
        per = np.bincount([e.planner for e in sc.events if e.when[0] != "tick"], minlength=n)
        assert per.max() == 16 and per.min() == 0
        assert sum(1 for e in sc.events if e.when == ("tick", 3)) == n
    worst, stats = gd.both(sc, hip, oracle_backend, eu.EVENT_TICKS, "events n=%d" % n)
    assert stats['errors'] == 0, stats
    lock, one = sc.read
    assert lock["tick"] == one["tick"] == eu.EVENT_TICKS
    assert np.array_equal(lock["fired_tick"], one["fired_tick"])                                  # one call: the lockstep run's fired ticks
    ft = lock["fired_tick"]
    assert np.array_equal(ft[sc.host_events], sc.script.fired_tick), (ft[sc.host_events], sc.script.fired_tick)
    # every planner of a kind: the fired ticks of the kind's first planner (which the host computed)
    by_planner = {}
    for i, e in enumerate(sc.events):
        by_planner.setdefault(e.planner, []).append(int(ft[i]))
    first = {}
    for p in range(n):
        assert by_planner[p] == by_planner[first.setdefault(sc.classes[p], p)], p
    kinds = {}
    for i, e in enumerate(sc.events):
        kinds.setdefault(e.when[0], []).append(int(ft[i]))
    assert all(t >= 0 for t in kinds["tick"]) and 0 in kinds["tick"] and eu.SPLIT - 1 in kinds["tick"] and eu.SPLIT in kinds["tick"]
    assert any(t > 0 for t in kinds["opp_within"]) and any(t > 0 for t in kinds["vel_above"]) and any(t > 0 for t in kinds["after"])
    assert all(t < 0 for t in kinds["vel_below"])
    print("events n=%d: fired ticks by condition kind %s" % (n, {k: sorted(set(v)) for k, v in kinds.items()}))


# ---- 8. decision boundaries ------------------------------------------------------------------------------------------------------------
def first_tick(series, cond):
    return next((k for k, v in enumerate(series) if cond(v)), -1)


def test_conditions_at_their_decision_boundaries(hip, monteblanco, race, c2):
    """Planner 0 accelerates behind an opponent it closes in on, planner 1 starts at 15 m/s and brakes. The state in front of every tick is
    read from a fleet without events; the thresholds are that state's own values and their neighbours. Every event writes the value its
    target has anyway, so the run with events is the run without, bit for bit, and the series holds for it."""
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    from graphbasedlocaltrajectoryplanner_amd.sim import Event, EventScript
    st = c2[0]['start']
    T = 24
    entries = [dict(eu.entry(tuple(st['pos']), [(120.0, 0.2, 5.0)]), vel_est=15.0),
               dict(eu.entry(tuple(st['pos']), [(60.0, 0.2, 5.0)]), vel_est=15.0)]

    def make():
        fleet = Fleet(hip, 2)
        for p in range(2):
            assert fleet.set_start(p, st['pos'], st['heading'], 15.0, st['max_heading_offset'])[0]
        fleet.sim_setup(race, entries)
        fleet.sim_vel(**sl.C2_VEL)
        return fleet
    ref = make()
    mirror = EventScript([], 2, race=race)
    vel, d2, rows = [], [], []
    for k in range(T):
        state = eu.fleet_state(ref, [0, 1, 2])
        vel.append(state["vel"].copy())
        d2.append([mirror.opp_dist2(state, p, 0) for p in range(2)])
        rows.append(ref.sim_run(1)[0])
    vel, d2 = np.array(vel), np.array(d2)
    # ticks in front of which the value is a strict new extreme: nothing with a threshold at that value fired before
    up = next(k for k in range(T - 1, 0, -1) if vel[k, 0] > vel[:k, 0].max())
    down = next(k for k in range(T - 1, 0, -1) if vel[k, 1] < vel[:k, 1].min())
    near = next(k for k in range(T - 1, 0, -1) if d2[k, 0] < d2[:k, 0].min())
    assert min(up, down, near) >= 5, (up, down, near)
    v_up, v_down, q = float(vel[up, 0]), float(vel[down, 1]), float(d2[near, 0])
    d_hi = math.sqrt(q)
    while d_hi * d_hi < q:
        d_hi = math.nextafter(d_hi, math.inf)
    while math.nextafter(d_hi, 0.0) ** 2 >= q:
        d_hi = math.nextafter(d_hi, 0.0)
    d_lo = math.nextafter(d_hi, 0.0)
    assert d_lo * d_lo < q <= d_hi * d_hi
    same = ("opp_vel_scale", 0, 0.2)
    events = [Event(0, when=("vel_above", v_up), set=same), Event(0, when=("vel_above", math.nextafter(v_up, -math.inf)), set=same),
              Event(1, when=("vel_below", v_down), set=same), Event(1, when=("vel_below", math.nextafter(v_down, math.inf)), set=same),
              Event(0, when=("opp_within", 0, d_hi), set=same), Event(0, when=("opp_within", 0, d_lo), set=same)]
    fleet = make()
    fleet.sim_events(events)
    tr = fleet.sim_run(T)[0]
    same_bits(tr, np.concatenate(rows), "boundaries")
    ft = fleet.sim_events_read()["fired_tick"].tolist()
    print("\nboundaries: vel_above at tick %d (%r), vel_below at tick %d (%r), opp_within at tick %d (dist^2 %r, d %r | %r): fired %s" % (
        up, v_up, down, v_down, near, q, d_lo, d_hi, ft))
    assert ft[1] == up and ft[0] != up and ft[0] == first_tick(vel[:, 0], lambda v: v > v_up)
    assert ft[3] == down and ft[2] != down and ft[2] == first_tick(vel[:, 1], lambda v: v < v_down)
    assert ft[4] == near and ft[5] != near and ft[5] == first_tick(d2[:, 0], lambda v: v <= d_lo * d_lo)
    fleet.close()
    ref.close()


# ---- 9. nothing else changes; interplay --------------------------------------------------------------------------------------------------
def test_a_list_that_never_fires_changes_nothing(hip, monteblanco, race, c2):
    from graphbasedlocaltrajectoryplanner_amd.sim import Event
    n, T = 3, 25
    never = [Event(0, when=("vel_below", -1.0), set=("gg_scale", 0.5)), Event(0, when=("after", 0, 1), set=("vel_max", 5.0)),
             Event(1, when=("opp_within", 7, 0.0), set=("opp_vel_scale", 7, 0.0)), Event(1, when=("vel_above", 1.0e9), set=("pref", 0, "follow")),
             Event(2, when=("tick", T), set=("safety_d", 1.0)), Event(2, when=("tick", 10 ** 9), set=("incl_emerg", True))]
    out = []
    for events in (None, never):
        fleet = c2_fleet(hip, monteblanco, race, c2, n)
        gs.set_vel(fleet, [c2], [range(n)], 0)
        fleet.sim_telemetry()
        fleet.sim_events(events)
        out.append((fleet.sim_run(T)[0], fleet))
    same_bits(out[1][0], out[0][0], "never firing list")
    same_state(out[1][1], out[0][1], "never firing list")
    ta, tb = out[0][1].sim_telemetry_read(), out[1][1].sim_telemetry_read()
    assert all(np.array_equal(ta[k], tb[k], equal_nan=True) for k in ta)
    off = out[0][1].sim_events_read()
    assert off["tick"] == 0 and off["fired_tick"].size == 0
    rd = out[1][1].sim_events_read()
    assert rd["tick"] == T and rd["fired_tick"].tolist() == [-1] * len(never)
    for _, fleet in out:
        fleet.close()


def test_a_failed_planner_fires_nothing(hip, monteblanco, race, c2):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.sim import Event
    e = gs.planner_entry(monteblanco, "c2", c2)
    fleet = c2_fleet(hip, monteblanco, race, c2, 3, [e, dict(e, pref=("right",)), e])       # planner 1: no matching action in tick 0
    gs.set_vel(fleet, [c2], [range(3)], 0)
    events = []
    for p in range(3):
        events += [Event(p, when=("tick", 0), set=("gg_scale", 0.9)), Event(p, when=("tick", 4), set=("safety_d", 25.0)),
                   Event(p, when=("vel_above", -1.0), set=("vel_max", 80.0)), Event(p, when=("after", 2, 2), set=("gg_ax", 4.5)),
                   Event(p, when=("opp_within", 0, 1.0e5), set=("opp_length", 0, 4.0))]
    fleet.sim_events(events)
    with pytest.raises(BackendError, match="planner 1: closed-loop simulation"):
        fleet.sim_run(8)
    tr = fleet.last_trace
    assert np.all(tr[:, 1, 8] != 0) and np.all(tr[:, [0, 2], 8] == 0)
    ft = fleet.sim_events_read()["fired_tick"].reshape(3, 5).tolist()
    # planner 1 is healthy in front of tick 0 only: what fires there fires; the chain's tick (2) and the timed tick 4 pass while it is failed
    assert ft[0] == ft[2] == [0, 4, 0, 2, 0] and ft[1] == [0, -1, 0, -1, 0], ft
    same_bits(tr[:, 0], tr[:, 2], "neighbours of the failed planner")
    fleet.close()


def test_snapshot_and_branch_leave_the_list_alone_and_sim_vel_overwrites(hip, monteblanco, race, c2):
    from graphbasedlocaltrajectoryplanner_amd.sim import Event
    n = 2
    fleet = c2_fleet(hip, monteblanco, race, c2, n)
    gs.set_vel(fleet, [c2], [range(n)], 0)
    # planner 1's opponents 0 and 3 stop at tick 2; a chain is in flight across the branch; a timed event lies behind it
    events = [Event(1, when=("tick", 2), set=("opp_vel_scale", 0, 0.0)), Event(1, when=("tick", 2), set=("opp_vel_scale", 3, 0.0)),
              Event(0, when=("vel_above", -1.0), set=("safety_d", 28.0)), Event(0, when=("after", 0, 7), set=("safety_d", 26.0)),
              Event(1, when=("tick", 9), set=("gg_scale", 0.95))]
    fleet.sim_events(events)
    fleet.sim_run(5)
    fleet.sim_snapshot(0)
    before = fleet.sim_events_read()
    assert before["tick"] == 5 and before["fired_tick"].tolist() == [2, 2, 0, -1, -1]
    fleet.sim_run(1)
    fleet.sim_branch(0, [1])                                   # live planner 0 -> planner 1: state travels, configuration stays
    rd = fleet.sim_events_read()
    assert rd["tick"] == 6 and rd["fired_tick"].tolist() == before["fired_tick"].tolist()
    fleet.sim_restore(0)                                       # both planners back to tick 5: the schedule tick is not rewound
    rd = fleet.sim_events_read()
    assert rd["tick"] == 6 and rd["fired_tick"].tolist() == before["fired_tick"].tolist()
    s0 = fleet.sim_state()
    fleet.sim_run(4)
    s1 = fleet.sim_state()
    rd = fleet.sim_events_read()
    assert rd["tick"] == 10 and rd["fired_tick"].tolist() == [2, 2, 0, 7, 9]
    o0, o1 = s0["opp_s"].reshape(n, -1), s1["opp_s"].reshape(n, -1)
    moved = o1 != o0
    assert moved[0].all() and moved[1].tolist() == [False, True, True, False, True, True, True, True]      # the written configuration stayed
    fleet.close()
    # a later sim_vel sets its arrays anew: the event's value is gone, and it is not applied again
    base = gs.vel_of(c2[0])
    kw = dict(local_gg=tuple(base["local_gg"]), gg_scale=base["gg_scale"], ax_max_machines=base["ax_max_machines"], vel_max=base["vel_max"],
              incl_emerg_traj=bool(base["incl_emerg_traj"]))
    a = c2_fleet(hip, monteblanco, race, c2, n)
    a.sim_vel(safety_d=base["safety_d"], **kw)
    a.sim_events([Event(0, when=("tick", 1), set=("safety_d", 10.0))])
    ta = [a.sim_run(3)[0]]
    a.sim_vel(safety_d=base["safety_d"], **kw)
    ta.append(a.sim_run(5)[0])
    assert a.sim_events_read()["tick"] == 8 and a.sim_events_read()["fired_tick"].tolist() == [1]
    b = c2_fleet(hip, monteblanco, race, c2, n)
    b.sim_vel(safety_d=base["safety_d"], **kw)
    tb = [b.sim_run(1)[0]]
    b.sim_vel(safety_d=[10.0, base["safety_d"]], **kw)
    tb.append(b.sim_run(2)[0])
    b.sim_vel(safety_d=base["safety_d"], **kw)
    tb.append(b.sim_run(5)[0])
    same_bits(np.concatenate(ta), np.concatenate(tb), "sim_vel after an event")
    same_state(a, b, "sim_vel after an event")
    a.close()
    b.close()


def test_two_fleets_on_one_handle(hip, monteblanco, race, c2):
    from graphbasedlocaltrajectoryplanner_amd.sim import Event
    lists = ([Event(0, when=("tick", 3), set=("safety_d", 12.0)), Event(1, when=("vel_above", 0.02), set=("opp_vel_scale", 0, 0.1))],
             [Event(0, when=("tick", 5), set=("vel_max", 30.0)), Event(0, when=("vel_above", 0.04), set=("pref", 0, "left")),
              Event(2, when=("vel_above", 0.04), set=("gg_ay", 4.0)), Event(2, when=("after", 0, 2), set=("gg_scale", 0.8)),
              Event(2, when=("tick", 3), set=("safety_d", 40.0))])
    sizes = (2, 3)

    def make(k):
        fleet = c2_fleet(hip, monteblanco, race, c2, sizes[k])
        gs.set_vel(fleet, [c2], [range(sizes[k])], 0)
        fleet.sim_events(lists[k])
        return fleet
    solo = []
    for k in range(2):
        fleet = make(k)
        solo.append((fleet.sim_run(12)[0], fleet.sim_events_read()["fired_tick"].tolist()))
        fleet.close()
    both = [make(0), make(1)]
    parts = [[], []]
    for a, b in ((0, 4), (4, 5), (5, 12)):                      # interleaved: each fleet keeps its own list, tick and fired ticks
        for k in range(2):
            parts[k].append(both[k].sim_run(b - a)[0])
    for k in range(2):
        same_bits(np.concatenate(parts[k]), solo[k][0], "fleet %d of two" % k)
        rd = both[k].sim_events_read()
        assert rd["tick"] == 12 and rd["fired_tick"].tolist() == solo[k][1] and all(t >= 0 for t in solo[k][1]), (k, rd, solo[k][1])
        both[k].close()


def test_emergency_flag_event_of_a_failed_planner_and_flags_after_the_list_is_switched_off(hip, monteblanco, race, c2):
    """The one write that does not ask for the error word: the host shapes the launches of the emergency stage from its shadow of the flags,
    so the device takes a timed incl_emerg event of a FAILED planner as well (the event is not marked fired). Shown by reviving the
    planner with a neighbour's state -- configuration stays the destination's own -- after the list was switched off: the shadow still
    launches the emergency stage, and the revived planner, alone, exports an emergency trajectory."""
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.sim import Event
    e = gs.planner_entry(monteblanco, "c2", c2)
    fleet = c2_fleet(hip, monteblanco, race, c2, 3, [e, dict(e, pref=("right",)), e])       # planner 1: no matching action in tick 0
    assert not any(bool(t['vel_args']['incl_emerg_traj']) for t in c2[:12])
    gs.set_vel(fleet, [c2], [range(3)], 0)
    fleet.sim_events([Event(1, when=("tick", 2), set=("incl_emerg", True)), Event(2, when=("tick", 3), set=("safety_d", 25.0))])
    with pytest.raises(BackendError, match="planner 1: closed-loop simulation"):
        fleet.sim_run(6)
    assert np.all(fleet.last_trace[:, 1, 8] != 0)
    rd = fleet.sim_events_read()
    assert rd["tick"] == 6 and rd["fired_tick"].tolist() == [-1, 3]
    assert all("emergency" not in fleet.trajectories(p)[0] for p in (0, 2))
    fleet.sim_events(None)                                     # the flag and the host's shadow of it are configuration: they stay
    fleet.sim_branch(0, [1])                                   # planner 0's state revives planner 1 ('right' is on offer by now)
    tr, _ = fleet.sim_run(3)
    assert np.all(tr[:, :, 8] == 0)
    assert "emergency" in fleet.trajectories(1)[0] and "emergency" not in fleet.trajectories(0)[0]
    fleet.close()
