"""
CPU: scripted events of the fleet simulation (ltpl_fleet_sim_events / _events_read, include/ltpl_hip.h; csrc/fleet_events.hpp) on the host.

  1. The binding and the header declare the two entry points and the constants.
  2. The argument checks, what a refused or failing call keeps, and the launches per tick on the stand-in runtime
     (tools/fakehip/sim_events_args.py, plain build).
  3. ``sim.EventScript``, the host mirror of the two kernels, on made-up states: every condition on both sides of its boundary, chains,
     the order of application, a failed planner, at most once.
  4. The seeded scenarios of tests/test_gpu_sim_events.py on the free-running host loop are not vacuous: every condition kind fires,
     some trigger never fires, and an opponent that brakes changes what its planner selects.
The kernels themselves are tested on the device: tests/test_gpu_sim_events.py.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import planner_replay as pr
import sim_events_util as eu
import sim_loop as sl
from graphbasedlocaltrajectoryplanner_amd import sim
from graphbasedlocaltrajectoryplanner_amd.sim import Event, EventScript

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. ---------------------------------------------------------------------------------------------------------------------------
def test_binding_and_header_declare_the_entry_points_and_constants():
    from graphbasedlocaltrajectoryplanner_amd import fleet
    assert fleet.SIM_MAX_TRIGGERS == sim.MAX_TRIGGERS == 16
    for name in ("sim_events", "sim_events_read"):
        assert callable(getattr(fleet.Fleet, name)), name
    with open(os.path.join(ROOT, "include", "ltpl_hip.h")) as fh:
        hdr = fh.read()
    assert "#define LTPL_FLEET_SIM_MAX_TRIGGERS 16" in hdr
    for name in ("ltpl_fleet_sim_events(", "ltpl_fleet_sim_events_read(", "} ltpl_fleet_sim_events_in;"):
        assert name in hdr, name
    import re
    for prefix, table in (("LTPL_SIM_WHEN_", sim.WHEN_KINDS), ("LTPL_SIM_SET_", sim.SET_KINDS)):
        found = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define %s(\w+)\s+(\d+)" % prefix, hdr)}
        assert found == table, (found, table)
    fields = [n for n, _ in fleet.SimEventsIn._fields_]
    assert fields == ["n_events", "ev_off", "when_kind", "when_index", "when_value", "set_kind", "set_index", "set_value"]
    assert all(re.search(r"\*\s+%s;" % f, hdr) for f in fields[1:])


# ---- 2. ---------------------------------------------------------------------------------------------------------------------------
def test_event_entry_points_check_their_arguments_without_a_device():
    env = dict(os.environ, FAKEHIP_SAN="none", LTPL_NO_SELFTEST="1")
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "sim_events_args.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and "sim events args OK" in p.stdout, p.stdout[-3000:]
    for line in ("refused run:", "launches per tick:", "emergency launches: tick k", "emergency launches: a flag set by an event", "previous list kept"):
        assert line in p.stdout, (line, p.stdout[-3000:])
    assert p.stdout.count("refused (") >= 27, p.stdout[-3000:]


# ---- 3. ---------------------------------------------------------------------------------------------------------------------------
class Line(object):
    """A straight race line along x (what EventScript reads of a RaceLineTable): the opponent at arc length s stands at (s, 0)."""

    def lists(self):
        s = [10.0 * k for k in range(1, 101)]
        return [s, list(s), [0.0] * len(s), [0.0] * len(s), [10.0] * len(s)]


def state(pos=((0.0, 0.0),), vel=(0.0,), opp_s=((),), failed=None):
    return dict(pos=[list(p) for p in pos], vel=list(vel), opp_s=[list(o) for o in opp_s], failed=failed)


def fired(script, st):
    return [(i, w) for i, _, w in script.before_tick(st)]


def test_speed_conditions_are_strict():
    v = 7.25
    for kind, at, inside in (("vel_below", v, math.nextafter(v, -math.inf)), ("vel_above", v, math.nextafter(v, math.inf))):
        sc = EventScript([Event(0, when=(kind, v), set=("gg_scale", 0.5))], 1)
        assert fired(sc, state(vel=(at,))) == [] and sc.fired_tick[0] == -1                   # equal: not yet
        assert fired(sc, state(vel=(inside,))) == [(0, ("gg_scale", 0, 0.5))] and sc.fired_tick[0] == 1
        assert fired(sc, state(vel=(inside,))) == [] and sc.fired_tick[0] == 1 and sc.tick == 3   # at most once


def test_distance_condition_includes_its_boundary():
    # the opponent at (300, 0), the ego at (297, 4): dist^2 = 25 exactly
    st = state(pos=((297.0, 4.0),), opp_s=((300.0,),))
    for d, fires in ((5.0, True), (math.nextafter(5.0, 0.0), False), (math.nextafter(5.0, 6.0), True), (0.0, False)):
        sc = EventScript([Event(0, when=("opp_within", 0, d), set=("opp_vel_scale", 0, 0.2))], 1, race=Line())
        assert sc.opp_dist2(st, 0, 0) == 25.0
        assert bool(fired(sc, st)) == fires, d
    # between two knots and beyond both ends of the table (np.interp clamps); flat opp_s with offsets reads the planner's own opponent
    sc = EventScript([Event(1, when=("opp_within", 1, 1.0), set=("opp_vel_scale", 1, 0.2))], 2, race=Line())
    flat = dict(pos=[[0.0, 0.0], [1000.0, 0.5]], vel=[0.0, 0.0], opp_s=[1000.0, 500.0, 2000.0], opp_off=[0, 1, 3])
    assert sc.opp_dist2(flat, 1, 1) == 0.25 and sc.opp_dist2(flat, 1, 0) == 500.0 ** 2 + 0.25 and sc.opp_dist2(flat, 0, 0) == 1000.0 ** 2
    assert fired(sc, flat) == [(0, ("opp_vel_scale", 1, 0.2))]
    assert EventScript([], 1, race=Line()).opp_dist2(state(pos=((4.0, 3.0),), opp_s=((1.0,),)), 0, 0) == 36.0 + 9.0     # below s_rl[0]: the first row


def test_after_chains_and_the_order_of_application():
    ev = [Event(0, when=("vel_above", 1.0), set=("safety_d", 20.0)),          # 0
          Event(0, when=("after", 0, 2), set=("safety_d", 25.0)),             # 1: two ticks after 0
          Event(0, when=("after", 1, 1), set=("pref", 1, "left")),            # 2: one tick after 1
          Event(0, when=("vel_above", 1.0), set=("safety_d", 10.0)),          # 3: fires with 0, later in the list: it wins
          Event(0, when=("tick", 3), set=("safety_d", 40.0)),                 # 4: timed, in the tick in which 1 fires: applied first
          Event(1, when=("tick", 3), set=("incl_emerg", True)),               # 5
          Event(1, when=("vel_below", 0.0), set=("vel_max", 50.0))]           # 6: never
    sc = EventScript(ev, 2)
    slow, fast = state(pos=((0, 0), (0, 0)), vel=(0.5, 0.5), opp_s=((), ())), state(pos=((0, 0), (0, 0)), vel=(1.5, 0.5), opp_s=((), ()))
    assert fired(sc, slow) == []                                                                  # tick 0
    assert fired(sc, fast) == [(0, ("safety_d", 0, 20.0)), (3, ("safety_d", 0, 10.0))]            # tick 1: list order, the later one last
    assert fired(sc, slow) == []                                                                  # tick 2 (a condition that held once need not hold on)
    assert fired(sc, slow) == [(4, ("safety_d", 0, 40.0)), (5, ("incl_emerg", 0, True)), (1, ("safety_d", 0, 25.0))]     # tick 3: timed first
    assert fired(sc, slow) == [(2, ("pref", 1, "left"))]                                          # tick 4
    assert fired(sc, fast) == [] and sc.tick == 6
    assert sc.fired_tick.tolist() == [1, 3, 4, 1, 3, 3, -1]
    # applied in this order to a host loop's configuration, the last write stands
    class Loop(object):
        cfg = [dict(opp=[], static=[], pref=["right", "straight"])]
        velkw = [dict(safety_d=30.0)]
    sc = EventScript(ev[:5], 1)
    for st in (slow, fast, slow, slow, slow):
        eu.apply_writes(Loop, sc.before_tick(dict(st, pos=st["pos"][:1], vel=st["vel"][:1], opp_s=[()])))
    assert Loop.velkw[0]["safety_d"] == 25.0 and Loop.cfg[0]["pref"] == ["right", "left"]


def test_a_failed_planner_fires_nothing():
    ev = [Event(0, when=("tick", 1), set=("gg_scale", 0.5)), Event(0, when=("vel_above", 1.0), set=("safety_d", 20.0)),
          Event(1, when=("tick", 1), set=("gg_scale", 0.6)), Event(1, when=("vel_above", 1.0), set=("safety_d", 21.0)),
          Event(0, when=("after", 1, 1), set=("vel_max", 50.0))]
    sc = EventScript(ev, 2)
    st = state(pos=((0, 0), (0, 0)), vel=(2.0, 2.0), opp_s=((), ()), failed=[True, False])
    assert fired(sc, st) == [(3, ("safety_d", 0, 21.0))]
    assert fired(sc, st) == [(2, ("gg_scale", 0, 0.6))]
    assert fired(sc, dict(st, failed=[False, False])) == [(1, ("safety_d", 0, 20.0))]             # revived: its triggers are still armed,
    assert fired(sc, st) == [] and sc.fired_tick.tolist() == [-1, 2, 1, 0, -1]                    # the timed event's tick has passed; a chain
    assert fired(sc, dict(st, failed=[False, False])) == []                                       # whose tick passed while failed is lost


def test_script_refuses_what_the_library_refuses():
    for ev in ([Event(0, when=("after", 0, 1), set=("gg_scale", 0.5))],
               [Event(0, when=("tick", 1), set=("gg_scale", 0.5)), Event(0, when=("after", 0, 1), set=("gg_scale", 0.5))],
               [Event(0, when=("vel_above", 1.0), set=("gg_scale", 0.5)), Event(0, when=("after", 0, 0), set=("gg_scale", 0.5))],
               [Event(0, when=("vel_above", 1.0), set=("incl_emerg", True))],
               [Event(0, when=("vel_above", 1.0 + k), set=("gg_scale", 0.5)) for k in range(17)],
               [Event(1, when=("tick", 1), set=("gg_scale", 0.5))]):
        with pytest.raises(ValueError):
            EventScript(ev, 1)
    with pytest.raises(ValueError):
        Event(0, when=("sometime", 1), set=("gg_scale", 0.5))
    with pytest.raises(ValueError):
        Event(0, when=("tick", 1), set=("opp_length", 4.0))
    a = sim.pack_events([Event(1, ("tick", 4), ("gg_scale", 0.5)), Event(0, ("vel_below", 2.0), ("pref", 1, "left")), Event(1, ("tick", 2), ("gg_ay", 3.0))], 3)
    assert a["ev_off"].tolist() == [0, 1, 3, 3] and a["order"].tolist() == [1, 0, 2] and a["when_index"].tolist() == [0, 4, 2]
    assert a["set_kind"].tolist() == [7, 9, 11] and a["set_value"].tolist() == [2.0, 0.5, 3.0] and a["set_index"].tolist() == [1, 0, 0]


# ---- 4. ---------------------------------------------------------------------------------------------------------------------------
def test_seeded_event_scenarios_are_not_vacuous(monteblanco, oracle_backend):
    from oracle.planner_host import HostPlannerBackend
    track = np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz"))
    table = sim.RaceLineTable.from_track(track)
    start = pr.load_ticks("c2")[0]['start']
    host = HostPlannerBackend(monteblanco)
    entries, events, classes, start_vel = eu.scenario(tuple(start['pos']), track, 5)
    assert classes == ["brake", "statics", "many", "statics2", "plain"]
    # the same list with the two writes of planner 0's braking opponent turned into writes of the value it has anyway
    no_brake = [Event(0, e.when, ("opp_vel_scale", 0, eu.BRAKE_SCALE0)) if e.planner == 0 and e.set[0] == "opp_vel_scale" else e for e in events]

    def run(events):
        loop = sl.HostSimLoop(monteblanco, table, entries, [host.planner(1) for _ in entries], oracle=oracle_backend)
        for h in range(len(entries)):
            assert loop.set_start(h, start['pos'], start['heading'], start_vel[h], start['max_heading_offset'])[0]
            loop.sim_vel(h, **sl.C2_VEL)
        script = EventScript(events, len(entries), race=table)
        sels, cnts = [], []
        for _ in range(eu.EVENT_TICKS):
            eu.apply_writes(loop, script.before_tick(eu.loop_state(loop)))
            recs = loop.tick()
            assert not any(r["failed"] for r in recs)
            sels.append([r["sel"] for r in recs])
            cnts.append([r["cnt"] for r in recs])
        return script, sels, cnts
    script, sels, cnts = run(events)
    script0, sels0, cnts0 = run(no_brake)
    ft = script.fired_tick
    by_kind = {}
    for e, t in zip(events, ft):
        by_kind.setdefault(e.when[0], []).append(int(t))
    assert all(any(t >= 0 for t in by_kind[k]) for k in ("tick", "opp_within", "vel_above", "after")), by_kind
    assert any(t < 0 for k in ("vel_below", "vel_above", "opp_within", "after") for t in by_kind.get(k, ())), by_kind     # some trigger never fires
    assert any(t > 0 for t in by_kind["opp_within"]) and any(t > 0 for t in by_kind["vel_above"]), by_kind                 # ... and not all at once
    assert 0 in by_kind["tick"] and eu.SPLIT - 1 in by_kind["tick"] and eu.SPLIT in by_kind["tick"]
    # the braking opponent of planner 0 fired, and accelerated again; its planner selects something else in a later tick than in the same
    # loop whose opponent does not brake (every other event as it is)
    brake = next(i for i, e in enumerate(events) if e.planner == 0 and e.when[0] == "opp_within")
    assert 0 < ft[brake] and ft[brake + 1] == ft[brake] + eu.BRAKE_TICKS < eu.EVENT_TICKS - 1
    assert script0.fired_tick[brake] == ft[brake]
    assert all(a[0] == b[0] for a, b in zip(sels[:ft[brake]], sels0[:ft[brake]]))
    assert any(a[0] != b[0] for a, b in zip(sels[ft[brake]:], sels0[ft[brake]:])), (ft[brake], [a[0] for a in sels], [b[0] for b in sels0])
    # the static of planner 1 that is moved onto the track is taken in from its tick on (the loop without events: never)
    _, _, cnts_off = run([])
    assert cnts[4][1] == cnts_off[4][1] and cnts[5][1] == cnts_off[5][1] + 1
