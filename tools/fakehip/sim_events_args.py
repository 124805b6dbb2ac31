"""TEST TOOL: argument checks and launch bookkeeping of ltpl_fleet_sim_events / ltpl_fleet_sim_events_read (scripted events of the fleet
simulation, csrc/fleet_events.hpp) without a device. The library's host code built against the stand-in runtime without sanitizers
(FAKEHIP_SAN=none tools/fakehip/build.sh); kernels do nothing, so no event ever fires here -- only the return codes, the messages, what
``events_read`` reports and the number of kernel launches:
  - every refused call (null fleet, no simulation, an index out of range, an 'after' that points forward or at a timed event, delay 0,
    the emergency flag on a trigger, a duplicate timed write, 17 triggers, bad values) returns its status and a message that names the
    planner and the event, before any device allocation, and launches nothing; a refused call keeps the previous list and its tick;
  - a run whose list holds a friction event while no maps are set is refused before its first launch and allocation;
  - an allocation failing at each allocation of ltpl_fleet_sim_events leaves the previous list, its tick and its size unchanged;
  - launches per tick: unchanged without events and with a list that is switched off again; + 1 in exactly the ticks whose bucket of
    timed events is not empty; + 1 in every tick while the list holds triggers;
  - timed emergency-flag events: tick k launches what a run split at k (ltpl_fleet_sim_vel in between) launches; a flag an event set keeps
    these launches after the list is switched off or replaced, until ltpl_fleet_sim_vel sets the flags anew."""
import ctypes

import numpy as np

import sim_args_common as common
from sim_args_common import CAPACITY, INVALID, UNSUPPORTED, _capi, expect, launches_out as launches, msg, quiet, sim
from graphbasedlocaltrajectoryplanner_amd.fleet import SimEventsIn
from graphbasedlocaltrajectoryplanner_amd.sim import Event

N = 6
lib, fleet, table = common.start(N)
OPPONENTS = (1, 1, 0, 2, 1, 1)
STATICS = (0, 2, 0, 0, 1, 0)
lib.ltpl_fleet_sim_events.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.ltpl_fleet_sim_events_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
h = fleet.handle


def set_events(events):
    """ltpl_fleet_sim_events through the raw entry point: (status, message)."""
    a = sim.pack_events(events, N)
    ei = SimEventsIn()
    ei.n_events = len(events)
    for k in ("ev_off", "when_kind", "when_index", "when_value", "set_kind", "set_index", "set_value"):
        setattr(ei, k, a[k].ctypes.data)
    return lib.ltpl_fleet_sim_events(h, ctypes.byref(ei)), msg()


def read():
    n, tick = ctypes.c_int32(-7), ctypes.c_int32(-7)
    fired = np.full(1024, -5, np.int32)
    rc = lib.ltpl_fleet_sim_events_read(h, fired.ctypes.data, ctypes.byref(n), ctypes.byref(tick))
    return rc, n.value, tick.value, fired[:max(n.value, 0)].tolist()


def fresh(**vel):
    common.fresh([dict(common.GOOD_ENTRY, opponents=[(250.0 + 100.0 * k, 0.3, 5.0) for k in range(no)],
                       static=[(10.0 * k, 5.0, 0.0, 0.0, 4.0) for k in range(ns)]) for no, ns in zip(OPPONENTS, STATICS)], **vel)


def per_tick(n):
    return [launches(lambda: fleet.sim_run(1, trace=False))[0] for _ in range(n)]


T, W, B, A = "tick", "opp_within", "vel_below", "after"
GG = ("gg_scale", 0.8)

# null fleet, no simulation
assert lib.ltpl_fleet_sim_events(None, None) == INVALID and lib.ltpl_fleet_sim_events_read(None, None, None, None) == INVALID
expect(quiet(lambda: set_events([Event(0, (T, 1), GG)])), INVALID, "ltpl_fleet_sim_setup first")
assert quiet(lambda: lib.ltpl_fleet_sim_events(h, None)) == INVALID and "ltpl_fleet_sim_setup first" in msg()
assert quiet(lambda: lib.ltpl_fleet_sim_events_read(h, None, None, None)) == INVALID and "ltpl_fleet_sim_setup first" in msg()

fresh()
plain = per_tick(3)
assert len(set(plain)) == 1
plain = plain[0]
assert read() == (0, 0, 0, [])                                                            # events are off
assert quiet(lambda: lib.ltpl_fleet_sim_events(h, None)) == 0                               # switching off what is off: nothing to do

# a valid list first: every refusal below has to keep it
good = [Event(3, (W, 1, 40.0), ("opp_vel_scale", 1, 0.2)), Event(3, (A, 0, 5), ("opp_vel_scale", 1, 0.5)), Event(0, (T, 2), GG),
        Event(5, (T, 2), ("safety_d", 20.0)), Event(1, (T, 4), ("static_x", 1, 3.0))]
n_launch, rc = launches(lambda: set_events(good))
assert rc[0] == 0 and n_launch == 0, (rc, n_launch)
assert read() == (0, 5, 0, [-1] * 5)
assert per_tick(2) == [plain + 1, plain + 1] and read()[:3] == (0, 5, 2)
held = read()

REFUSALS = [
    # index out of range
    ([Event(2, (W, 0, 40.0), GG)], INVALID, ("planner 2 event 0", "opponent 0 out of range")),
    ([Event(0, (T, 0), GG), Event(0, (W, 1, 40.0), GG)], INVALID, ("planner 0 event 1", "opponent 1 out of range")),
    ([Event(3, (W, -1, 40.0), GG)], INVALID, ("planner 3 event 0", "out of range")),
    ([Event(4, (T, 0), ("opp_length", 1, 4.0))], INVALID, ("planner 4 event 0", "opponent 1 out of range")),
    ([Event(4, (T, 0), ("static_v", 1, 4.0))], INVALID, ("planner 4 event 0", "static object 1 out of range")),
    ([Event(0, (T, 0), ("static_x", 0, 4.0))], INVALID, ("planner 0 event 0", "static object 0 out of range")),
    ([Event(1, (T, 0), ("pref", 2, "left"))], INVALID, ("planner 1 event 0", "preference entry 2 out of range")),
    ([Event(1, (T, -1), GG)], INVALID, ("planner 1 event 0", "tick must not be negative")),
    # 'after': forward, itself, at a timed event, delay 0 / fractional
    ([Event(1, (A, 1, 5), GG), Event(1, (B, 3.0), GG)], INVALID, ("planner 1 event 0", "earlier event")),
    ([Event(1, (B, 3.0), GG), Event(1, (A, 1, 5), GG)], INVALID, ("planner 1 event 1", "earlier event")),
    ([Event(1, (T, 3), GG), Event(1, (A, 0, 5), ("vel_max", 50.0))], INVALID, ("planner 1 event 1", "use LTPL_SIM_WHEN_TICK")),
    ([Event(1, (B, 3.0), GG), Event(1, (A, 0, 0), ("vel_max", 50.0))], INVALID, ("planner 1 event 1", "delay")),
    ([Event(1, (B, 3.0), GG), Event(1, (A, 0, 2.5), ("vel_max", 50.0))], INVALID, ("planner 1 event 1", "delay")),
    # the emergency flag on a trigger
    ([Event(5, (B, 3.0), ("incl_emerg", True))], UNSUPPORTED, ("planner 5 event 0", "LTPL_SIM_WHEN_TICK only")),
    ([Event(5, (W, 0, 30.0), GG), Event(5, (A, 0, 3), ("incl_emerg", False))], UNSUPPORTED, ("planner 5 event 1", "LTPL_SIM_WHEN_TICK only")),
    # a duplicate timed write
    ([Event(4, (T, 7), ("opp_length", 0, 4.0)), Event(4, (T, 6), GG), Event(4, (T, 7), ("opp_length", 0, 6.0))], INVALID,
     ("planner 4 event 2", "event 0", "same tick 7")),
    # values
    ([Event(0, (W, 0, -1.0), GG)], INVALID, ("planner 0 event 0", "distance")),
    ([Event(0, (W, 0, float("nan")), GG)], INVALID, ("planner 0 event 0", "distance")),
    ([Event(0, (B, float("inf")), GG)], INVALID, ("planner 0 event 0", "speed")),
    ([Event(0, (T, 0), ("gg_scale", 0.0))], INVALID, ("planner 0 event 0", "positive")),
    ([Event(0, (T, 0), ("opp_length", 0, 0.0))], INVALID, ("planner 0 event 0", "positive")),
    ([Event(0, (T, 0), ("opp_vel_scale", 0, -0.1))], INVALID, ("planner 0 event 0", "negative")),
    ([Event(0, (T, 0), ("safety_d", float("nan")))], INVALID, ("planner 0 event 0", "finite")),
    ([Event(0, (T, 0), ("pref", 0, 5))], INVALID, ("planner 0 event 0", "unknown action")),
    ([Event(0, (T, 0), ("pref", 0, -1))], INVALID, ("planner 0 event 0", "unknown action")),
    ([Event(0, (T, 0), ("friction_scale", -1.0))], INVALID, ("planner 0 event 0", "positive")),
    # 17 triggers
    ([Event(3, (B, 1.0 + k), GG) for k in range(17)], CAPACITY, ("planner 3", "more than 16 triggers")),
]
for events, code, texts in REFUSALS:
    expect(quiet(lambda: set_events(events)), code, *texts)
    assert read() == held, "a refused call changed the list"
# the same timed write in another tick, for another index or another planner is no duplicate; 16 triggers and many timed events are fine
ok = [Event(4, (T, 7), ("opp_length", 0, 4.0)), Event(4, (T, 8), ("opp_length", 0, 6.0)), Event(3, (T, 7), ("opp_length", 0, 4.0)),
      Event(3, (T, 7), ("opp_length", 1, 4.0))] + [Event(3, (B, 1.0 + k), GG) for k in range(16)] + \
     [Event(0, (T, k), ("vel_max", 60.0 + k)) for k in range(400)]
assert set_events(ok)[0] == 0 and read()[1:3] == (len(ok), 0)
# raw structure errors
ei = SimEventsIn()
ei.n_events = 2
assert quiet(lambda: lib.ltpl_fleet_sim_events(h, ctypes.byref(ei))) == INVALID and "array is missing" in msg()
ei.n_events = -1
assert quiet(lambda: lib.ltpl_fleet_sim_events(h, ctypes.byref(ei))) == INVALID and "negative" in msg()
a = sim.pack_events(good, N)
for k in ("ev_off", "when_kind", "when_index", "when_value", "set_kind", "set_index", "set_value"):
    setattr(ei, k, a[k].ctypes.data)
ei.n_events = 4                                                                           # ev_off ends at 5
assert quiet(lambda: lib.ltpl_fleet_sim_events(h, ctypes.byref(ei))) == INVALID and "ev_off" in msg()
a["when_kind"][0] = 9
ei.n_events = 5
assert quiet(lambda: lib.ltpl_fleet_sim_events(h, ctypes.byref(ei))) == INVALID and "unknown condition kind 9" in msg()
a["when_kind"][0], a["set_kind"][0] = 0, 15
assert quiet(lambda: lib.ltpl_fleet_sim_events(h, ctypes.byref(ei))) == INVALID and "unknown write kind 15" in msg()
assert read()[1:3] == (len(ok), 0)

# a friction event without maps: accepted when the list is set, the run is refused before its first launch and allocation
assert set_events([Event(2, (T, 1), ("friction_scale", 0.7))])[0] == 0


def refused_run():
    try:
        fleet.sim_run(2, trace=True)
    except _capi.BackendError as e:
        return str(e)
    return None


m = quiet(refused_run)
assert m is not None and "LTPL_SIM_SET_FRICTION_SCALE" in m and "no friction maps" in m, m
assert read()[1:3] == (1, 0)                                                              # (no tick ran)
print("refused run: %s" % m)
fleet.sim_events(None)
assert read() == (0, 0, 0, []) and per_tick(2) == [plain, plain]

# launches per tick
fresh()
fleet.sim_events([Event(0, (T, 1), GG), Event(5, (T, 1), GG), Event(2, (T, 4), GG), Event(2, (T, 5), ("vel_max", 70.0))])
got = per_tick(7)
assert got == [plain, plain + 1, plain, plain, plain + 1, plain + 1, plain], (got, plain)
assert read()[1:3] == (4, 7)
fleet.sim_events([Event(1, (T, 2), GG)])                                                  # a new list: the tick starts at 0 again
assert read()[1:3] == (1, 0)
n_launch, _ = launches(lambda: fleet.sim_run(5, trace=False))                             # ... and goes on across calls
assert n_launch == 5 * plain + 1 and read()[2] == 5 and per_tick(2) == [plain, plain]
fleet.sim_events([Event(1, (T, 2), GG), Event(4, (B, 1.0), GG), Event(4, (A, 0, 3), ("vel_max", 70.0))])
assert per_tick(4) == [plain + 1, plain + 1, plain + 2, plain + 1]
fleet.sim_events([])
assert per_tick(2) == [plain, plain]
fleet.sim_events([Event(4, (B, 1.0), GG)])
fresh()                                                                                   # sim_setup switches the events off
assert read() == (0, 0, 0, []) and per_tick(2) == [plain, plain]
print("launches per tick: %d without events, + 1 in the ticks of a timed event, + 1 per tick with triggers" % plain)

# timed emergency-flag events: tick k launches what a run split at k launches
PATTERN = {1: (0, True), 3: (4, True), 4: (0, False), 6: (4, False), 8: (2, True), 9: (2, False)}      # tick: (planner, flag)
fresh(incl_emerg_traj=False)
flags = [False] * N
split = []
for k in range(11):
    if k in PATTERN:
        flags[PATTERN[k][0]] = PATTERN[k][1]
        fleet.sim_vel(incl_emerg_traj=list(flags))
    split.append(launches(lambda: fleet.sim_run(1, trace=False))[0])
assert len(set(split)) == 2 and split[0] == plain and split[1] > plain and split[5] > plain and split[6] == plain and split[8] > plain and split[9] == plain, split
fresh(incl_emerg_traj=False)
fleet.sim_events([Event(p, (T, k), ("incl_emerg", v)) for k, (p, v) in PATTERN.items()])
scripted = per_tick(11)
assert scripted == [n + (1 if k in PATTERN else 0) for k, n in enumerate(split)], (scripted, split)
n_launch, _ = launches(lambda: (fleet.sim_events([Event(p, (T, k), ("incl_emerg", v)) for k, (p, v) in PATTERN.items()]), fleet.sim_run(11, trace=False)))
assert n_launch == sum(scripted), (n_launch, sum(scripted))                               # (all flags were off again: the same in one call)
fleet.sim_vel(incl_emerg_traj=True)                                                       # a later sim_vel sets the flags, and the shadow, anew
fleet.sim_events([Event(p, (T, 1), ("incl_emerg", False)) for p in range(N)])
assert per_tick(3) == [split[1], plain + 1, plain]
print("emergency launches: tick k of the scripted run launches what the run split at k launches (%s)" % split)

# a flag an event wrote is configuration: it keeps its launches when the list is switched off or replaced, until sim_vel sets the flags anew
emerg = split[1]                                                                          # launches of a tick of sim_vel(incl_emerg_traj=[.. True ..])
fresh(incl_emerg_traj=False)
fleet.sim_events([Event(3, (T, 1), ("incl_emerg", True))])
assert per_tick(3) == [plain, emerg + 1, emerg]
fleet.sim_events(None)
assert per_tick(2) == [emerg, emerg], "the emergency launches went with the list"
fleet.sim_events([Event(0, (B, -1.0), GG)])
assert per_tick(1) == [emerg + 1]
fleet.sim_events([])
fleet.sim_vel(incl_emerg_traj=False)
assert per_tick(1) == [plain]
print("emergency launches: a flag set by an event keeps them after the list is switched off (%d per tick), sim_vel takes them back (%d)" % (emerg, plain))

# an allocation failing at each allocation of ltpl_fleet_sim_events: the previous list, its tick and its size stay
def list_at_tick_3():
    fresh()
    assert set_events(good)[0] == 0
    fleet.sim_run(3, trace=False)
    held = read()
    assert held[1:3] == (5, 3)
    return held


def list_kept(k, held):
    assert read() == held, (k, read(), held)
    assert per_tick(1) == [plain + 1] and read()[2] == 4                                  # (the kept list still runs: its triggers)


def new_list():
    assert read()[1:3] == (len(ok), 0)


failures = common.alloc_sweep("ltpl_fleet_sim_events", lambda: set_events(ok), 40, list_kept, before=list_at_tick_3, after_success=new_list)
assert failures >= 11, failures
print("allocation failure at each of the %d allocations of ltpl_fleet_sim_events: previous list kept" % failures)
common.finish("sim events args OK")
