"""TEST TOOL: argument checks of ltpl_fleet_sim_react / ltpl_fleet_sim_react_read / ltpl_fleet_sim_react_eval (the reactive opponents of the
fleet simulation, csrc/fleet_react.hpp) without a device. The library's host code built against the stand-in runtime without sanitizers
(FAKEHIP_SAN=none tools/fakehip/build.sh); kernels do nothing, so no scale is looked at -- only the return codes, the messages and the
kernel launches (by number and, through fakehip_launches_of, by name):
  - every refused call (null fleet, no simulation, a missing array, an `on` that is neither 0 nor 1, an a_max / b_comf / b_max / look that
    is not positive, a negative headway / gap0 / lat_gate / ego_len, a NaN anywhere, an infinity anywhere but look = +inf, a negative
    tick0, an unknown flag; the read's record size; the hook's counts, arrays, offsets, dt, tick, parameters and opponents) returns
    LTPL_ERR_INVALID_ARG with a message that names the argument, before any device allocation, and launches nothing;
  - a refused or failing call keeps the previous model (the tick still launches k_fleet_sim_react, the records stay readable); an
    allocation failing at each allocation of the call is LTPL_ERR_HIP, and the fleet runs on;
  - per tick a fleet with the model set launches k_fleet_sim_react once, one kernel more than before whatever else runs; a fleet that had
    one and cleared it (in == NULL, or on == 0 for every planner), and one after ltpl_fleet_sim_setup, launch what a fleet that never had
    one launches, k_fleet_sim_react never; ltpl_fleet_sim_race and ltpl_fleet_sim_predictor keep it;
  - snapshot and branch launch k_fleet_sim_branch_react only while the model is set."""
import ctypes

import numpy as np

import sim_args_common as common
from sim_args_common import I32, INVALID, P, expect, launches, msg, quiet, run1, sim
from graphbasedlocaltrajectoryplanner_amd.fleet import SimReactIn

N = 4
lib, fleet, table = common.start(N)
lib.ltpl_fleet_sim_react.argtypes = [P, P]
lib.ltpl_fleet_sim_react_read.argtypes = [P, P, I32, P]
lib.ltpl_fleet_sim_react_eval.argtypes = [P, I32] + [P] * 10
h = fleet.handle
RD = sim.REACT_DOUBLES
NAMES = sim.REACT_PARAMS[1:]
POSITIVE = ("a_max", "b_comf", "b_max", "look")


GOOD = dict(sim.REACT_DEFAULTS)


def react(missing=None, on=1, tick0=0, flags=0, **par):
    keep = [np.ascontiguousarray(np.broadcast_to(np.asarray(on, np.int32), (N,)))]
    si = SimReactIn()
    si.on = None if missing == "on" else keep[0].ctypes.data
    for k in NAMES:
        keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(dict(GOOD, **par)[k], np.float64), (N,))))
        setattr(si, k, None if k == missing else keep[-1].ctypes.data)
    si.tick0, si.flags = tick0, flags
    return lib.ltpl_fleet_sim_react(h, ctypes.byref(si)), msg()


REACT = b"_Z17k_fleet_sim_react"         # the whole mangled name up to the arguments: 17 = len("k_fleet_sim_react"), so the hook
                                        # k_fleet_sim_react_eval (_Z22...) does not match
BRANCH = b"_Z24k_fleet_sim_branch_react"


def named(fn, name=REACT):
    return common.named(fn, name)


def fresh():
    entries = common.moving_entries(N)
    for p in range(1, N, 2):
        entries[p]["opponents"] = [(250.0, 0.3, 5.0), (300.0, 0.2, 5.0)]
    common.fresh(entries)


out, eff = np.zeros((N, RD)), np.zeros(16)


def read(size=RD, rec=True, scales=True):
    return lib.ltpl_fleet_sim_react_read(h, out.ctypes.data if rec else None, size, eff.ctypes.data if scales else None), msg()


# null fleet, no simulation
assert lib.ltpl_fleet_sim_react(None, None) == INVALID and lib.ltpl_fleet_sim_react_read(None, out.ctypes.data, RD, None) == INVALID
assert lib.ltpl_fleet_sim_react_eval(None, 0, *([None] * 10)) == INVALID
expect(quiet(lambda: react()), "ltpl_fleet_sim_setup first")
expect(quiet(lambda: (lib.ltpl_fleet_sim_react(h, None), msg())), "ltpl_fleet_sim_setup first")
expect(quiet(read), "ltpl_fleet_sim_setup first")
expect(quiet(lambda: (lib.ltpl_fleet_sim_react_eval(h, 1, *([None] * 10)), msg())), "ltpl_fleet_sim_setup first")

fresh()
plain = launches(run1)
assert named(run1) == 0
expect(quiet(read), "the model is off")
assert quiet(lambda: lib.ltpl_fleet_sim_react(h, None)) == 0                # clearing what is off: nothing to do, nothing allocated
assert quiet(lambda: react(on=0))[0] == 0 and named(run1) == 0              # on == 0 everywhere: off, nothing allocated


def refusals():
    for name in ("on",) + NAMES:
        expect(quiet(lambda: react(missing=name)), name + " missing")
    for name in NAMES:
        word = " must be positive" if name in POSITIVE else " must not be negative"
        for bad in ((0.0, -1.0, [1.0, 1.0, 1.0, -1e-300]) if name in POSITIVE else (-1.0, [0.0, 0.0, 0.0, -5e-324])):
            expect(quiet(lambda: react(**{name: bad})), name + word)
        for bad in (np.nan, -np.inf) + (() if name == "look" else (np.inf,)):
            expect(quiet(lambda: react(**{name: [GOOD[name], bad, GOOD[name], GOOD[name]]})), "planner 1: " + name + " must be finite")
    for bad in (2, -1, [1, 0, 1, 7]):
        expect(quiet(lambda: react(on=bad)), "on must be 0 or 1")
    expect(quiet(lambda: react(tick0=-1)), "tick0")
    expect(quiet(lambda: react(flags=2)), "unknown flag")


refusals()
# the edges that are arguments
assert react(a_max=5e-324, b_comf=5e-324, b_max=5e-324, headway=0.0, gap0=0.0, look=np.inf, lat_gate=0.0, ego_len=0.0)[0] == 0
assert react(on=[1, 0, 1, 0], tick0=2 ** 31 - 1, flags=1)[0] == 0           # (KEEP_STATE on a set model)
with_react = launches(run1)
assert with_react == plain + 1, (with_react, plain)
assert named(run1) == 1
assert read()[0] == 0
expect(quiet(lambda: read(size=RD - 1)), "record size")
expect(quiet(lambda: read(rec=False)), "out missing")
assert read(scales=False)[0] == 0                                            # (without the scales)
# a refused call keeps the previous model
refusals()
assert named(lambda: fleet.sim_run(3, trace=False)) == 3 and read()[0] == 0
# snapshot and branch copy scales and record with a kernel of their own, only while a model is set
assert named(lambda: fleet.sim_snapshot(0), BRANCH) == 1 and named(lambda: fleet.sim_restore(0), BRANCH) == 1
assert named(lambda: fleet.sim_branch(0, [2]), BRANCH) == 1
assert lib.ltpl_fleet_sim_react(h, None) == 0
assert launches(run1) == plain and named(run1) == 0                          # set, then cleared: what a fleet that never had one launches
expect(quiet(read), "the model is off")
assert named(lambda: fleet.sim_snapshot(1), BRANCH) == 0 and named(lambda: fleet.sim_restore(0), BRANCH) == 0
assert named(lambda: fleet.sim_branch(0, [2]), BRANCH) == 0
assert react()[0] == 0 and named(run1) == 1
assert react(on=0)[0] == 0 and launches(run1) == plain and named(run1) == 0  # on == 0 for every planner switches it off
expect(quiet(read), "the model is off")

# races, telemetry, noise, sensor, tracker, predictor, selector and safety next to it: one launch more, whatever else runs
fresh()
fleet.sim_react()
fleet.sim_race([1, 3])                                                       # ltpl_fleet_sim_race keeps the model
assert named(run1) == 1
fleet.sim_react(None)
fleet.sim_telemetry()
fleet.sim_noise(seed=5, pos=0.1, obj_pos=0.3)
fleet.sim_sensor(range=100.0, fov_deg=120.0, occl=1.0, p_drop=0.1, seed=3)
fleet.sim_tracker()
fleet.sim_selector()
fleet.sim_safety()
busy = launches(run1)
fleet.sim_react()
fleet.sim_predictor(n_points=4)                                              # ltpl_fleet_sim_predictor keeps the model
busy_pred = launches(lambda: (fleet.sim_react(None), run1())[1])
fleet.sim_react()
assert launches(run1) == busy_pred + 1 and named(run1) == 1 and busy_pred == busy
fresh()                                                                      # sim_setup switches the model off
assert launches(run1) == plain and named(run1) == 0
expect(quiet(read), "the model is off")

# an allocation failing at each allocation of ltpl_fleet_sim_react: setting, replacing, and replacing with KEEP_STATE
for what, call, ok_after in (("setting", lambda: react(), 0), ("replacing", lambda: react(a_max=2.0), 1),
                             ("keeping the state", lambda: react(a_max=4.0, flags=1), 1)):
    def still(k, _):
        assert launches(run1) == plain + ok_after and named(run1) == ok_after, (what, k)      # the previous state: still off / still the old model
        assert (read()[0] == 0) == (ok_after == 1), (what, k)
    failures = common.alloc_sweep("ltpl_fleet_sim_react", call, 40, still)
    assert failures == 3, (what, failures)
    print("%s: allocation failure at each of the %d allocations of ltpl_fleet_sim_react: the fleet runs on" % (what, failures))
assert named(run1) == 1
assert lib.ltpl_fleet_sim_react(h, None) == 0 and named(run1) == 0

# the hook
M = 2
par = np.tile(np.array([1.0] + [GOOD[k] for k in NAMES]), (M, 1))
ego, dt, tick = np.zeros((M, 3)), np.full(M, 0.05), np.zeros(M, np.int32)
opp, rec, e_out, per_opp, ego_out = np.ones((200, 4)), np.zeros((M, RD)), np.zeros(200), np.zeros((200, 4)), np.zeros((M, 3))


def hook(n=M, off=(0, 1, 2), hole=None, params=par, dts=dt, ticks=tick, opps=opp):
    o = np.array(off, np.int32)
    args = [params.ctypes.data, ego.ctypes.data, dts.ctypes.data, ticks.ctypes.data, o.ctypes.data, opps.ctypes.data, rec.ctypes.data,
            e_out.ctypes.data, per_opp.ctypes.data, ego_out.ctypes.data]
    if hole is not None:
        args[hole] = None
    return lib.ltpl_fleet_sim_react_eval(h, n, *args), msg()


expect(quiet(lambda: hook(n=-1)), "n_cases")
for hole in range(10):
    expect(quiet(lambda: hook(hole=hole)), "missing")
expect(quiet(lambda: hook(off=(1, 2, 3))), "start at 0")
expect(quiet(lambda: hook(off=(0, 97, 98))), "0 .. 96 opponents")
expect(quiet(lambda: hook(off=(0, 3, 2))), "0 .. 96 opponents")
for c, bad, text in ((0, 2.0, "on must be 0 or 1"), (1, 0.0, "a_max must be positive"), (2, np.nan, "b_comf must be finite"), (3, -1.0, "b_max must be positive"),
                     (4, -0.5, "headway"), (5, np.inf, "gap0 must be finite"), (6, 0.0, "look must be positive"), (6, -np.inf, "look must be finite"),
                     (7, -0.5, "lat_gate"), (8, np.nan, "ego_len must be finite")):
    q = par.copy()
    q[1, c] = bad
    expect(quiet(lambda: hook(params=q)), "case 1: " + text)
for bad in (0.0, -0.05, np.nan, np.inf):
    expect(quiet(lambda: hook(dts=np.array([0.05, bad]))), "case 1: dt")
expect(quiet(lambda: hook(ticks=np.array([0, -1], np.int32))), "case 1: tick")
for bad in (np.nan, np.inf):
    q = opp.copy()
    q[1, 2] = bad
    expect(quiet(lambda: hook(opps=q)), "opponent 1: s, c, e and length must be finite")
assert quiet(lambda: lib.ltpl_fleet_sim_react_eval(h, 0, *([None] * 10))) == 0
assert launches(lambda: hook(off=(0, 96, 192))) == 1
q = par.copy()
q[:, 6] = np.inf
assert launches(lambda: hook(params=q)) == 1                                 # (look = +inf is an argument)
assert launches(lambda: (hook(off=(0, 0, 0), hole=5), hook(off=(0, 0, 0), hole=7), hook(off=(0, 0, 0), hole=8))) == 3       # (no opponents: opp, e_out, per_opp may be null)
print("launches per tick: %d without the model, %d with it (k_fleet_sim_react behind the events and the selector, in front of the step kernel); "
      "%d and %d with races, telemetry, noise, sensor, tracker, predictor, selector and safety" % (plain, with_react, busy_pred, busy_pred + 1))
common.finish("sim react args OK")
