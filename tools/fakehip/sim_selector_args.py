"""TEST TOOL: argument checks of ltpl_fleet_sim_selector / ltpl_fleet_sim_selector_read / ltpl_fleet_sim_selector_eval (the behaviour selector
of the fleet simulation, csrc/fleet_select.hpp) without a device. The library's host code built against the stand-in runtime without
sanitizers (FAKEHIP_SAN=none tools/fakehip/build.sh); kernels do nothing, so no decision is looked at -- only the return codes, the
messages and the kernel launches (by number and, through fakehip_launches_of, by name):
  - every refused call (null fleet, no simulation, a missing array, a horizon that is not positive, a negative r_ego / w_clear / w_switch,
    a NaN anywhere; the read's record size; the hook's counts, arrays, lists, rows and parameters) returns LTPL_ERR_INVALID_ARG with a
    message that names the argument, before any device allocation, and launches nothing;
  - a refused or failing call keeps the previous selector (the tick still launches k_fleet_sim_select, the records stay readable); an
    allocation failing at each allocation of the call is LTPL_ERR_HIP, and the fleet runs on;
  - per tick a fleet with the selector set launches k_fleet_sim_select once, one kernel more than before; a fleet that had one and cleared
    it, and one after ltpl_fleet_sim_setup, launch what a fleet that never had one launches, k_fleet_sim_select never."""
import ctypes

import numpy as np

import sim_args_common as common
from sim_args_common import I32, INVALID, P, expect, launches, msg, quiet, run1, sim
from graphbasedlocaltrajectoryplanner_amd.fleet import SimSelectorIn

N = 4
lib, fleet, table = common.start(N)
N_PREF = 2 * N
lib.ltpl_fleet_sim_selector.argtypes = [P, P]
lib.ltpl_fleet_sim_selector_read.argtypes = [P, P, I32, P, I32]
lib.ltpl_fleet_sim_selector_eval.argtypes = [P, I32] + [P] * 10
h = fleet.handle
GOOD = dict(sim.SELECTOR_DEFAULTS)


def selector(missing=None, on=1, **par):
    keep = [np.ascontiguousarray(np.broadcast_to(np.asarray(on, np.int32), (N,)))]
    si = SimSelectorIn()
    si.on = None if missing == "on" else keep[0].ctypes.data
    for k in sim.SELECTOR_PARAMS:
        keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(dict(GOOD, **par)[k], np.float64), (N,))))
        setattr(si, k, None if k == missing else keep[-1].ctypes.data)
    return lib.ltpl_fleet_sim_selector(h, ctypes.byref(si)), msg()


SELECT = b"_Z18k_fleet_sim_select"       # the whole mangled name up to the arguments: 18 = len("k_fleet_sim_select"), so the hook
                                        # k_fleet_sim_selector_eval (_Z25...) does not match


def named(fn):
    return common.named(fn, SELECT)


def fresh():
    common.fresh(common.moving_entries(N))


out, order = np.zeros((N, sim.SELECTOR_DOUBLES)), np.zeros(N_PREF, np.int32)


def read(size=sim.SELECTOR_DOUBLES, rec=True, n_ordered=N_PREF):
    return lib.ltpl_fleet_sim_selector_read(h, out.ctypes.data if rec else None, size, order.ctypes.data, n_ordered), msg()


# null fleet, no simulation
assert lib.ltpl_fleet_sim_selector(None, None) == INVALID and lib.ltpl_fleet_sim_selector_read(None, out.ctypes.data, 12, None, 0) == INVALID
assert lib.ltpl_fleet_sim_selector_eval(None, 0, *([None] * 10)) == INVALID
expect(quiet(lambda: selector()), "ltpl_fleet_sim_setup first")
expect(quiet(lambda: (lib.ltpl_fleet_sim_selector(h, None), msg())), "ltpl_fleet_sim_setup first")
expect(quiet(read), "ltpl_fleet_sim_setup first")

fresh()
plain = launches(run1)
assert named(run1) == 0
expect(quiet(read), "the selector is off")
assert quiet(lambda: lib.ltpl_fleet_sim_selector(h, None)) == 0             # switching off what is off: nothing to do, nothing allocated


def refusals():
    for name in ("on",) + sim.SELECTOR_PARAMS:
        expect(quiet(lambda: selector(missing=name)), name + " missing")
    for bad in (0.0, -1.0, -np.inf, [1.0, 1.0, 1.0, -1e-300]):
        expect(quiet(lambda: selector(horizon=bad)), "horizon")
    for name in ("r_ego", "w_clear", "w_switch"):
        for bad in (-1.0, -np.inf, [0.0, 0.0, 0.0, -5e-324]):
            expect(quiet(lambda: selector(**{name: bad})), name)
    for name in sim.SELECTOR_PARAMS:
        expect(quiet(lambda: selector(**{name: [GOOD[name], np.nan, GOOD[name], GOOD[name]]})), "planner 1: a parameter is NaN")


refusals()
# the edges that are arguments
assert selector(horizon=5e-324, r_ego=0.0, c_hard=-np.inf, c_soft=-np.inf, w_clear=0.0, w_switch=0.0)[0] == 0
assert selector(on=[1, 0, 1, 0], horizon=np.inf, r_ego=np.inf, c_hard=np.inf, c_soft=np.inf, w_clear=np.inf, w_switch=np.inf)[0] == 0
with_sel = launches(run1)
assert with_sel == plain + 1, (with_sel, plain)
assert named(run1) == 1
assert read()[0] == 0
expect(quiet(lambda: read(size=11)), "record size")
expect(quiet(lambda: read(rec=False)), "out missing")
for bad in (N_PREF - 1, N_PREF + 1, 0):
    expect(quiet(lambda: read(n_ordered=bad)), "n_ordered")
assert lib.ltpl_fleet_sim_selector_read(h, out.ctypes.data, sim.SELECTOR_DOUBLES, None, 0) == 0       # (without the lists)
# a refused call keeps the previous selector
refusals()
assert named(lambda: fleet.sim_run(3, trace=False)) == 3 and read()[0] == 0
assert lib.ltpl_fleet_sim_selector(h, None) == 0
assert launches(run1) == plain and named(run1) == 0                          # set, then cleared: what a fleet that never had one launches
expect(quiet(read), "the selector is off")

# races, telemetry, noise, sensor, tracker and predictor next to it: one launch more, whatever else runs
fresh()
fleet.sim_race([1, 3])
fleet.sim_telemetry()
fleet.sim_noise(seed=5, pos=0.1, obj_pos=0.3)
fleet.sim_sensor(range=100.0, fov_deg=120.0, occl=1.0, p_drop=0.1, seed=3)
fleet.sim_tracker()
fleet.sim_predictor(n_points=4)
busy = launches(run1)
fleet.sim_selector()
assert launches(run1) == busy + 1 and named(run1) == 1
fresh()                                                                      # sim_setup switches the selector off
assert launches(run1) == plain and named(run1) == 0
expect(quiet(read), "the selector is off")

# an allocation failing at each allocation of ltpl_fleet_sim_selector: setting and replacing
for what, call, ok_after in (("setting", lambda: selector(), 0), ("replacing", lambda: selector(horizon=9.0), 1)):
    def still(k, _):
        assert launches(run1) == plain + ok_after and named(run1) == ok_after, (what, k)      # the previous state: still off / still the old selector
        assert (read()[0] == 0) == (ok_after == 1), (what, k)
    failures = common.alloc_sweep("ltpl_fleet_sim_selector", call, 40, still)
    assert failures == 4, (what, failures)
    print("%s: allocation failure at each of the %d allocations of ltpl_fleet_sim_selector: the fleet runs on" % (what, failures))
assert named(run1) == 1
assert lib.ltpl_fleet_sim_selector(h, None) == 0 and named(run1) == 0

# the hook
M = 2
par = np.tile(np.array([GOOD[k] for k in sim.SELECTOR_PARAMS]), (M, 1))
lists = np.array([[2, 0, 0, 0, 2, 0, 0, 0], [3, 1, 1, 4, 1, 0, 0, 0]], np.int32)
n_rows = np.array([[5, -1, 5, -1], [256, 0, -1, 2]], np.int32)
rows, objs = np.zeros((M, 4, 4, 256)), np.zeros((200, 5))
ordered, act_d, act_i, rec = np.zeros((M, 5), np.int32), np.zeros((M, 4, 3)), np.zeros((M, 4, 2), np.int32), np.zeros((M, sim.SELECTOR_DOUBLES))


def hook(n=M, off=(0, 1, 2), hole=None, params=par, li=lists, nr=n_rows):
    o = np.array(off, np.int32)
    args = [params.ctypes.data, li.ctypes.data, nr.ctypes.data, rows.ctypes.data, o.ctypes.data, objs.ctypes.data, ordered.ctypes.data,
            act_d.ctypes.data, act_i.ctypes.data, rec.ctypes.data]
    if hole is not None:
        args[hole] = None
    return lib.ltpl_fleet_sim_selector_eval(h, n, *args), msg()


expect(quiet(lambda: hook(n=-1)), "n_cases")
for hole in range(10):
    expect(quiet(lambda: hook(hole=hole)), "missing")
expect(quiet(lambda: hook(off=(1, 2, 3))), "start at 0")
expect(quiet(lambda: hook(off=(0, 97, 98))), "0 .. 96 objects")
expect(quiet(lambda: hook(off=(0, 3, 2))), "0 .. 96 objects")
for c, bad, text in ((0, 0.0, "horizon"), (0, np.nan, "a parameter is NaN"), (1, -1.0, "r_ego"), (2, np.nan, "a parameter is NaN"), (4, -0.5, "w_clear"), (5, -0.5, "w_switch")):
    q = par.copy()
    q[1, c] = bad
    expect(quiet(lambda: hook(params=q)), "case 1: " + text)
for col, bad, text in ((0, 0, "a preference list needs 1 .. 5 entries"), (0, 6, "a preference list needs 1 .. 5 entries"), (3, 5, "unknown action"), (4, -1, "unknown action")):
    q = lists.copy()
    q[1, col] = bad
    expect(quiet(lambda: hook(li=q)), "case 1: " + text)
for bad in (-2, 257):
    q = n_rows.copy()
    q[1, 2] = bad
    expect(quiet(lambda: hook(nr=q)), "case 1: rows")
assert quiet(lambda: lib.ltpl_fleet_sim_selector_eval(h, 0, *([None] * 10))) == 0
assert launches(lambda: hook(off=(0, 96, 192))) == 1 and launches(lambda: hook(off=(0, 0, 0), hole=5)) == 1
print("launches per tick: %d without the selector, %d with it (k_fleet_sim_select at the head of the tick); %d and %d with races, telemetry, "
      "noise, sensor, tracker and predictor" % (plain, with_sel, busy, busy + 1))
common.finish("sim selector args OK")
