"""TEST TOOL: argument checks of ltpl_fleet_sim_safety / ltpl_fleet_sim_safety_read / ltpl_fleet_sim_safety_eval (the safety monitor of the
fleet simulation, csrc/fleet_safety.hpp) without a device. The library's host code built against the stand-in runtime without sanitizers
(FAKEHIP_SAN=none tools/fakehip/build.sh); kernels do nothing, so no measure is looked at -- only the return codes, the messages and the
kernel launches (by number and, through fakehip_launches_of, by name):
  - every refused call (null fleet, no simulation, a missing array, an `on` that is neither 0 nor 1, a ttc_thr that is not positive, a
    negative r_ego / drac_thr / thw_thr / margin, a NaN or an infinity anywhere, a negative tick0, an unknown flag; the read's record and
    incident sizes; the hook's counts, arrays, offsets, dt, tick and parameters) returns LTPL_ERR_INVALID_ARG with a message that names the
    argument, before any device allocation, and launches nothing;
  - a refused or failing call keeps the previous monitor (the tick still launches k_fleet_sim_safety, the records stay readable); an
    allocation failing at each allocation of the call is LTPL_ERR_HIP, and the fleet runs on;
  - per tick a fleet with the monitor set launches k_fleet_sim_safety once, one kernel more than before whatever else runs; a fleet that
    had one and cleared it, and one after ltpl_fleet_sim_setup, launch what a fleet that never had one launches, k_fleet_sim_safety never;
  - snapshot and branch launch k_fleet_sim_branch_safety only while the monitor is set."""
import ctypes

import numpy as np

import sim_args_common as common
from sim_args_common import I32, INVALID, P, expect, launches, msg, quiet, run1, sim
from graphbasedlocaltrajectoryplanner_amd.fleet import SimSafetyIn

N = 4
lib, fleet, table = common.start(N)
lib.ltpl_fleet_sim_safety.argtypes = [P, P]
lib.ltpl_fleet_sim_safety_read.argtypes = [P, P, I32, P, I32]
lib.ltpl_fleet_sim_safety_eval.argtypes = [P, I32] + [P] * 10
h = fleet.handle
RD, ID = sim.SAFETY_DOUBLES, sim.INCIDENT_DOUBLES
GOOD = dict(sim.SAFETY_DEFAULTS)


def safety(missing=None, on=1, tick0=0, flags=0, **par):
    keep = [np.ascontiguousarray(np.broadcast_to(np.asarray(on, np.int32), (N,)))]
    si = SimSafetyIn()
    si.on = None if missing == "on" else keep[0].ctypes.data
    for k in sim.SAFETY_PARAMS:
        keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(dict(GOOD, **par)[k], np.float64), (N,))))
        setattr(si, k, None if k == missing else keep[-1].ctypes.data)
    si.tick0, si.flags = tick0, flags
    return lib.ltpl_fleet_sim_safety(h, ctypes.byref(si)), msg()


SAFETY = b"_Z18k_fleet_sim_safety"       # the whole mangled name up to the arguments: 18 = len("k_fleet_sim_safety"), so the hook
                                        # k_fleet_sim_safety_eval (_Z23...) does not match
BRANCH = b"_Z25k_fleet_sim_branch_safety"


def named(fn, name=SAFETY):
    return common.named(fn, name)


def fresh():
    common.fresh(common.moving_entries(N))


out, inc = np.zeros((N, RD)), np.zeros((N, sim.SAFETY_INCIDENTS, ID))


def read(size=RD, rec=True, ring=True, isize=ID):
    return lib.ltpl_fleet_sim_safety_read(h, out.ctypes.data if rec else None, size, inc.ctypes.data if ring else None, isize), msg()


# null fleet, no simulation
assert lib.ltpl_fleet_sim_safety(None, None) == INVALID and lib.ltpl_fleet_sim_safety_read(None, out.ctypes.data, RD, None, ID) == INVALID
assert lib.ltpl_fleet_sim_safety_eval(None, 0, *([None] * 10)) == INVALID
expect(quiet(lambda: safety()), "ltpl_fleet_sim_setup first")
expect(quiet(lambda: (lib.ltpl_fleet_sim_safety(h, None), msg())), "ltpl_fleet_sim_setup first")
expect(quiet(read), "ltpl_fleet_sim_setup first")

fresh()
plain = launches(run1)
assert named(run1) == 0
expect(quiet(read), "the monitor is off")
assert quiet(lambda: lib.ltpl_fleet_sim_safety(h, None)) == 0               # clearing what is off: nothing to do, nothing allocated


def refusals():
    for name in ("on",) + sim.SAFETY_PARAMS:
        expect(quiet(lambda: safety(missing=name)), name + " missing")
    for bad in (0.0, -1.0, [1.0, 1.0, 1.0, -1e-300]):
        expect(quiet(lambda: safety(ttc_thr=bad)), "ttc_thr must be positive")
    for name in ("r_ego", "drac_thr", "thw_thr", "margin"):
        for bad in (-1.0, [0.0, 0.0, 0.0, -5e-324]):
            expect(quiet(lambda: safety(**{name: bad})), name + " must not be negative")
    for name in sim.SAFETY_PARAMS:
        for bad in (np.nan, np.inf, -np.inf):
            expect(quiet(lambda: safety(**{name: [GOOD[name], bad, GOOD[name], GOOD[name]]})), "planner 1: " + name + " must be finite")
    for bad in (2, -1, [1, 0, 1, 7]):
        expect(quiet(lambda: safety(on=bad)), "on must be 0 or 1")
    expect(quiet(lambda: safety(tick0=-1)), "tick0")
    expect(quiet(lambda: safety(flags=2)), "unknown flag")


refusals()
# the edges that are arguments
assert safety(r_ego=0.0, ttc_thr=5e-324, drac_thr=0.0, thw_thr=0.0, margin=0.0)[0] == 0
assert safety(on=[1, 0, 1, 0], tick0=2 ** 31 - 1, flags=1)[0] == 0          # (KEEP_STATE on a set monitor)
with_saf = launches(run1)
assert with_saf == plain + 1, (with_saf, plain)
assert named(run1) == 1
assert read()[0] == 0
expect(quiet(lambda: read(size=RD - 1)), "record size")
expect(quiet(lambda: read(rec=False)), "out missing")
expect(quiet(lambda: read(isize=ID + 1)), "incident size")
assert read(ring=False, isize=0)[0] == 0                                     # (without the rings)
# a refused call keeps the previous monitor
refusals()
assert named(lambda: fleet.sim_run(3, trace=False)) == 3 and read()[0] == 0
# snapshot and branch copy record and ring with a kernel of their own, only while a monitor is set
assert named(lambda: fleet.sim_snapshot(0), BRANCH) == 1 and named(lambda: fleet.sim_restore(0), BRANCH) == 1
assert named(lambda: fleet.sim_branch(0, [1, 2]), BRANCH) == 1
assert lib.ltpl_fleet_sim_safety(h, None) == 0
assert launches(run1) == plain and named(run1) == 0                          # set, then cleared: what a fleet that never had one launches
expect(quiet(read), "the monitor is off")
assert named(lambda: fleet.sim_snapshot(1), BRANCH) == 0 and named(lambda: fleet.sim_restore(0), BRANCH) == 0
assert named(lambda: fleet.sim_branch(0, [1, 2]), BRANCH) == 0

# races, telemetry, noise, sensor, tracker, predictor and selector next to it: one launch more, whatever else runs
fresh()
fleet.sim_race([1, 3])
fleet.sim_telemetry()
fleet.sim_noise(seed=5, pos=0.1, obj_pos=0.3)
fleet.sim_sensor(range=100.0, fov_deg=120.0, occl=1.0, p_drop=0.1, seed=3)
fleet.sim_tracker()
fleet.sim_predictor(n_points=4)
fleet.sim_selector()
busy = launches(run1)
fleet.sim_safety()
assert launches(run1) == busy + 1 and named(run1) == 1
fresh()                                                                      # sim_setup switches the monitor off
assert launches(run1) == plain and named(run1) == 0
expect(quiet(read), "the monitor is off")

# an allocation failing at each allocation of ltpl_fleet_sim_safety: setting, replacing, and replacing with KEEP_STATE
for what, call, ok_after in (("setting", lambda: safety(), 0), ("replacing", lambda: safety(ttc_thr=9.0), 1),
                             ("keeping the state", lambda: safety(ttc_thr=2.0, flags=1), 1)):
    def still(k, _):
        assert launches(run1) == plain + ok_after and named(run1) == ok_after, (what, k)      # the previous state: still off / still the old monitor
        assert (read()[0] == 0) == (ok_after == 1), (what, k)
    failures = common.alloc_sweep("ltpl_fleet_sim_safety", call, 40, still)
    assert failures == 4, (what, failures)
    print("%s: allocation failure at each of the %d allocations of ltpl_fleet_sim_safety: the fleet runs on" % (what, failures))
assert named(run1) == 1
assert lib.ltpl_fleet_sim_safety(h, None) == 0 and named(run1) == 0

# the hook
M = 2
par = np.tile(np.array([GOOD[k] for k in sim.SAFETY_PARAMS]), (M, 1))
pose, dt, tick = np.zeros((M, 2)), np.full(M, 0.05), np.zeros(M, np.int32)
objs, rec, ring, per_obj, per_tick = np.zeros((200, 5)), np.zeros((M, RD)), np.zeros((M, 8, ID)), np.zeros((200, 6)), np.zeros((M, 8))


def hook(n=M, off=(0, 1, 2), hole=None, params=par, dts=dt, ticks=tick):
    o = np.array(off, np.int32)
    args = [pose.ctypes.data, dts.ctypes.data, ticks.ctypes.data, params.ctypes.data, o.ctypes.data, objs.ctypes.data, rec.ctypes.data,
            ring.ctypes.data, per_obj.ctypes.data, per_tick.ctypes.data]
    if hole is not None:
        args[hole] = None
    return lib.ltpl_fleet_sim_safety_eval(h, n, *args), msg()


expect(quiet(lambda: hook(n=-1)), "n_cases")
for hole in range(10):
    expect(quiet(lambda: hook(hole=hole)), "missing")
expect(quiet(lambda: hook(off=(1, 2, 3))), "start at 0")
expect(quiet(lambda: hook(off=(0, 97, 98))), "0 .. 96 objects")
expect(quiet(lambda: hook(off=(0, 3, 2))), "0 .. 96 objects")
for c, bad, text in ((0, -1.0, "r_ego must not be negative"), (1, 0.0, "ttc_thr must be positive"), (1, np.nan, "ttc_thr must be finite"),
                     (2, -0.5, "drac_thr"), (3, np.inf, "thw_thr must be finite"), (4, -0.5, "margin")):
    q = par.copy()
    q[1, c] = bad
    expect(quiet(lambda: hook(params=q)), "case 1: " + text)
for bad in (0.0, -0.05, np.nan, np.inf):
    expect(quiet(lambda: hook(dts=np.array([0.05, bad]))), "case 1: dt")
expect(quiet(lambda: hook(ticks=np.array([0, -1], np.int32))), "case 1: tick")
assert quiet(lambda: lib.ltpl_fleet_sim_safety_eval(h, 0, *([None] * 10))) == 0
assert launches(lambda: hook(off=(0, 96, 192))) == 1
assert launches(lambda: (hook(off=(0, 0, 0), hole=5), hook(off=(0, 0, 0), hole=8))) == 2       # (no objects: objs and per_obj may be null)
print("launches per tick: %d without the monitor, %d with it (k_fleet_sim_safety behind telemetry, in front of the sensor); %d and %d with "
      "races, telemetry, noise, sensor, tracker, predictor and selector" % (plain, with_saf, busy, busy + 1))
common.finish("sim safety args OK")
