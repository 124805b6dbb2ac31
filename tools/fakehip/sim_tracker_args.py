"""TEST TOOL: argument checks of ltpl_fleet_sim_tracker / ltpl_fleet_sim_tracker_read / ltpl_fleet_sim_tracker_eval (the object tracker of the
fleet simulation, csrc/fleet_track.hpp) without a device. The library's host code built against the stand-in runtime without sanitizers
(FAKEHIP_SAN=none tools/fakehip/build.sh); kernels do nothing, so no decision is looked at -- only the return codes, the messages and the
number of kernel launches:
  - every refused call (null fleet, no simulation, a missing array, a gate that is not finite and positive, w_pos / w_vel outside [0, 1),
    n_confirm outside 1 .. 255, n_coast outside 0 .. 255, a negative tick0; the read's record size and planner indices; the hook's counts,
    arrays and parameters) returns LTPL_ERR_INVALID_ARG with a message that names the argument, before any device allocation, and
    launches nothing;
  - a tick of ltpl_fleet_sim_run launches ONE kernel more while the tracker is set (k_fleet_sim_track), two more with the sensor set as
    well, and the same number as before when it is off, never set, or after ltpl_fleet_sim_setup; ltpl_fleet_sim_race keeps it;
  - a refused or failing call keeps the previous tracker (the tick still launches the extra kernel, the records stay readable);
  - an allocation failing at each allocation of ltpl_fleet_sim_tracker is LTPL_ERR_HIP, and the fleet runs on."""
import ctypes

import numpy as np

import sim_args_common as common
from sim_args_common import I32, P, expect, launches, msg, quiet, sim
from graphbasedlocaltrajectoryplanner_amd.fleet import SimTrackerIn

N = 4
lib, fleet, table = common.start(N)
lib.ltpl_fleet_sim_tracker.argtypes = [P, P]
lib.ltpl_fleet_sim_tracker_read.argtypes = [P, P, I32, I32, P, P, P]
lib.ltpl_fleet_sim_tracker_eval.argtypes = [P, I32] + [P] * 16
h = fleet.handle
GOOD = dict(gate=5.0, w_pos=0.5, w_vel=0.25, n_confirm=2, n_coast=3)


def tracker(tick0=0, missing=None, **par):
    keep = []
    ti = SimTrackerIn()
    for k, v in dict(GOOD, **par).items():
        keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32 if k.startswith("n_") else np.float64), (N,))))
        setattr(ti, k, None if k == missing else keep[-1].ctypes.data)
    ti.tick0 = tick0
    return lib.ltpl_fleet_sim_tracker(h, ctypes.byref(ti)), msg()


def fresh():
    common.fresh(common.moving_entries(N, static=[(1.0, 2.0, 0.0, 0.0, 4.0)]))


out = np.zeros((N, 12))
sel, tabs, cnt = np.arange(N, dtype=np.int32), np.zeros((N, 96, 10)), np.zeros(N, np.int32)


def read(size=12, n_sel=0, rec=True, hole=None, planners=sel):
    a = [planners.ctypes.data, tabs.ctypes.data, cnt.ctypes.data]
    if hole is not None:
        a[hole] = None
    return lib.ltpl_fleet_sim_tracker_read(h, out.ctypes.data if rec else None, size, n_sel, *a), msg()


# null fleet, no simulation
assert lib.ltpl_fleet_sim_tracker(None, None) == 1 and lib.ltpl_fleet_sim_tracker_read(None, out.ctypes.data, 12, 0, None, None, None) == 1
assert lib.ltpl_fleet_sim_tracker_eval(None, 0, *([None] * 16)) == 1
expect(quiet(lambda: tracker()), "ltpl_fleet_sim_setup first")
expect(quiet(lambda: (lib.ltpl_fleet_sim_tracker(h, None), msg())), "ltpl_fleet_sim_setup first")
expect(quiet(read), "ltpl_fleet_sim_setup first")

fresh()
plain = launches(lambda: fleet.sim_run(1, trace=False))
expect(quiet(read), "the tracker is off")
assert quiet(lambda: lib.ltpl_fleet_sim_tracker(h, None)) == 0              # switching off what is off: nothing to do


def refusals():
    for name in sim.TRACKER_PARAMS:
        expect(quiet(lambda: tracker(missing=name)), name + " missing")
    for bad in (np.nan, 0.0, -1.0, np.inf, -np.inf, [5.0, 5.0, 5.0, -1e-300]):
        expect(quiet(lambda: tracker(gate=bad)), "gate")
    for bad in (np.nan, -0.1, 1.0, 1.5, np.inf, [0.0, 0.0, 1.0, 0.0]):
        expect(quiet(lambda: tracker(w_pos=bad)), "w_pos")
        expect(quiet(lambda: tracker(w_vel=bad)), "w_vel")
    for bad in (0, -1, 256, [1, 1, 1, 1000]):
        expect(quiet(lambda: tracker(n_confirm=bad)), "n_confirm")
    for bad in (-1, 256, [0, 0, -5, 0]):
        expect(quiet(lambda: tracker(n_coast=bad)), "n_coast")
    expect(quiet(lambda: tracker(tick0=-1)), "tick0")


refusals()
# the edges that are arguments
assert tracker(gate=5e-324, w_pos=0.0, w_vel=float(np.nextafter(1.0, 0.0)), n_confirm=1, n_coast=0)[0] == 0
assert tracker(gate=1e300, n_confirm=255, n_coast=255, tick0=2 ** 31 - 1)[0] == 0
with_tracker = launches(lambda: fleet.sim_run(1, trace=False))
assert with_tracker == plain + 1, (with_tracker, plain)                      # k_fleet_sim_track, nothing else
assert read()[0] == 0 and read(n_sel=N)[0] == 0
expect(quiet(lambda: read(size=11)), "record size")
expect(quiet(lambda: read(rec=False)), "rec_out")
expect(quiet(lambda: read(n_sel=-1)), "n_sel")
for hole in range(3):
    expect(quiet(lambda: read(n_sel=2, hole=hole)), "missing")
expect(quiet(lambda: read(n_sel=2, planners=np.array([0, N], np.int32))), "out of range")
expect(quiet(lambda: read(n_sel=1, planners=np.array([-1], np.int32))), "out of range")
# a refused call keeps the previous tracker
refusals()
assert launches(lambda: fleet.sim_run(2, trace=False)) == 2 * with_tracker and read()[0] == 0
assert lib.ltpl_fleet_sim_tracker(h, None) == 0
assert launches(lambda: fleet.sim_run(1, trace=False)) == plain

# races, telemetry, noise and the sensor next to it: one launch more, whatever else runs; ltpl_fleet_sim_race keeps the tracker
fresh()
fleet.sim_tracker()
fleet.sim_race([1, 3])
assert read()[0] == 0
fleet.sim_telemetry()
fleet.sim_noise(seed=5, pos=0.1, obj_pos=0.3)
fleet.sim_tracker(None)
busy = launches(lambda: fleet.sim_run(1, trace=False))
fleet.sim_tracker(gate=4.0, n_confirm=3)
assert launches(lambda: fleet.sim_run(1, trace=False)) == busy + 1
fleet.sim_sensor(range=100.0, fov_deg=120.0, occl=1.0, p_drop=0.1, seed=3)
assert launches(lambda: fleet.sim_run(1, trace=False)) == busy + 2
fresh()                                                                      # sim_setup switches the tracker off
assert launches(lambda: fleet.sim_run(1, trace=False)) == plain
expect(quiet(read), "the tracker is off")

# an allocation failing at each allocation of ltpl_fleet_sim_tracker
assert tracker()[0] == 0
def runs_on(k, _):
    assert launches(lambda: fleet.sim_run(1, trace=False)) == with_tracker and read(n_sel=N)[0] == 0


failures = common.alloc_sweep("ltpl_fleet_sim_tracker", lambda: tracker(gate=9.0, tick0=7), 20, runs_on)
assert failures == 8, failures
print("allocation failure at each of the %d allocations of ltpl_fleet_sim_tracker: the fleet runs on" % failures)

# the hook
M = 2
par = np.tile(np.array([5.0, 0.5, 0.5, 2.0, 3.0]), (M, 1))
adv, tick, cs, nid = np.full(M, 0.25), np.zeros(M, np.uint32), np.tile(np.array([96, 96], np.int32), (M, 1)), np.zeros(M)
tracks, dets = np.zeros((200, 10)), np.zeros((200, 6))
o_tab, o_n, o_id, o_out, o_nout, o_asg, o_rec = np.zeros((M, 96, 10)), np.zeros(M, np.int32), np.zeros(M), np.zeros((M, 96, 6)), np.zeros(M, np.int32), \
    np.zeros(200, np.int32), np.zeros((M, 12))


def hook(n=M, toff=(0, 1, 2), doff=(0, 1, 2), hole=None, params=par, caps=cs):
    t, d = np.array(toff, np.int32), np.array(doff, np.int32)
    args = [params.ctypes.data, adv.ctypes.data, tick.ctypes.data, caps.ctypes.data, t.ctypes.data, tracks.ctypes.data, nid.ctypes.data, d.ctypes.data,
            dets.ctypes.data, o_tab.ctypes.data, o_n.ctypes.data, o_id.ctypes.data, o_out.ctypes.data, o_nout.ctypes.data, o_asg.ctypes.data,
            o_rec.ctypes.data]
    if hole is not None:
        args[hole] = None
    return lib.ltpl_fleet_sim_tracker_eval(h, n, *args), msg()


expect(quiet(lambda: hook(n=-1)), "n_cases")
for hole in range(16):
    expect(quiet(lambda: hook(hole=hole)), "missing")
expect(quiet(lambda: hook(toff=(1, 2, 3))), "start at 0")
expect(quiet(lambda: hook(doff=(1, 2, 3))), "start at 0")
expect(quiet(lambda: hook(toff=(0, 97, 98))), "capacity tracks")
expect(quiet(lambda: hook(toff=(0, 3, 2))), "capacity tracks")
expect(quiet(lambda: hook(doff=(0, 97, 98))), "slots detections")
expect(quiet(lambda: hook(caps=np.array([[97, 96], [96, 96]], np.int32))), "0 .. 96")
expect(quiet(lambda: hook(caps=np.array([[96, 96], [96, -1]], np.int32))), "0 .. 96")
expect(quiet(lambda: hook(toff=(0, 3, 6), caps=np.array([[2, 96], [96, 96]], np.int32))), "capacity tracks")
for c, bad in ((0, 0.0), (0, np.nan), (1, 1.0), (2, -0.5), (3, 0.0), (3, 256.0), (4, -1.0), (4, 256.0)):
    q = par.copy()
    q[1, c] = bad
    expect(quiet(lambda: hook(params=q)), "parameters out of range")
assert quiet(lambda: lib.ltpl_fleet_sim_tracker_eval(h, 0, *([None] * 16))) == 0
assert launches(lambda: hook(toff=(0, 96, 192), doff=(0, 96, 192))) == 1 and launches(lambda: hook(toff=(0, 0, 0), doff=(0, 0, 0), hole=5)) == 1
print("launches per tick: %d without the tracker, %d with it (%d and %d with races, telemetry and noise, %d with the sensor as well)" % (
    plain, with_tracker, busy, busy + 1, busy + 2))
common.finish("sim tracker args OK")
