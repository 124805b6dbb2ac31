"""TEST TOOL: argument checks of ltpl_fleet_sim_sensor / ltpl_fleet_sim_sensor_read / ltpl_fleet_sim_sensor_eval (the sensor model of the
fleet simulation, csrc/fleet_sensor.hpp) without a device. The library's host code built against the stand-in runtime without sanitizers
(FAKEHIP_SAN=none tools/fakehip/build.sh); kernels do nothing, so no decision is looked at -- only the return codes, the messages and the
number of kernel launches:
  - every refused call (null fleet, no simulation, a missing array, a NaN or negative range, r_near outside [0, range], fov_cos outside
    [-1, 1], a negative or infinite occl, p_drop outside [0, 1), a negative tick0; the hook's counts and arrays) returns
    LTPL_ERR_INVALID_ARG with a message that names the argument, before any device allocation, and launches nothing;
  - a tick of ltpl_fleet_sim_run launches ONE kernel more while the sensor is set (k_fleet_sim_sense) and the same number as before when
    it is off, never set, or after ltpl_fleet_sim_setup;
  - a refused or failing call keeps the previous sensor (the tick still launches the extra kernel, the records stay readable);
  - an allocation failing at each allocation of ltpl_fleet_sim_sensor is LTPL_ERR_HIP, and the fleet runs on."""
import ctypes

import numpy as np

import sim_args_common as common
from sim_args_common import expect, launches, msg, quiet
from graphbasedlocaltrajectoryplanner_amd.fleet import SimSensorIn

N = 4
lib, fleet, table = common.start(N)
lib.ltpl_fleet_sim_sensor.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.ltpl_fleet_sim_sensor_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
lib.ltpl_fleet_sim_sensor_eval.argtypes = [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 8
h = fleet.handle
GOOD = dict(range=120.0, r_near=5.0, fov_cos=0.5, occl=1.0, p_drop=0.1)


def sensor(tick0=0, missing=None, **par):
    keep = []
    si = SimSensorIn()
    for k, v in dict(GOOD, **par).items():
        keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (N,))))
        setattr(si, k, None if k == missing else keep[-1].ctypes.data)
    keep.append(np.arange(N, dtype=np.uint64))
    si.seed, si.tick0 = None if missing == "seed" else keep[-1].ctypes.data, tick0
    return lib.ltpl_fleet_sim_sensor(h, ctypes.byref(si)), msg()


def fresh():
    common.fresh(common.moving_entries(N, static=[(1.0, 2.0, 0.0, 0.0, 4.0)]))


out = np.zeros((N, 10))
# null fleet, no simulation
assert lib.ltpl_fleet_sim_sensor(None, None) == 1 and lib.ltpl_fleet_sim_sensor_read(None, out.ctypes.data, 10) == 1
assert lib.ltpl_fleet_sim_sensor_eval(None, 0, None, None, None, None, None, None, None, None) == 1
expect(quiet(lambda: sensor()), "ltpl_fleet_sim_setup first")
expect(quiet(lambda: (lib.ltpl_fleet_sim_sensor(h, None), msg())), "ltpl_fleet_sim_setup first")
expect(quiet(lambda: (lib.ltpl_fleet_sim_sensor_read(h, out.ctypes.data, 10), msg())), "ltpl_fleet_sim_setup first")

fresh()
plain = launches(lambda: fleet.sim_run(1, trace=False))
expect(quiet(lambda: (lib.ltpl_fleet_sim_sensor_read(h, out.ctypes.data, 10), msg())), "the sensor is off")
assert quiet(lambda: lib.ltpl_fleet_sim_sensor(h, None)) == 0               # switching off what is off: nothing to do


def refusals():
    for name in ("range", "r_near", "fov_cos", "occl", "p_drop", "seed"):
        expect(quiet(lambda: sensor(missing=name)), name + " missing")
    for bad in (np.nan, -1.0, -np.inf, [120.0, 120.0, 120.0, -1e-300]):
        expect(quiet(lambda: sensor(range=bad, r_near=0.0)), "range")
    for bad in (np.nan, -0.5, 120.5, np.inf, [0.0, 0.0, 121.0, 0.0]):
        expect(quiet(lambda: sensor(r_near=bad)), "r_near")
    for bad in (np.nan, -1.0000001, 1.0000001, np.inf, -np.inf):
        expect(quiet(lambda: sensor(fov_cos=bad)), "fov_cos")
    for bad in (np.nan, -0.1, np.inf, -np.inf):
        expect(quiet(lambda: sensor(occl=bad)), "occl")
    for bad in (np.nan, -0.1, 1.0, 1.5, np.inf):
        expect(quiet(lambda: sensor(p_drop=bad)), "p_drop")
    expect(quiet(lambda: sensor(tick0=-1)), "tick0")


refusals()
# the edges that are arguments: range +inf and 0, r_near = range, fov_cos -1 and 1, occl 0, p_drop 0 and the largest value below 1
assert sensor(range=np.inf, r_near=1e300, fov_cos=-1.0, occl=0.0, p_drop=0.0)[0] == 0
assert sensor(range=0.0, r_near=-0.0, fov_cos=1.0, p_drop=float(np.nextafter(1.0, 0.0)), tick0=2 ** 31 - 1)[0] == 0
assert sensor(r_near=120.0)[0] == 0
with_sensor = launches(lambda: fleet.sim_run(1, trace=False))
assert with_sensor == plain + 1, (with_sensor, plain)                        # k_fleet_sim_sense, nothing else
assert lib.ltpl_fleet_sim_sensor_read(h, out.ctypes.data, 10) == 0
expect(quiet(lambda: (lib.ltpl_fleet_sim_sensor_read(h, out.ctypes.data, 9), msg())), "record size")
assert lib.ltpl_fleet_sim_sensor_read(h, None, 10) == 1
# a refused call keeps the previous sensor
refusals()
assert launches(lambda: fleet.sim_run(2, trace=False)) == 2 * with_sensor and lib.ltpl_fleet_sim_sensor_read(h, out.ctypes.data, 10) == 0
assert lib.ltpl_fleet_sim_sensor(h, None) == 0
assert launches(lambda: fleet.sim_run(1, trace=False)) == plain

# races, telemetry and noise next to it: one launch more, whatever else runs
fresh()
fleet.sim_race([1, 3])
fleet.sim_telemetry()
fleet.sim_noise(seed=5, pos=0.1, obj_pos=0.3)
busy = launches(lambda: fleet.sim_run(1, trace=False))
fleet.sim_sensor(range=100.0, fov_deg=120.0, occl=1.0, p_drop=0.1, seed=3)
assert launches(lambda: fleet.sim_run(1, trace=False)) == busy + 1
fresh()                                                                      # sim_setup switches the sensor off
assert launches(lambda: fleet.sim_run(1, trace=False)) == plain
expect(quiet(lambda: (lib.ltpl_fleet_sim_sensor_read(h, out.ctypes.data, 10), msg())), "the sensor is off")

# an allocation failing at each allocation of ltpl_fleet_sim_sensor
assert sensor()[0] == 0
def runs_on(k, _):
    assert launches(lambda: fleet.sim_run(1, trace=False)) == with_sensor and lib.ltpl_fleet_sim_sensor_read(h, out.ctypes.data, 10) == 0


failures = common.alloc_sweep("ltpl_fleet_sim_sensor", lambda: sensor(range=50.0, tick0=7), 10, runs_on)
assert failures == 3, failures
print("allocation failure at each of the %d allocations of ltpl_fleet_sim_sensor: the fleet runs on" % failures)

# the hook
pf, par = np.zeros((2, 4)), np.zeros((2, 5))
seed, tick = np.zeros(2, np.uint64), np.zeros(2, np.uint32)
objs, cause, u = np.zeros((200, 3)), np.zeros(200, np.int32), np.zeros(200)


def hook(n=2, off=(0, 1, 2), hole=None):
    o = np.array(off, np.int32)
    args = [pf.ctypes.data, par.ctypes.data, seed.ctypes.data, tick.ctypes.data, o.ctypes.data, objs.ctypes.data, cause.ctypes.data, u.ctypes.data]
    if hole is not None:
        args[hole] = None
    return lib.ltpl_fleet_sim_sensor_eval(h, n, *args), msg()


expect(quiet(lambda: hook(n=-1)), "n_cases")
for hole in range(8):
    expect(quiet(lambda: hook(hole=hole)), "missing")
expect(quiet(lambda: hook(off=(1, 2, 3))), "start at 0")
expect(quiet(lambda: hook(off=(0, 97, 98))), "0 .. 96 objects")
expect(quiet(lambda: hook(off=(0, 3, 2))), "0 .. 96 objects")
assert quiet(lambda: lib.ltpl_fleet_sim_sensor_eval(h, 0, None, None, None, None, None, None, None, None)) == 0
assert launches(lambda: hook(off=(0, 96, 192))) == 1 and launches(lambda: hook(off=(0, 0, 0), hole=5)) == 1
print("launches per tick: %d without the sensor, %d with it (%d and %d with races, telemetry and noise)" % (plain, with_sensor, busy, busy + 1))
common.finish("sim sensor args OK")
