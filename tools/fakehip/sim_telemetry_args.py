"""TEST TOOL: argument checks of ltpl_fleet_sim_telemetry / ltpl_fleet_sim_telemetry_read (the race telemetry of the fleet simulation)
without a device. The library's host code built against the stand-in runtime without sanitizers (FAKEHIP_SAN=none
tools/fakehip/build.sh); kernels do nothing, so the records read back are the "before the first tick" values -- only those, the return
codes, the messages and the number of kernel launches per simulated tick are looked at:
  - every error case (no simulation, NaN / infinite / negative radius, non-finite grid_s, wrong record size, a read while off) returns
    LTPL_ERR_INVALID_ARG before any device allocation, with the previous telemetry intact;
  - set, reset and off: telemetry adds one launch per tick (k_fleet_sim_tele), two with a race of more than one planner
    (k_fleet_sim_rank); off, and after ltpl_fleet_sim_setup, a tick launches what it launched before;
  - an allocation failing at any point of ltpl_fleet_sim_telemetry leaves the previous telemetry in place."""
import ctypes

import numpy as np

import sim_args_common as common
from sim_args_common import _capi, expect, launches_per_tick, msg, no_allocation, sim
from graphbasedlocaltrajectoryplanner_amd.fleet import SimTeleIn

N = 4
lib, fleet, table = common.start(N)
D = sim.TELEMETRY_DOUBLES
lib.ltpl_fleet_sim_telemetry.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.ltpl_fleet_sim_telemetry_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
h = fleet.handle


def call(radius=2.5, grid_s=None):
    rad = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float64), (N,)))
    ti = SimTeleIn()
    ti.radius = rad.ctypes.data
    if grid_s is not None:
        gs = np.ascontiguousarray(np.broadcast_to(np.asarray(grid_s, np.float64), (N,)))
        ti.grid_s = gs.ctypes.data
    return lib.ltpl_fleet_sim_telemetry(h, ctypes.byref(ti)), msg()


def read(doubles=D):
    out = np.full((N, D), 7.0)
    L = ctypes.c_double(0.0)
    rc = lib.ltpl_fleet_sim_telemetry_read(h, out.ctypes.data, doubles, ctypes.byref(L))
    return rc, out, L.value, msg()


BEFORE = np.zeros(D)
BEFORE[[1, 4, 5, 6, 21]] = np.nan
BEFORE[8], BEFORE[14], BEFORE[15], BEFORE[16] = -np.inf, np.inf, -1.0, -1.0


def intact():
    """The telemetry set before a refused call is still there: a read succeeds and returns the untouched records."""
    rc, out, L, _ = read()
    assert rc == 0 and abs(L - 2382.2979975) < 1e-6 and all(np.array_equal(row, BEFORE, equal_nan=True) for row in out), (rc, L, out)


def fresh(races=None):
    common.fresh()
    if races:
        fleet.sim_race(races)


# no simulation set up
assert lib.ltpl_fleet_sim_telemetry(None, None) == 1 and lib.ltpl_fleet_sim_telemetry_read(None, None, D, None) == 1
expect(no_allocation(call), 1, "ltpl_fleet_sim_setup first")
expect(no_allocation(read), 1, "ltpl_fleet_sim_setup first")
assert no_allocation(lambda: lib.ltpl_fleet_sim_telemetry(h, None)) == 1

fresh()
plain = launches_per_tick()
expect(no_allocation(read), 1, "telemetry is off")                              # a read while telemetry is off
assert lib.ltpl_fleet_sim_telemetry(h, None) == 0                               # off while off: nothing to do
assert call(grid_s=[5.0, 2380.0, 1.0, 0.0])[0] == 0
intact()
for kw, text in ((dict(radius=np.nan), "finite and not negative"), (dict(radius=-0.5), "finite and not negative"),
                 (dict(radius=np.inf), "finite and not negative"), (dict(radius=[2.5, 2.5, 2.5, -1e-300]), "finite and not negative"),
                 (dict(grid_s=np.nan), "grid_s must be finite"), (dict(grid_s=[0.0, 1.0, -np.inf, 2.0]), "grid_s must be finite")):
    expect(no_allocation(lambda: call(**kw)), 1, text)                          # LTPL_ERR_INVALID_ARG
    intact()
ti = SimTeleIn()
assert no_allocation(lambda: lib.ltpl_fleet_sim_telemetry(h, ctypes.byref(ti))) == 1 and b"radius missing" in lib.ltpl_fleet_last_error(h)
intact()
expect(no_allocation(lambda: read(D - 1)), 1, "record size mismatch")
expect(no_allocation(lambda: read(D + 30)), 1, "record size mismatch")
assert lib.ltpl_fleet_sim_telemetry_read(h, None, D, None) == 1
intact()
assert call(radius=0.0)[0] == 0                                                 # a radius of zero is allowed

# set, reset, off: launches per tick
assert launches_per_tick() == plain + 1                                         # + k_fleet_sim_tele
fleet.sim_telemetry(radius=[1.0, 2.0, 3.0, 4.0])                                # (the Python form; resets)
assert launches_per_tick() == plain + 1
d = fleet.sim_telemetry_read()
assert d["act"].shape == (N, 5) and d["rank"].dtype == np.int64 and abs(d["track_length"] - 2382.2979975) < 1e-6
fleet.sim_telemetry(radius=None)
assert launches_per_tick() == plain
expect(read(), 1, "telemetry is off")
try:
    fleet.sim_telemetry_read()
    raise AssertionError("read while off accepted")
except _capi.BackendError:
    pass
fresh([1, 3])
with_mates = launches_per_tick()
assert with_mates == plain + 1                                                  # + k_fleet_sim_mates
fleet.sim_telemetry()
assert launches_per_tick() == with_mates + 2                                    # + k_fleet_sim_tele + k_fleet_sim_rank
fresh([1, 1, 1, 1])
fleet.sim_telemetry(grid_s=0.0)
assert launches_per_tick() == plain + 1                                         # races of size 1: no rank kernel
fresh()                                                                         # sim_setup switches the telemetry off
assert launches_per_tick() == plain
expect(read(), 1, "telemetry is off")
# telemetry may be set before the races (after sim_setup at any time between runs)
fresh()
fleet.sim_telemetry()
fleet.sim_race([2, 2])
assert launches_per_tick() == plain + 3

# an allocation failing at every point of ltpl_fleet_sim_telemetry: the previous telemetry stays in place and works
def telemetry_set():
    fresh()
    assert call()[0] == 0


def telemetry_kept(k, _):
    intact()
    assert launches_per_tick() == plain + 1


failures = common.alloc_sweep("ltpl_fleet_sim_telemetry", lambda: call(radius=1.0), 32, telemetry_kept, before=telemetry_set)
assert failures >= 7, failures
print("allocation failure at each of the %d allocations of ltpl_fleet_sim_telemetry: previous telemetry kept" % failures)
print("launches per tick: %d without telemetry, %d with, %d with a race" % (plain, plain + 1, plain + 3))
common.finish("sim telemetry args OK")
