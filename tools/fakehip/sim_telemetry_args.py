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
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from graphbasedlocaltrajectoryplanner_amd import _capi, sim               # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet, SimTeleIn   # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.lattice import Lattice          # noqa: E402

FAKE = os.path.join(ROOT, "tools", "fakehip", "build_plain", "libltpl_hip_fake.so")
N = 4
D = sim.TELEMETRY_DOUBLES
lat = Lattice.load(os.path.join(ROOT, "tests", "golden", "monteblanco_lattice.npz"))
table = sim.RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))
hip = _capi.HipBackend(lat, lib_path=FAKE)
lib = hip.lib
lib.fakehip_launch_count.restype = ctypes.c_long
lib.fakehip_fail_malloc_after.argtypes = [ctypes.c_long]
lib.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
lib.hipFree.argtypes = [ctypes.c_void_p]
lib.ltpl_fleet_last_error.restype = ctypes.c_char_p
lib.ltpl_fleet_last_error.argtypes = [ctypes.c_void_p]
lib.ltpl_fleet_sim_telemetry.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.ltpl_fleet_sim_telemetry_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
fleet = Fleet(hip, N)
h = fleet.handle


def no_allocation(fn):
    """Runs ``fn`` with an allocation failure armed for the next hipMalloc; asserts that ``fn`` did not allocate (the failure is still
    pending afterwards). Returns ``fn``'s result."""
    lib.fakehip_fail_malloc_after(1)
    try:
        out = fn()
    finally:
        p = ctypes.c_void_p()
        pending = lib.hipMalloc(ctypes.byref(p), 8) != 0
        if not pending:
            lib.hipFree(p)
        lib.fakehip_fail_malloc_after(0)
    assert pending, "a refused call allocated device memory"
    return out


def call(radius=2.5, grid_s=None):
    rad = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float64), (N,)))
    ti = SimTeleIn()
    ti.radius = rad.ctypes.data
    if grid_s is not None:
        gs = np.ascontiguousarray(np.broadcast_to(np.asarray(grid_s, np.float64), (N,)))
        ti.grid_s = gs.ctypes.data
    rc = lib.ltpl_fleet_sim_telemetry(h, ctypes.byref(ti))
    return rc, (lib.ltpl_fleet_last_error(h) or b"").decode()


def read(doubles=D):
    out = np.full((N, D), 7.0)
    L = ctypes.c_double(0.0)
    rc = lib.ltpl_fleet_sim_telemetry_read(h, out.ctypes.data, doubles, ctypes.byref(L))
    return rc, out, L.value, (lib.ltpl_fleet_last_error(h) or b"").decode()


def expect(rc_msg, code, text):
    rc, msg = rc_msg[0], rc_msg[-1]
    assert rc == code and text in msg, (rc, msg, code, text)
    print("refused (%d): %s" % (rc, msg))


def launches_per_tick():
    before = lib.fakehip_launch_count()
    fleet.sim_run(1, trace=False)
    return lib.fakehip_launch_count() - before


BEFORE = np.zeros(D)
BEFORE[[1, 4, 5, 6, 21]] = np.nan
BEFORE[8], BEFORE[14], BEFORE[15], BEFORE[16] = -np.inf, np.inf, -1.0, -1.0


def intact():
    """The telemetry set before a refused call is still there: a read succeeds and returns the untouched records."""
    rc, out, L, _ = read()
    assert rc == 0 and abs(L - 2382.2979975) < 1e-6 and all(np.array_equal(row, BEFORE, equal_nan=True) for row in out), (rc, L, out)


good = dict(opponents=[(250.0, 0.3, 5.0)], pref=("right", "straight"), pos_est=(0.0, 0.0), zone_gids=[3])


def fresh(races=None):
    fleet.sim_setup(table, [good] * N)
    fleet.sim_vel()
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
failures = 0
for k in range(1, 32):
    fresh()
    assert call()[0] == 0
    lib.fakehip_fail_malloc_after(k)
    rc, msg = call(radius=1.0)
    lib.fakehip_fail_malloc_after(0)
    if rc == 0:
        break
    assert rc == 3 and "hipMalloc" in msg, (k, rc, msg)                         # LTPL_ERR_HIP
    failures += 1
    intact()
    assert launches_per_tick() == plain + 1
else:
    raise AssertionError("ltpl_fleet_sim_telemetry never succeeded")
assert failures >= 7, failures
print("allocation failure at each of the %d allocations of ltpl_fleet_sim_telemetry: previous telemetry kept" % failures)
print("launches per tick: %d without telemetry, %d with, %d with a race" % (plain, plain + 1, plain + 3))
fleet.close()
hip.close()
print("sim telemetry args OK")
