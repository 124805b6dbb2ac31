"""TEST TOOL: argument checks of ltpl_fleet_sim_record / _record_info / _record_get (the flight recorder of the fleet simulation) without a
device. The library's host code built against the stand-in runtime without sanitizers (FAKEHIP_SAN=none tools/fakehip/build.sh); kernels
do nothing, so a record read back is the zeroed ring -- only the return codes, the messages, the tick bookkeeping and the number of kernel
launches per simulated tick are looked at:
  - every error case (no simulation, an index outside 0 .. n - 1, an index given twice, depth < 1, a tick the ring does not hold, a slot
    outside the recorded planners, a read while off) returns LTPL_ERR_INVALID_ARG before any device allocation, the previous recorder intact;
  - a recorder adds two launches per tick to the unfused sequence (k_fleet_sim_rec_paths, k_fleet_sim_rec_vel); off, and after
    ltpl_fleet_sim_setup, a tick launches what it launched before;
  - an allocation failing at any point of ltpl_fleet_sim_record leaves the previous recorder, its depth and its tick count in place."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from graphbasedlocaltrajectoryplanner_amd import _capi, sim               # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet              # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.lattice import Lattice          # noqa: E402

FAKE = os.path.join(ROOT, "tools", "fakehip", "build_plain", "libltpl_hip_fake.so")
N = 6
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
fleet = Fleet(hip, N)
h = fleet.handle


def no_allocation(fn):
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


def record(planners, depth):
    idx = np.ascontiguousarray(np.asarray(planners, np.int32))
    rc = lib.ltpl_fleet_sim_record(h, idx.ctypes.data if idx.size else None, int(idx.size), depth)
    return rc, (lib.ltpl_fleet_last_error(h) or b"").decode()


def get(tick, slot):
    rc = lib.ltpl_fleet_sim_record_get(h, tick, slot, None, None, None, None, None)
    return rc, (lib.ltpl_fleet_last_error(h) or b"").decode()


def expect(rc_msg, code, text):
    rc, msg = rc_msg
    assert rc == code and text in msg, (rc, msg, code, text)
    print("refused (%d): %s" % (rc, msg))


def launches_per_tick(n=1):
    before = lib.fakehip_launch_count()
    fleet.sim_run(n, trace=False)
    return (lib.fakehip_launch_count() - before) // n


good = dict(opponents=[(250.0, 0.3, 5.0)], pref=("right", "straight"), pos_est=(0.0, 0.0), zone_gids=[3])


def fresh():
    fleet.sim_setup(table, [good] * N)
    fleet.sim_vel()


assert lib.ltpl_fleet_sim_record(None, None, 0, 1) == 1 and lib.ltpl_fleet_sim_record_info(None, None, None, None, None) == 1
expect(no_allocation(lambda: record([0], 2)), 1, "ltpl_fleet_sim_setup first")
expect(no_allocation(lambda: get(0, 0)), 1, "ltpl_fleet_sim_setup first")
fresh()
fused = launches_per_tick()
os.environ["LTPL_FLEET_NO_FUSE"] = "1"
unfused_fleet = Fleet(hip, N)
unfused_fleet.sim_setup(table, [good] * N)
unfused_fleet.sim_vel()
before = lib.fakehip_launch_count()
unfused_fleet.sim_run(1, trace=False)
unfused = lib.fakehip_launch_count() - before
unfused_fleet.close()
del os.environ["LTPL_FLEET_NO_FUSE"]
assert unfused == fused + 1, (fused, unfused)
expect(no_allocation(lambda: get(0, 0)), 1, "recorder is off")
assert fleet.sim_record_info() == dict(n_planners=0, depth=0, first_tick=0, n_ticks=0)
assert record([], 3)[0] == 0                                                    # off while off: nothing to do
assert record([5, 0, 3], 4)[0] == 0
assert fleet.sim_record_info() == dict(n_planners=3, depth=4, first_tick=0, n_ticks=0)
assert launches_per_tick(6) == unfused + 2                                      # + k_fleet_sim_rec_paths + k_fleet_sim_rec_vel
assert fleet.sim_record_info() == dict(n_planners=3, depth=4, first_tick=2, n_ticks=4)
for args, text in ((([0, N], 4), "out of range"), (([-1], 4), "out of range"), (([2, 4, 2], 4), "given twice"), (([1], 0), "depth must be positive"),
                   (([1], -3), "depth must be positive"), ((list(range(N)) + [0], 2), "more recorded planners")):
    expect(no_allocation(lambda: record(*args)), 1, text)
    assert fleet.sim_record_info() == dict(n_planners=3, depth=4, first_tick=2, n_ticks=4)
for args, text in (((1, 0), "does not hold this tick"), ((6, 0), "does not hold this tick"), ((-1, 0), "does not hold this tick"),
                   ((3, 3), "slot outside"), ((3, -1), "slot outside")):
    expect(get(*args), 1, text)
assert get(2, 0)[0] == 0 and get(5, 2)[0] == 0
recs = fleet.sim_record_read()
assert len(recs) == 4 and all(len(r) == 3 for r in recs)
assert launches_per_tick() == unfused + 2                                       # bad arguments did not switch it off
assert record([1], 1)[0] == 0                                                   # a new recorder restarts tick 0
assert fleet.sim_record_info() == dict(n_planners=1, depth=1, first_tick=0, n_ticks=0)
fleet.sim_record(None)
assert launches_per_tick() == fused
fleet.sim_record(range(N), 2)
fresh()                                                                         # sim_setup switches the recorder off
assert launches_per_tick() == fused and fleet.sim_record_info()["n_planners"] == 0
# before and after the races and the telemetry
fresh()
fleet.sim_record([0, 1], 3)
fleet.sim_race([2, 4])
fleet.sim_telemetry()
assert launches_per_tick() == unfused + 2 + 3
assert fleet.sim_record_info() == dict(n_planners=2, depth=3, first_tick=0, n_ticks=1)

# an allocation failing at every point of ltpl_fleet_sim_record: the previous recorder stays in place and works
failures = 0
for k in range(1, 16):
    fresh()
    assert record([4, 2], 5)[0] == 0
    fleet.sim_run(3, trace=False)
    lib.fakehip_fail_malloc_after(k)
    rc, msg = record([0], 9)
    lib.fakehip_fail_malloc_after(0)
    if rc == 0:
        break
    assert rc == 3 and "hipMalloc" in msg, (k, rc, msg)                         # LTPL_ERR_HIP
    failures += 1
    assert fleet.sim_record_info() == dict(n_planners=2, depth=5, first_tick=0, n_ticks=3)
    assert launches_per_tick() == unfused + 2 and get(3, 1)[0] == 0
else:
    raise AssertionError("ltpl_fleet_sim_record never succeeded")
assert failures >= 2, failures
print("allocation failure at each of the %d allocations of ltpl_fleet_sim_record: previous recorder kept" % failures)
print("launches per tick: %d fused, %d unfused, %d with a recorder" % (fused, unfused, unfused + 2))
fleet.close()
hip.close()
print("sim record args OK")
