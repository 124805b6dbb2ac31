"""TEST TOOL: argument checks of ltpl_fleet_sim_record / _record_info / _record_get (the flight recorder of the fleet simulation) without a
device. The library's host code built against the stand-in runtime without sanitizers (FAKEHIP_SAN=none tools/fakehip/build.sh); kernels
do nothing, so a record read back is the zeroed ring -- only the return codes, the messages, the tick bookkeeping and the number of kernel
launches per simulated tick are looked at:
  - every error case (no simulation, an index outside 0 .. n - 1, an index given twice, depth < 1, a tick the ring does not hold, a slot
    outside the recorded planners, a read while off) returns LTPL_ERR_INVALID_ARG before any device allocation, the previous recorder intact;
  - a recorder adds two launches per tick to the unfused sequence (k_fleet_sim_rec_paths, k_fleet_sim_rec_vel); off, and after
    ltpl_fleet_sim_setup, a tick launches what it launched before;
  - an allocation failing at any point of ltpl_fleet_sim_record leaves the previous recorder, its depth and its tick count in place."""
import os

import numpy as np

import sim_args_common as common
from sim_args_common import expect, fresh, launches_per_tick, msg, no_allocation

N = 6
lib, fleet, table = common.start(N)
h = fleet.handle


def record(planners, depth):
    idx = np.ascontiguousarray(np.asarray(planners, np.int32))
    rc = lib.ltpl_fleet_sim_record(h, idx.ctypes.data if idx.size else None, int(idx.size), depth)
    return rc, msg()


def get(tick, slot):
    return lib.ltpl_fleet_sim_record_get(h, tick, slot, None, None, None, None, None), msg()



assert lib.ltpl_fleet_sim_record(None, None, 0, 1) == 1 and lib.ltpl_fleet_sim_record_info(None, None, None, None, None) == 1
expect(no_allocation(lambda: record([0], 2)), 1, "ltpl_fleet_sim_setup first")
expect(no_allocation(lambda: get(0, 0)), 1, "ltpl_fleet_sim_setup first")
fresh()
fused = launches_per_tick()
os.environ["LTPL_FLEET_NO_FUSE"] = "1"
unfused_fleet = common.Fleet(common.hip, N)
unfused_fleet.sim_setup(table, [common.GOOD_ENTRY] * N)
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
def three_ticks_recorded():
    fresh()
    assert record([4, 2], 5)[0] == 0
    fleet.sim_run(3, trace=False)


def recorder_kept(k, _):
    assert fleet.sim_record_info() == dict(n_planners=2, depth=5, first_tick=0, n_ticks=3)
    assert launches_per_tick() == unfused + 2 and get(3, 1)[0] == 0


failures = common.alloc_sweep("ltpl_fleet_sim_record", lambda: record([0], 9), 16, recorder_kept, before=three_ticks_recorded)
assert failures >= 2, failures
print("allocation failure at each of the %d allocations of ltpl_fleet_sim_record: previous recorder kept" % failures)
print("launches per tick: %d fused, %d unfused, %d with a recorder" % (fused, unfused, unfused + 2))
common.finish("sim record args OK")
