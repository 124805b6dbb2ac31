"""TEST TOOL: argument checks of ltpl_fleet_sim_race / ltpl_fleet_sim_heading (the races of the fleet simulation) without a device. The
library's host code built against the stand-in runtime without sanitizers (FAKEHIP_SAN=none tools/fakehip/build.sh); kernels do nothing,
so results are not looked at -- only the return codes, the messages and the number of kernel launches per simulated tick:
  - the capacity rule (opponents + statics + race size - 1 <= 96) and every invalid argument are refused before any device allocation
    (an allocation failure armed for the next hipMalloc is still pending after the refused call);
  - a race with more than one planner adds exactly one launch per tick (k_fleet_sim_mates); races of size 1 add none;
  - ltpl_fleet_sim_setup clears the races; ltpl_fleet_sim_race after a run is refused;
  - an allocation failing at any point of ltpl_fleet_sim_race leaves the fleet with its previous races and staging: the call returns
    LTPL_ERR_HIP and the next run launches what the previous state launches."""
import ctypes

import numpy as np

import sim_args_common as common
from sim_args_common import expect, launches_per_tick, no_allocation
from graphbasedlocaltrajectoryplanner_amd.fleet import SimRaceIn

N = 4
lib, fleet, table = common.start(N)
lib.ltpl_fleet_sim_race.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.ltpl_fleet_sim_heading.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
h = fleet.handle


def call(off, length=5.0, heading0=0.0, n_races=None):
    off = np.ascontiguousarray(np.asarray(off, np.int32))
    lens = np.ascontiguousarray(np.broadcast_to(np.asarray(length, np.float64), (N,)))
    h0 = np.ascontiguousarray(np.broadcast_to(np.asarray(heading0, np.float64), (N,)))
    ri = SimRaceIn()
    ri.n_races = len(off) - 1 if n_races is None else n_races
    ri.race_off, ri.length, ri.heading0 = off.ctypes.data, lens.ctypes.data, h0.ctypes.data
    before = lib.fakehip_launch_count()
    rc = lib.ltpl_fleet_sim_race(h, ctypes.byref(ri))
    return rc, lib.fakehip_launch_count() - before, (lib.ltpl_fleet_last_error(h) or b"").decode()


assert lib.ltpl_fleet_sim_race(None, None) == 1 and lib.ltpl_fleet_sim_heading(None, None) == 1
expect(no_allocation(lambda: call([0, N])), 1, "ltpl_fleet_sim_setup first")
assert lib.ltpl_fleet_sim_heading(h, np.zeros(N).ctypes.data) == 1

good = common.GOOD_ENTRY
crowded = dict(good, opponents=[(10.0 * k, 0.3, 5.0) for k in range(95)])
fleet.sim_setup(table, [crowded, good, good, good])
fleet.sim_vel()
# capacity: 95 opponents + a race of 3 (2 mates) > 96; a race of 2 (1 mate) fits
expect(no_allocation(lambda: call([0, 3, 4])), 4, "above 96")                    # LTPL_ERR_CAPACITY
assert call([0, 2, 4])[0] == 0
fleet.sim_setup(table, [crowded, good, good, good])
fleet.sim_vel()
for off, kw, text in (([0, 2, 3], {}, "cover the planners"), ([1, 2, 4], {}, "cover the planners"),
                      ([0, 3, 2, 4], {}, "must not decrease"), ([0, 4], dict(n_races=0), "race offsets missing"),
                      ([0, 4], dict(length=0.0), "finite and positive"), ([0, 4], dict(length=-5.0), "finite and positive"),
                      ([0, 4], dict(length=np.nan), "finite and positive"), ([0, 4], dict(length=np.inf), "finite and positive"),
                      ([0, 4], dict(heading0=np.nan), "heading0 must be finite"), ([0, 4], dict(heading0=-np.inf), "heading0 must be finite")):
    expect(no_allocation(lambda: call(off, **kw)), 1, text)                    # LTPL_ERR_INVALID_ARG
# null arrays
ri = SimRaceIn()
off = np.array([0, N], np.int32)
ri.n_races, ri.race_off = 1, off.ctypes.data
assert no_allocation(lambda: lib.ltpl_fleet_sim_race(h, ctypes.byref(ri))) == 1 and b"missing" in lib.ltpl_fleet_last_error(h)


def fresh():
    common.fresh([crowded, good, good, good])               # (clears the races)


fresh()
plain = launches_per_tick()
expect(no_allocation(lambda: call([0, 2, 4])), 1, "before the first ltpl_fleet_sim_run")      # races come before the first run
fresh()
assert call([0, 1, 2, 3, 4])[0] == 0                        # races of size 1: today's kernels
assert launches_per_tick() == plain
fresh()
fleet.sim_race([1, 2, 1], heading0=[0.5, -0.5, 1.0, 3.0])    # (the Python form: sizes)
assert launches_per_tick() == plain + 1                      # + k_fleet_sim_mates
fresh()
fleet.sim_race([range(0, 1), range(1, 4)], length=[4.0, 5.0, 6.0, 7.0])
assert launches_per_tick() == plain + 1
try:
    fleet.sim_race([range(0, 2), range(3, 4)])
    raise AssertionError("ranges with a gap accepted")
except ValueError:
    pass
fresh()                                                      # sim_setup clears the races
assert launches_per_tick() == plain
assert lib.ltpl_fleet_sim_heading(h, np.zeros(N).ctypes.data) == 0
# an allocation failing at every point of ltpl_fleet_sim_race: the previous state (here: races of 1, 1, 2) stays in place and works
def races_1_1_2():
    fresh()
    assert call([0, 1, 2, 4])[0] == 0


def still_runs(k, _):
    assert launches_per_tick() == plain + 1                  # the previous races still run (their buffers were not freed)
    assert fleet.sim_state()["pos_est"].shape == (N, 2)


def mates_run():
    assert launches_per_tick() == plain + 1


failures = common.alloc_sweep("ltpl_fleet_sim_race", lambda: call([0, 2, 4]), 64, still_runs, before=races_1_1_2, after_success=mates_run)
assert failures >= 10, failures
print("allocation failure at each of the %d allocations of ltpl_fleet_sim_race: previous state kept" % failures)
print("launches per tick: %d without mates, %d with" % (plain, plain + 1))
# exactly at the cap: 93 own objects + 3 mates = 96 fits, one own object more is refused
at_cap = dict(good, opponents=[(10.0 * k, 0.3, 5.0) for k in range(93)])
fleet.sim_setup(table, [at_cap] * N)
fleet.sim_vel()
assert call([0, N])[0] == 0
fleet.sim_setup(table, [at_cap] * (N - 1) + [dict(at_cap, static=[(0.0, 0.0, 0.0, 0.0, 4.0)])])
fleet.sim_vel()
expect(no_allocation(lambda: call([0, N])), 4, "above 96")                       # LTPL_ERR_CAPACITY
print("own objects + mates: 96 accepted, 97 refused")
common.finish("sim race args OK")
