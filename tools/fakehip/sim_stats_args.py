"""TEST TOOL: argument checks of ltpl_fleet_sim_stats / _stats_reduce / _stats_series / _stats_eval (the campaign statistics of the fleet
simulation, csrc/fleet_stats.hpp) without a device. The library's host code built against the stand-in runtime without sanitizers
(FAKEHIP_SAN=none tools/fakehip/build.sh); kernels do nothing, so no row is looked at -- only the return codes, the messages and the
kernel launches (by number and, through fakehip_launches_of, by name):
  - every refused call (null fleet, no simulation, n_groups outside 1 .. 4096, a group index outside -1 .. G - 1, n_measures outside
    1 .. 64, a missing array, an unknown family, a column outside the family's record, a family whose module is off, bins outside 1 .. 16,
    lo / hi not finite or not lo < hi, top_dir outside -1 / 0 / +1, top_k outside 0 .. 8, a negative period, a period without a depth, a
    negative tick0, an unknown flag, KEEP_SERIES with another shape; the reduce's and the series' sizes; the hook's counts, arrays, offsets
    and specs) returns LTPL_ERR_INVALID_ARG -- a series above 256 MiB LTPL_ERR_CAPACITY -- with a message that names the argument, before
    any device allocation, and launches nothing;
  - a refused or failing call keeps the previous plan and series; an allocation failing at each allocation of the call is LTPL_ERR_HIP,
    and the fleet runs on;
  - launches by kernel name: with no plan, a cleared plan or after ltpl_fleet_sim_setup a tick launches what it launched before and the
    statistics kernels never; a plan without a period launches them in ltpl_fleet_sim_stats_reduce only; a plan with period P launches
    the two kernels exactly on the ticks with (tick0 + ticks since the call + 1) % P == 0, looked at tick by tick over 2 P + 1 ticks;
  - a module switched off under the plan: reduce and a run with a period refuse, naming the family, before the first tick;
  - snapshot, restore and branch launch nothing of the statistics."""
import ctypes

import numpy as np

import sim_args_common as common
from sim_args_common import CAPACITY, I32, INVALID, P, expect, launches, msg, quiet, run1, sim
from graphbasedlocaltrajectoryplanner_amd.fleet import SimStatsIn

N = 4
lib, fleet, table = common.start(N)
lib.ltpl_fleet_sim_stats.argtypes = [P, P]
lib.ltpl_fleet_sim_stats_reduce.argtypes = [P, P, I32, P, I32]
lib.ltpl_fleet_sim_stats_series.argtypes = [P, P, P, I32, P, P]
lib.ltpl_fleet_sim_stats_eval.argtypes = [P, I32] + [P] * 6
h = fleet.handle
RD = sim.STATS_DOUBLES
TELE, SAF, STATE = sim.STATS_FAMILIES.index("telemetry"), sim.STATS_FAMILIES.index("safety"), sim.STATS_FAMILIES.index("state")
CHUNK, MERGE, EVAL = b"_Z23k_fleet_sim_stats_chunk", b"_Z23k_fleet_sim_stats_merge", b"_Z22k_fleet_sim_stats_eval"
GOOD = dict(n_groups=2, group=[0, 1, -1, 1], family=[TELE, STATE], column=[14, 0], lo=[0.0, 0.0], hi=[10.0, 2.0], bins=[8, 2], top_dir=[-1, 1],
            top_k=2, period=0, depth=0, tick0=0, flags=0)


def stats(missing=None, n_measures=None, **over):
    a = dict(GOOD, **over)
    keep = dict(group=np.ascontiguousarray(np.broadcast_to(np.asarray(a["group"], np.int32), (N,))))
    for k, dt in (("family", np.int32), ("column", np.int32), ("lo", np.float64), ("hi", np.float64), ("bins", np.int32), ("top_dir", np.int32)):
        keep[k] = np.ascontiguousarray(np.asarray(a[k], dt).reshape(-1))
    si = SimStatsIn()
    si.n_groups, si.n_measures = a["n_groups"], len(keep["family"]) if n_measures is None else n_measures
    for k, arr in keep.items():
        setattr(si, k, None if k == missing else arr.ctypes.data)
    si.top_k, si.period, si.depth, si.tick0, si.flags = a["top_k"], a["period"], a["depth"], a["tick0"], a["flags"]
    return lib.ltpl_fleet_sim_stats(h, ctypes.byref(si)), msg()


def named(fn):
    """(chunk, merge, hook) launches during ``fn``."""
    before = [lib.fakehip_launches_of(k) for k in (CHUNK, MERGE, EVAL)]
    fn()
    return tuple(lib.fakehip_launches_of(k) - b for k, b in zip((CHUNK, MERGE, EVAL), before))


def fresh(tele=True):
    common.fresh(common.moving_entries(N))
    if tele:
        fleet.sim_telemetry()


rows, tops = np.zeros((4, 4, RD)), np.zeros((4, 4, 8, 2))
ticks, ring = np.zeros(64, np.int32), np.zeros((64, 4, 4, RD))
held, total = ctypes.c_int32(0), ctypes.c_int64(0)


def reduce(size=RD, out=True, top=True, k=2):
    return lib.ltpl_fleet_sim_stats_reduce(h, rows.ctypes.data if out else None, size, tops.ctypes.data if top else None, k), msg()


def series(size=RD):
    return lib.ltpl_fleet_sim_stats_series(h, ticks.ctypes.data, ring.ctypes.data, size, ctypes.byref(held), ctypes.byref(total)), msg()


# null fleet, no simulation
assert lib.ltpl_fleet_sim_stats(None, None) == INVALID and lib.ltpl_fleet_sim_stats_reduce(None, rows.ctypes.data, RD, None, 0) == INVALID
assert lib.ltpl_fleet_sim_stats_series(None, None, None, RD, None, None) == INVALID and lib.ltpl_fleet_sim_stats_eval(None, 0, *([None] * 6)) == INVALID
expect(quiet(lambda: stats()), "ltpl_fleet_sim_setup first")
expect(quiet(lambda: (lib.ltpl_fleet_sim_stats(h, None), msg())), "ltpl_fleet_sim_setup first")
expect(quiet(reduce), "ltpl_fleet_sim_setup first")
expect(quiet(series), "ltpl_fleet_sim_setup first")

fresh()
plain = launches(run1)
assert named(run1) == (0, 0, 0)
expect(quiet(reduce), "no plan")
expect(quiet(series), "no series")
assert quiet(lambda: lib.ltpl_fleet_sim_stats(h, None)) == 0                # clearing what is off: nothing to do, nothing allocated


def refusals():
    for bad in (0, -1, 4097):
        expect(quiet(lambda: stats(n_groups=bad)), "n_groups must be 1 .. 4096")
    for bad in ([0, 1, -2, 1], [0, 2, 0, 0], 2):
        expect(quiet(lambda: stats(group=bad)), "group must be -1 .. n_groups - 1")
    for bad in (0, -1, 65):
        expect(quiet(lambda: stats(n_measures=bad)), "n_measures must be 1 .. 64")
    for name in ("group", "family", "column", "lo", "hi", "bins", "top_dir"):
        expect(quiet(lambda: stats(missing=name)), "missing")
    for bad in (-1, len(sim.STATS_FAMILIES)):
        expect(quiet(lambda: stats(family=[TELE, bad])), "measure 1: unknown family")
    expect(quiet(lambda: stats(column=[sim.TELEMETRY_DOUBLES, 0])), "measure 0: column outside the 22 doubles of family telemetry")
    expect(quiet(lambda: stats(column=[0, 1])), "measure 1: column outside the 1 doubles of family state")
    expect(quiet(lambda: stats(column=[-1, 0])), "measure 0: column")
    expect(quiet(lambda: stats(family=[TELE, SAF])), "measure 1: family safety is off")
    for bad in (0, 17, -3):
        expect(quiet(lambda: stats(bins=[8, bad])), "measure 1: bins must be 1 .. 16")
    for bad in (np.nan, np.inf, -np.inf):
        expect(quiet(lambda: stats(lo=[bad, 0.0])), "measure 0: lo and hi must be finite")
        expect(quiet(lambda: stats(hi=[10.0, bad])), "measure 1: lo and hi must be finite")
    for lo in (10.0, 11.0):
        expect(quiet(lambda: stats(lo=[lo, 0.0])), "measure 0: lo must be below hi")
    for bad in (2, -2):
        expect(quiet(lambda: stats(top_dir=[bad, 0])), "measure 0: top_dir")
    for bad in (-1, 9):
        expect(quiet(lambda: stats(top_k=bad)), "top_k must be 0 .. 8")
    expect(quiet(lambda: stats(period=-1)), "period must not be negative")
    for bad in (0, -1):
        expect(quiet(lambda: stats(period=3, depth=bad)), "depth must be positive")
    expect(quiet(lambda: stats(tick0=-1)), "tick0")
    expect(quiet(lambda: stats(flags=2)), "unknown flag")
    expect(quiet(lambda: stats(period=1, depth=2 ** 31 - 1)), "256 MiB", CAPACITY)
    expect(quiet(lambda: stats(n_groups=4096, group=0, family=[TELE] * 64, column=[0] * 64, lo=[0.0] * 64, hi=[1.0] * 64, bins=[1] * 64,
                               top_dir=[0] * 64, period=1, depth=5)), "256 MiB", CAPACITY)


refusals()
# the edges that are arguments; a plan without a period: nothing in the tick, the two kernels in reduce
assert stats(n_groups=4096, group=-1, bins=[1, 16], top_k=0, tick0=2 ** 31 - 1)[0] == 0
assert stats(top_k=8, lo=[-5e-324, 0.0], hi=[0.0, 5e-324])[0] == 0
assert stats()[0] == 0
assert launches(run1) == plain and named(lambda: fleet.sim_run(5, trace=False)) == (0, 0, 0)
assert named(lambda: reduce()) == (1, 1, 0) and reduce()[0] == 0
assert reduce(top=False, k=0)[0] == 0
expect(quiet(lambda: reduce(size=RD - 1)), "row size")
expect(quiet(lambda: reduce(out=False)), "rows_out missing")
expect(quiet(lambda: reduce(k=3)), "top_k is not the plan's")
expect(quiet(series), "no series")
# a refused call keeps the previous plan
refusals()
assert named(lambda: reduce()) == (1, 1, 0)
# groups without a member: no chunk, the merge alone
assert stats(group=-1)[0] == 0 and named(lambda: reduce()) == (0, 1, 0)

# a series: the two kernels exactly on the ticks of the rule, tick by tick over 2 P + 1 ticks
for period, tick0 in ((3, 0), (4, 2), (1, 7), (5, 4)):
    assert stats(period=period, depth=2, tick0=tick0)[0] == 0
    seen = []
    for k in range(2 * period + 1):
        got = named(run1)
        assert got in ((0, 0, 0), (1, 1, 0)), got
        seen.append(got[0])
    want = [1 if (tick0 + k + 1) % period == 0 else 0 for k in range(2 * period + 1)]
    assert seen == want, (period, tick0, seen, want)
    n_rows = sum(want)
    assert series()[0] == 0 and total.value == n_rows and held.value == min(n_rows, 2), (period, held.value, total.value)
    assert [int(t) for t in ticks[:held.value]] == [tick0 + k for k in range(2 * period + 1) if want[k]][-held.value:]
    assert launches(lambda: fleet.sim_run(period, trace=False)) == period * plain + 2
    print("period %d, tick0 %d: reductions on ticks %s of %d" % (period, tick0, [k for k, w in enumerate(want) if w], 2 * period + 1))
expect(quiet(lambda: series(size=RD + 1)), "row size")
# KEEP_SERIES: the ring and its count stay with the same shape, and only then
assert stats(period=2, depth=3)[0] == 0
fleet.sim_run(4, trace=False)
assert series()[0] == 0 and total.value == 2
assert stats(period=1, depth=3, flags=1, lo=[1.0, 0.0], tick0=50)[0] == 0
assert series()[0] == 0 and total.value == 2 and held.value == 2
fleet.sim_run(2, trace=False)
assert series()[0] == 0 and total.value == 4 and held.value == 3 and [int(t) for t in ticks[:3]] == [3, 50, 51]
for bad in (dict(depth=4), dict(n_groups=3), dict(period=0), dict(family=[TELE], column=[0], lo=[0.0], hi=[1.0], bins=[1], top_dir=[0])):
    expect(quiet(lambda: stats(**dict(dict(period=1, depth=3, flags=1), **bad))), "LTPL_SIM_STATS_KEEP_SERIES")
assert series()[0] == 0 and total.value == 4
assert stats(period=1, depth=3)[0] == 0 and series()[0] == 0 and total.value == 0          # without the flag the series starts anew
# snapshot, restore and branch: nothing of the statistics is launched, plan and series stay
fleet.sim_run(1, trace=False)
assert named(lambda: (fleet.sim_snapshot(0), fleet.sim_restore(0), fleet.sim_branch(0, [1, 2]))) == (0, 0, 0)
assert series()[0] == 0 and total.value == 1 and named(run1) == (1, 1, 0)
# a module switched off under the plan: reduce and a periodic run refuse before the first tick; cleared, the fleet runs on
fleet.sim_telemetry(None)
expect(quiet(reduce), "family telemetry is off")
before = lib.fakehip_launch_count()
try:
    fleet.sim_run(2, trace=False)
    raise AssertionError("a run over a family that is off was not refused")
except common._capi.BackendError as e:
    assert "family telemetry is off" in str(e), e
assert lib.fakehip_launch_count() == before
assert stats(family=[STATE, STATE], column=[0, 0])[0] == 0 and named(run1) == (0, 0, 0)     # (a plan on the state alone needs no module)
assert lib.ltpl_fleet_sim_stats(h, None) == 0
plain_off = launches(run1)
assert named(run1) == (0, 0, 0)
expect(quiet(reduce), "no plan")
fleet.sim_telemetry()
assert stats(period=1, depth=2)[0] == 0 and named(run1) == (1, 1, 0)
fresh()                                                                      # sim_setup clears the plan
assert launches(run1) == plain and named(run1) == (0, 0, 0)
expect(quiet(reduce), "no plan")

# an allocation failing at each allocation of ltpl_fleet_sim_stats: setting, replacing, and replacing with KEEP_SERIES
for what, call, ok_after, n_alloc in (("setting", lambda: stats(period=2, depth=2), 0, 16), ("replacing", lambda: stats(period=2, depth=2, top_k=1), 1, 16),
                                      ("keeping the series", lambda: stats(period=2, depth=2, top_k=1, flags=1), 1, 15)):
    def still(k, _):
        assert (reduce(k=2 if what == "replacing" else 1)[0] == 0) == (ok_after == 1), (what, k)      # the previous state: no plan / the old plan
        assert launches(lambda: fleet.sim_run(2, trace=False)) == 2 * plain + 2 * ok_after, (what, k)
    failures = common.alloc_sweep("ltpl_fleet_sim_stats", call, 60, still)
    assert failures == n_alloc, (what, failures)
    print("%s: allocation failure at each of the %d allocations of ltpl_fleet_sim_stats: the fleet runs on" % (what, failures))
assert lib.ltpl_fleet_sim_stats(h, None) == 0 and named(run1) == (0, 0, 0)

# the hook
M = 2
vals, idx, spec = np.zeros(4000), np.arange(4000, dtype=np.int32), np.tile(np.array([0.0, 1.0, 4.0, -1.0, 3.0]), (M, 1))
hrow, htop = np.zeros((M, RD)), np.zeros((M, 8, 2))


def hook(n=M, off=(0, 1, 2), hole=None, specs=spec, planners=idx):
    o = np.array(off, np.int32)
    args = [o.ctypes.data, vals.ctypes.data, planners.ctypes.data, specs.ctypes.data, hrow.ctypes.data, htop.ctypes.data]
    if hole is not None:
        args[hole] = None
    return lib.ltpl_fleet_sim_stats_eval(h, n, *args), msg()


expect(quiet(lambda: hook(n=-1)), "n_cases")
expect(quiet(lambda: (lib.ltpl_fleet_sim_stats_eval(h, 4097, *([None] * 6)), msg())), "at most 4096 cases")
for hole in (0, 1, 3, 4, 5):
    expect(quiet(lambda: hook(hole=hole)), "missing")
expect(quiet(lambda: hook(off=(1, 2, 3))), "start at 0")
expect(quiet(lambda: hook(off=(0, 3, 2))), "case 1: value offsets must not decrease")
for c, bad, text in ((2, 0.0, "bins"), (2, 17.0, "bins"), (2, 2.5, "bins"), (0, np.nan, "lo and hi must be finite"), (1, np.inf, "lo and hi must be finite"),
                     (0, 1.0, "lo must be below hi"), (3, 2.0, "top_dir"), (3, 0.5, "top_dir"), (4, 9.0, "top_k"), (4, -1.0, "top_k"), (4, 1.5, "top_k")):
    q = spec.copy()
    q[1, c] = bad
    expect(quiet(lambda: hook(specs=q)), "case 1: " + text)
expect(quiet(lambda: hook(planners=np.array([0, -1, 0, 0], np.int32))), "planner index")
assert quiet(lambda: lib.ltpl_fleet_sim_stats_eval(h, 0, *([None] * 6))) == 0
assert named(lambda: hook(off=(0, 1025, 3500))) == (0, 1, 1)                 # one launch over the 2 + 3 chunks, one merge launch for both cases
assert named(lambda: hook(off=(0, 0, 0), hole=1)) == (0, 1, 0)               # (no values: `values` may be null; no chunk, the merge alone)
assert named(lambda: hook(hole=2)) == (0, 1, 1)                              # (planner_idx may be null)
print("launches per tick: %d without a plan and with a plan without a period; %d more (k_fleet_sim_stats_chunk, k_fleet_sim_stats_merge) on the "
      "ticks of a period" % (plain, 2))
common.finish("sim stats args OK")
