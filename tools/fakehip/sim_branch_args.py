"""TEST TOOL: argument checks of ltpl_fleet_sim_snapshot / _snapshot_info / _snapshot_drop / ltpl_fleet_sim_branch (snapshot and branch of
the fleet simulation's planner state on the device) without a device. The library's host code built against the stand-in runtime without
sanitizers (FAKEHIP_SAN=none tools/fakehip/build.sh); kernels do nothing, so no copied state is looked at -- only the return codes, the
messages, what ``info`` reports and the number of kernel launches:
  - every refused call (null fleet, no simulation, slot out of range, empty slot, planner index out of range, a planner twice in a
    snapshot list, a destination twice, a source that is not in the snapshot, unequal opponent counts, a planner that is source and
    destination with the live fleet as source) returns LTPL_ERR_INVALID_ARG before any device allocation and launches nothing; so does
    n_pairs == 0, which returns LTPL_OK;
  - a pair src == dst with the live fleet as source is accepted (and skipped); ltpl_fleet_sim_setup empties every slot;
  - an allocation failing at each allocation of ltpl_fleet_sim_snapshot leaves the slot's previous content and ``info`` unchanged;
  - a tick of ltpl_fleet_sim_run launches the same kernels with and without snapshots held; a snapshot and a branch are one launch each;
  - with telemetry, the vehicle model, a tracker, a selector, a safety monitor and reactive opponents set together a branch (from the live
    fleet and from a snapshot) is four launches, each part kernel once, behind ONE allocation: failing, that allocation leaves nothing
    launched; a snapshot that fails at any of its allocations launches nothing and leaves the slot as it was."""
import ctypes

import numpy as np

import sim_args_common as common
from sim_args_common import _capi, expect, launches_out as launches, msg, quiet
from graphbasedlocaltrajectoryplanner_amd.fleet import SIM_SNAPSHOTS

N = 6
lib, fleet, table = common.start(N)
OPPONENTS = (1, 1, 0, 2, 1, 1)                                            # per planner: the offsets of planners 4 and 5 differ from 0 and 1
lib.ltpl_fleet_sim_snapshot.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32]
lib.ltpl_fleet_sim_snapshot_info.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
lib.ltpl_fleet_sim_snapshot_drop.argtypes = [ctypes.c_void_p, ctypes.c_int32]
lib.ltpl_fleet_sim_branch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
h = fleet.handle


def snapshot(slot, planners=None):
    if planners is None:
        return lib.ltpl_fleet_sim_snapshot(h, slot, None, 0), msg()
    idx = np.ascontiguousarray(np.asarray(list(planners) + [0], np.int32))                # (never a null pointer, an empty list included)
    return lib.ltpl_fleet_sim_snapshot(h, slot, idx.ctypes.data, len(planners)), msg()


def info(slot):
    n, b = ctypes.c_int32(-1), ctypes.c_uint64(0)
    idx = np.full(N, -1, np.int32)
    rc = lib.ltpl_fleet_sim_snapshot_info(h, slot, ctypes.byref(n), idx.ctypes.data, N, ctypes.byref(b))
    return rc, idx[:max(n.value, 0)].tolist(), b.value, msg()


def branch(slot, src, dst):
    s, d = np.ascontiguousarray(np.asarray(src, np.int32)), np.ascontiguousarray(np.asarray(dst, np.int32))
    ms = ctypes.c_float(-1.0)
    rc = lib.ltpl_fleet_sim_branch(h, slot, s.ctypes.data if s.size else None, d.ctypes.data if d.size else None, d.size, ctypes.byref(ms))
    return rc, msg()


def fresh():
    common.fresh([dict(common.GOOD_ENTRY, opponents=[(250.0 + 100.0 * k, 0.3, 5.0) for k in range(no)]) for no in OPPONENTS])


# null fleet, no simulation
assert lib.ltpl_fleet_sim_snapshot(None, 0, None, 0) == 1 and lib.ltpl_fleet_sim_snapshot_info(None, 0, None, None, 0, None) == 1
assert lib.ltpl_fleet_sim_snapshot_drop(None, 0) == 1 and lib.ltpl_fleet_sim_branch(None, -1, None, None, 0, None) == 1
expect(quiet(lambda: snapshot(0)), "ltpl_fleet_sim_setup first")
expect(quiet(lambda: info(0)), "ltpl_fleet_sim_setup first")
assert quiet(lambda: lib.ltpl_fleet_sim_snapshot_drop(h, 0)) == 1 and "ltpl_fleet_sim_setup first" in msg()
expect(quiet(lambda: branch(-1, [0], [1])), "ltpl_fleet_sim_setup first")

fresh()
plain = launches(lambda: fleet.sim_run(1, trace=False))[0]
# slots
for slot in (-1, SIM_SNAPSHOTS, 1 << 20):
    expect(quiet(lambda: snapshot(slot)), "out of range")
    expect(quiet(lambda: info(slot)), "out of range")
    assert quiet(lambda: lib.ltpl_fleet_sim_snapshot_drop(h, slot)) == 1 and "out of range" in msg()
for slot in (-2, SIM_SNAPSHOTS):
    expect(quiet(lambda: branch(slot, [0], [1])), "out of range")
for slot in range(SIM_SNAPSHOTS):
    assert quiet(lambda: info(slot))[:3] == (0, [], 0)
    assert quiet(lambda: lib.ltpl_fleet_sim_snapshot_drop(h, slot)) == 0                  # an empty slot: nothing to do
    expect(quiet(lambda: branch(slot, [0], [1])), "is empty")
assert fleet.sim_snapshot_info(3) is None
# planner lists of a snapshot
expect(quiet(lambda: snapshot(0, [0, N])), "out of range")
expect(quiet(lambda: snapshot(0, [-1])), "out of range")
expect(quiet(lambda: snapshot(0, [1, 4, 1])), "planner 1 is given twice")
expect(quiet(lambda: snapshot(0, [])), "1 .. n entries")
assert quiet(lambda: info(0))[:3] == (0, [], 0)

n_launch, rc = launches(lambda: snapshot(2, [4, 1, 3]))
assert rc[0] == 0 and n_launch == 1, (rc, n_launch)                                     # one launch: k_fleet_sim_branch
rc, planners, nbytes, _ = info(2)
assert rc == 0 and planners == [4, 1, 3] and nbytes > 3 * 200000, (rc, planners, nbytes)
assert fleet.sim_snapshot_info(2)["planners"].tolist() == [4, 1, 3] and fleet.sim_snapshot_info(2)["bytes"] == nbytes
small = np.zeros(2, np.int32)
assert quiet(lambda: lib.ltpl_fleet_sim_snapshot_info(h, 2, None, small.ctypes.data, 2, None)) == 1 and "planner buffer" in msg()
assert launches(lambda: snapshot(5))[0] == 1 and info(5)[1] == list(range(N)) and info(5)[2] > nbytes

# pairs of a branch
expect(quiet(lambda: branch(-1, [0, N], [1, 4])), "pair 1 (src %d, dst 4): planner index out of range" % N)
expect(quiet(lambda: branch(-1, [0], [-1])), "pair 0 (src 0, dst -1): planner index out of range")
expect(quiet(lambda: branch(2, [4, 1], [0, 0])), "pair 1 (src 1, dst 0): the destination is given twice")
expect(quiet(lambda: branch(2, [4, 0], [5, 1])), "pair 1 (src 0, dst 1): the source is not a planner of snapshot 2")
expect(quiet(lambda: branch(2, [4, 3], [0, 1])), "pair 1 (src 3, dst 1): the source has 2 opponents, the destination 1")
expect(quiet(lambda: branch(-1, [0, 1], [4, 2])), "pair 1 (src 1, dst 2): the source has 1 opponents, the destination 0")
expect(quiet(lambda: branch(-1, [0, 1], [1, 4])), "pair 1 (src 1, dst 4): with the live fleet as source no planner may be both")
expect(quiet(lambda: branch(-1, [0, 0], [0, 1])), "no planner may be both")              # (the identical pair excepts itself only)
null_rc = quiet(lambda: lib.ltpl_fleet_sim_branch(h, -1, None, None, 2, None))
assert null_rc == 1 and "src / dst missing" in msg()
expect(quiet(lambda: (lib.ltpl_fleet_sim_branch(h, -1, None, None, -1, None), msg())), "n_pairs must not be negative")
assert quiet(lambda: branch(-1, [], []))[0] == 0 and quiet(lambda: branch(2, [], []))[0] == 0     # n_pairs == 0: LTPL_OK, nothing done
assert quiet(lambda: branch(-1, [3, 0], [3, 0]))[0] == 0                                # src == dst on the live fleet: accepted, nothing to copy
n_launch, rc = launches(lambda: branch(-1, [3, 0, 0], [3, 1, 5]))                         # ... also next to real pairs (planner 5: another offset)
assert rc[0] == 0 and n_launch == 1, (rc, n_launch)
n_launch, rc = launches(lambda: branch(2, [4, 1, 3, 1], [0, 5, 3, 1]))                    # a snapshot's planner onto itself is a real copy
assert rc[0] == 0 and n_launch == 1, (rc, n_launch)
assert fleet.sim_branch(0, [1, 4, 5]) >= 0.0 and fleet.sim_branch(4, [0], snapshot=2) >= 0.0 and fleet.sim_restore(2) >= 0.0
try:
    fleet.sim_branch(0, [1], snapshot=2)
    raise AssertionError("a source outside the snapshot accepted")
except _capi.BackendError as e:
    assert "not a planner of snapshot 2" in str(e)

# a run launches what it launched before; the other settings keep the snapshots
assert launches(lambda: fleet.sim_run(1, trace=False))[0] == plain
fleet.sim_telemetry()
assert info(2)[1] == [4, 1, 3] and launches(lambda: branch(2, [4], [0]))[0] == 1          # (no telemetry part: the state alone)
with_tele = info(2)[2]
assert snapshot(2, [4, 1, 3])[0] == 0 and info(2)[2] > with_tele                          # taken with telemetry on: the records as well
fleet.sim_record([0, 1], 4)
fleet.sim_vel(vel_max=50.0)
assert info(2)[1] == [4, 1, 3] and info(5)[1] == list(range(N))
fleet.sim_telemetry(radius=None)
fleet.sim_record(None)
assert lib.ltpl_fleet_sim_snapshot_drop(h, 5) == 0 and info(5)[:3] == (0, [], 0) and info(2)[1] == [4, 1, 3]
fresh()                                                                                   # sim_setup empties every slot
assert all(info(slot)[:3] == (0, [], 0) for slot in range(SIM_SNAPSHOTS))
expect(quiet(lambda: branch(2, [4], [0])), "is empty")
assert snapshot(7)[0] == 0
fleet.sim_race([2, 4])                                                                    # (races are set before the first run)
assert info(7)[1] == list(range(N)) and branch(7, [0], [4])[0] == 0
fresh()
assert launches(lambda: fleet.sim_run(1, trace=False))[0] == plain

# an allocation failing at each allocation of ltpl_fleet_sim_snapshot: the slot keeps what it held
for tele in (False, True):
    def slot_1_taken():
        fresh()
        if tele:
            fleet.sim_telemetry()
        assert snapshot(1, [5, 0])[0] == 0
        return info(1)[:3]

    def slot_1_kept(k, held):
        assert info(1)[:3] == held and branch(1, [5], [4])[0] == 0, (k, info(1))

    def slot_1_new():
        assert info(1)[1] == [1, 2, 3]
    failures = common.alloc_sweep("ltpl_fleet_sim_snapshot", lambda: snapshot(1, [1, 2, 3]), 40, slot_1_kept, before=slot_1_taken, after_success=slot_1_new)
    assert failures >= (16 if tele else 13), failures
    print("allocation failure at each of the %d allocations of ltpl_fleet_sim_snapshot (telemetry %s): previous snapshot kept" % (
        failures, "on" if tele else "off"))
# ... and of ltpl_fleet_sim_branch (the pairs' entries): LTPL_ERR_HIP, nothing launched
fresh()
lib.fakehip_fail_malloc_after(1)
n_launch, rc = launches(lambda: branch(-1, [0], [1]))
lib.fakehip_fail_malloc_after(0)
assert rc[0] == 3 and "hipMalloc" in rc[1] and n_launch == 0, (rc, n_launch)

# telemetry, the vehicle model, a tracker, a selector, a safety monitor and reactive opponents set together: a branch is ONE allocation
# (the pairs' entries, in front of the first launch) and four launches, each part kernel once; a failing call launches nothing
BULK = b"_Z18k_fleet_sim_branchILb"                                                       # (either store form; 18: not the part kernels)
PARTS = (b"_Z25k_fleet_sim_branch_staged", b"_Z25k_fleet_sim_branch_safety", b"_Z24k_fleet_sim_branch_react")


def all_models():
    fresh()
    fleet.sim_telemetry()
    fleet.sim_vehicle()
    fleet.sim_tracker()
    fleet.sim_selector()
    fleet.sim_safety()
    fleet.sim_react()
    fleet.sim_run(1, trace=False)                                                         # (the staging holds a list)


def by_kernel(fn):
    """(launches during ``fn``, those of the bulk kernel, those of each part kernel, what ``fn`` returned)"""
    before = [lib.fakehip_launches_of(k) for k in (BULK,) + PARTS]
    n, out = launches(fn)
    return n, [lib.fakehip_launches_of(k) - b for k, b in zip((BULK,) + PARTS, before)], out


def armed(k, fn):
    """``fn`` with the k-th allocation from now on failing: (launches, what ``fn`` returned, the failure is still pending afterwards)"""
    lib.fakehip_fail_malloc_after(k)
    try:
        n, out = launches(fn)
    finally:
        p = ctypes.c_void_p()
        pending = lib.hipMalloc(ctypes.byref(p), 8) != 0
        if not pending:
            lib.hipFree(p)
        lib.fakehip_fail_malloc_after(0)
    return n, out, pending


all_models()
assert snapshot(3)[0] == 0
for slot, src, dst, what in ((-1, [0, 4], [1, 5], "the live fleet"), (3, [0, 4, 3], [1, 5, 3], "a snapshot")):
    n_launch, per_kernel, rc = by_kernel(lambda: branch(slot, src, dst))
    assert rc[0] == 0 and n_launch == 4 and per_kernel == [1, 1, 1, 1], (what, rc, n_launch, per_kernel)
    n_launch, rc, _ = armed(1, lambda: branch(slot, src, dst))
    assert rc[0] == 3 and "hipMalloc" in rc[1] and n_launch == 0, (what, rc, n_launch)
    n_launch, rc, pending = armed(2, lambda: branch(slot, src, dst))
    assert rc[0] == 0 and n_launch == 4 and pending, (what, rc, n_launch, pending)      # the call allocates once
    print("every model set, a branch from %s: 4 launches, each part kernel once, 1 allocation in front of them" % what)


def slot_1_taken_all():
    all_models()
    assert snapshot(1, [5, 0])[0] == 0
    return info(1)[:3], lib.fakehip_launch_count()


def slot_1_kept_all(k, ctx):
    held, count = ctx
    assert lib.fakehip_launch_count() == count, (k, "a failing snapshot launched")
    assert info(1)[:3] == held and branch(1, [5], [4])[0] == 0, (k, info(1))


def slot_1_new_all():
    assert info(1)[1] == [1, 2, 3]


failures = common.alloc_sweep("ltpl_fleet_sim_snapshot", lambda: snapshot(1, [1, 2, 3]), 40, slot_1_kept_all, before=slot_1_taken_all,
                              after_success=slot_1_new_all)
assert failures >= 16, failures
n_launch, per_kernel, rc = by_kernel(lambda: snapshot(1, [1, 2, 3]))
assert rc[0] == 0 and n_launch == 4 and per_kernel == [1, 1, 1, 1], (rc, n_launch, per_kernel)
print("every model set: allocation failure at each of the %d allocations of ltpl_fleet_sim_snapshot: nothing launched, the slot as it was" % failures)
print("launches per tick: %d with and without snapshots; a snapshot and a branch: 1 launch each" % plain)
common.finish("sim branch args OK")
