"""TEST TOOL: what the ``*_args.py`` scripts of this directory share. ``start(n)`` loads the library's host code built against the stand-in
runtime (FAKEHIP_SAN=none tools/fakehip/build.sh), declares the stand-in's counters and makes a fleet of ``n`` planners on the Monteblanco
lattice; the helpers below then look at what a call did without a device: whether it allocated, how many kernels it launched (by number
and, through fakehip_launches_of, by name), its status and its message."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from graphbasedlocaltrajectoryplanner_amd import _capi, sim               # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet              # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.lattice import Lattice          # noqa: E402

INVALID, HIP_ERR, CAPACITY, UNSUPPORTED = 1, 3, 4, 5      # LTPL_ERR_INVALID_ARG, LTPL_ERR_HIP, LTPL_ERR_CAPACITY, LTPL_ERR_UNSUPPORTED
P, I32 = ctypes.c_void_p, ctypes.c_int32
GOOD_ENTRY = dict(opponents=[(250.0, 0.3, 5.0)], pref=("right", "straight"), pos_est=(0.0, 0.0), zone_gids=[3])

hip = lib = fleet = table = None
n_planners = 0
h = None                                  # the handle msg() reads: the fleet's, unless use_handle names another


def start(n, build="build_plain"):
    """The backend on ``tools/fakehip/<build>/libltpl_hip_fake.so``, a fleet of ``n`` planners and the race-line table: (lib, fleet, table)."""
    global hip, lib, fleet, table, n_planners
    n_planners = n
    lat = Lattice.load(os.path.join(ROOT, "tests", "golden", "monteblanco_lattice.npz"))
    table = sim.RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))
    hip = _capi.HipBackend(lat, lib_path=os.path.join(ROOT, "tools", "fakehip", build, "libltpl_hip_fake.so"))
    lib = hip.lib
    lib.fakehip_launch_count.restype = ctypes.c_long
    lib.fakehip_launches_of.restype = ctypes.c_long
    lib.fakehip_launches_of.argtypes = [ctypes.c_char_p]
    lib.fakehip_fail_malloc_after.argtypes = [ctypes.c_long]
    lib.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    lib.hipFree.argtypes = [P]
    lib.ltpl_fleet_last_error.restype = ctypes.c_char_p
    lib.ltpl_fleet_last_error.argtypes = [P]
    fleet = Fleet(hip, n)
    use_handle(fleet.handle)
    return lib, fleet, table


def use_handle(handle):
    global h
    h = handle


def finish(ok_line):
    fleet.close()
    hip.close()
    print(ok_line)


def quiet(fn, may_launch=False):
    """Runs ``fn`` with an allocation failure armed for the next hipMalloc; asserts that ``fn`` neither allocated (the failure is still
    pending afterwards) nor, unless ``may_launch``, launched. Returns ``fn``'s result."""
    before = lib.fakehip_launch_count()
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
    assert may_launch or lib.fakehip_launch_count() == before, "a refused call launched a kernel"
    return out


def no_allocation(fn):
    """``quiet`` without the look at the launches."""
    return quiet(fn, may_launch=True)


def msg():
    return (lib.ltpl_fleet_last_error(h) or b"").decode()


def expect(rc_msg, *want, code=INVALID):
    """``rc_msg``: (status, ..., message) of a refused call. ``want``: the texts the message has to hold; an int among them is the status
    in ``code``'s place."""
    rc, m = rc_msg[0], rc_msg[-1]
    code, texts = ([w for w in want if isinstance(w, int)] + [code])[0], [w for w in want if not isinstance(w, int)]
    assert rc == code and all(t in m for t in texts), (rc_msg, want)
    print("refused (%d): %s" % (rc, m))


def launches(fn):
    """Kernel launches during ``fn``."""
    before = lib.fakehip_launch_count()
    fn()
    return lib.fakehip_launch_count() - before


def launches_out(fn):
    """(kernel launches during ``fn``, what ``fn`` returned)."""
    before = lib.fakehip_launch_count()
    out = fn()
    return lib.fakehip_launch_count() - before, out


def named(fn, name):
    """Launches during ``fn`` of the kernels whose mangled name holds ``name``."""
    a = lib.fakehip_launches_of(name)
    fn()
    return lib.fakehip_launches_of(name) - a


def run1():
    fleet.sim_run(1, trace=False)


def launches_per_tick(n=1):
    return launches(lambda: fleet.sim_run(n, trace=False)) // n


def fresh(entries=None, **vel):
    """ltpl_fleet_sim_setup (which switches every model off) and ltpl_fleet_sim_vel; by default one slow opponent per planner."""
    fleet.sim_setup(table, [GOOD_ENTRY] * n_planners if entries is None else entries)
    fleet.sim_vel(**vel)


def moving_entries(n, **over):
    """One opponent each, planners apart from one another and at different speeds."""
    return [dict(dict(opponents=[(250.0, 0.3, 5.0)], static=[], pref=("right", "straight"), pos_est=(10.0 + p, -3.0 * p), vel_est=1.5 * p,
                      zone_gids=[]), **over) for p in range(n)]


def alloc_sweep(what, call, bound, after_failure, before=None, after_success=None):
    """An allocation failing at the k-th hipMalloc of ``call`` (which returns (status, ..., message)) for k = 1, 2, ... below ``bound``,
    until the call succeeds. Every failure has to be LTPL_ERR_HIP with hipMalloc in its message; ``after_failure(k, ctx)`` then asserts
    what the script expects of the state the call left, ``ctx`` being what ``before()`` returned in front of the call. Returns the number
    of failures, that is of allocations of a successful ``call``."""
    failures = 0
    for k in range(1, bound):
        ctx = before() if before else None
        lib.fakehip_fail_malloc_after(k)
        out = call()
        lib.fakehip_fail_malloc_after(0)
        rc, m = out[0], out[-1]
        if rc == 0:
            if after_success:
                after_success()
            return failures
        assert rc == HIP_ERR and "hipMalloc" in m, (what, k, rc, m)
        failures += 1
        after_failure(k, ctx)
    raise AssertionError("%s never succeeded" % what)
