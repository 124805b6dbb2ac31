"""TEST TOOL: argument checks of ltpl_fleet_sim_predictor / ltpl_fleet_sim_predictor_read / ltpl_fleet_sim_predictor_eval (the prediction model
of the fleet simulation, csrc/fleet_predict.hpp) without a device. The library's host code built against the stand-in runtime without
sanitizers (FAKEHIP_SAN=none tools/fakehip/build.sh); kernels do nothing, so no decision is looked at -- only the return codes, the
messages and the kernel launches (by number and, through fakehip_launches_of, by name):
  - every refused call (null fleet, no simulation, n_points outside 1 .. 8, a missing array, a mode outside 0 .. 2, a horizon that is not
    finite and positive, relax outside [0, 1], a negative or NaN d_max; the read's record size; the hook's counts, arrays and parameters)
    returns LTPL_ERR_INVALID_ARG with a message that names the argument, before any device allocation, and launches nothing;
  - the capacity bound slots (1 + n_points) <= 192: exactly 192 is accepted, 193 and more are LTPL_ERR_CAPACITY, checked before anything
    is allocated; ltpl_fleet_sim_race is refused the same way, leaving everything as it was, when its slot counts break the bound;
  - a refused or failing call keeps the previous predictor (the tick still launches k_fleet_sim_predict, the records stay readable); an
    allocation failing at each allocation of the call is LTPL_ERR_HIP, and the fleet runs on;
  - per tick a fleet with the predictor set launches k_fleet_sim_predict and not k_fleet_sim_compact, the same number of kernels as
    before; a fleet that had one and cleared it, and one after ltpl_fleet_sim_setup, launch what a fleet that never had one launches."""
import ctypes

import numpy as np

import sim_args_common as common
from sim_args_common import CAPACITY as CAP, _capi, I32, INVALID, P, expect, launches, msg, quiet, run1, sim
from graphbasedlocaltrajectoryplanner_amd.fleet import SimPredictorIn

N = 4
lib, fleet, table = common.start(N)
lib.ltpl_fleet_sim_predictor.argtypes = [P, P]
lib.ltpl_fleet_sim_predictor_read.argtypes = [P, P, I32]
lib.ltpl_fleet_sim_predictor_eval.argtypes = [P, I32, I32] + [P] * 6
h = fleet.handle
GOOD = dict(mode=2, horizon=2.0, relax=0.25, d_max=6.0)


def predictor(n_points=4, missing=None, **par):
    keep = []
    pi = SimPredictorIn()
    pi.n_points = n_points
    for k, v in dict(GOOD, **par).items():
        keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32 if k == "mode" else np.float64), (N,))))
        setattr(pi, k, None if k == missing else keep[-1].ctypes.data)
    return lib.ltpl_fleet_sim_predictor(h, ctypes.byref(pi)), msg()


def named(fn):
    """(launches of k_fleet_sim_predict, of k_fleet_sim_compact) during ``fn``."""
    a = [lib.fakehip_launches_of(b"k_fleet_sim_predict"), lib.fakehip_launches_of(b"k_fleet_sim_compact")]
    fn()
    return lib.fakehip_launches_of(b"k_fleet_sim_predict") - a[0], lib.fakehip_launches_of(b"k_fleet_sim_compact") - a[1]


def fresh(opponents=(1, 1, 1, 1)):
    """``opponents``: opponents per planner (their staging slots before a race)."""
    entries = common.moving_entries(N)
    for p in range(N):
        entries[p]["opponents"] = [(250.0 + 5.0 * k, 0.3, 5.0) for k in range(opponents[p])]
    common.fresh(entries)


out = np.zeros((N, sim.PREDICTOR_DOUBLES))


def read(size=sim.PREDICTOR_DOUBLES, rec=True):
    return lib.ltpl_fleet_sim_predictor_read(h, out.ctypes.data if rec else None, size), msg()


# null fleet, no simulation
assert lib.ltpl_fleet_sim_predictor(None, None) == INVALID and lib.ltpl_fleet_sim_predictor_read(None, out.ctypes.data, 11) == INVALID
assert lib.ltpl_fleet_sim_predictor_eval(None, 0, 1, *([None] * 6)) == INVALID
expect(quiet(lambda: predictor()), "ltpl_fleet_sim_setup first")
expect(quiet(lambda: (lib.ltpl_fleet_sim_predictor(h, None), msg())), "ltpl_fleet_sim_setup first")
expect(quiet(read), "ltpl_fleet_sim_setup first")

fresh()
plain = launches(run1)
assert named(run1) == (0, 1)
expect(quiet(read), "the predictor is off")
assert quiet(lambda: lib.ltpl_fleet_sim_predictor(h, None)) == 0            # switching off what is off: nothing to do, nothing allocated


def refusals():
    for bad in (0, -1, 9, 1000):
        expect(quiet(lambda: predictor(n_points=bad)), "n_points")
    for name in sim.PREDICTOR_PARAMS:
        expect(quiet(lambda: predictor(missing=name)), name + " missing")
    for bad in (-1, 3, [0, 1, 2, 7]):
        expect(quiet(lambda: predictor(mode=bad)), "mode")
    for bad in (np.nan, 0.0, -1.0, np.inf, -np.inf, [1.0, 1.0, 1.0, -1e-300]):
        expect(quiet(lambda: predictor(horizon=bad)), "horizon")
    for bad in (np.nan, -0.1, 1.5, np.inf, [0.0, 0.0, float(np.nextafter(1.0, 2.0)), 0.0]):
        expect(quiet(lambda: predictor(relax=bad)), "relax")
    for bad in (np.nan, -1.0, -np.inf, [0.0, 0.0, 0.0, -5e-324]):
        expect(quiet(lambda: predictor(d_max=bad)), "d_max")


refusals()
# the edges that are arguments
assert predictor(n_points=1, mode=0, horizon=5e-324, relax=0.0, d_max=0.0)[0] == 0
assert predictor(n_points=8, mode=[0, 1, 2, 2], horizon=1e300, relax=1.0, d_max=np.inf)[0] == 0
with_pred = launches(run1)
assert with_pred == plain, (with_pred, plain)                                # one kernel in another's place
assert named(run1) == (1, 0)
assert read()[0] == 0
expect(quiet(lambda: read(size=10)), "record size")
expect(quiet(lambda: read(rec=False)), "out missing")
# a refused call keeps the previous predictor
refusals()
assert named(lambda: fleet.sim_run(2, trace=False)) == (2, 0) and read()[0] == 0
assert lib.ltpl_fleet_sim_predictor(h, None) == 0
assert launches(run1) == plain and named(run1) == (0, 1)                     # set, then cleared: what a fleet that never had one launches
expect(quiet(read), "the predictor is off")

# the capacity bound: slots (1 + K) <= 192 for every planner, checked before anything is allocated
fresh((96, 64, 24, 1))
assert predictor(n_points=1)[0] == 0                                         # 96 x 2 = 192: accepted
expect(quiet(lambda: predictor(n_points=2)), "above 192", code=CAP)          # 96 x 3 = 288
assert named(run1) == (1, 0) and read()[0] == 0                              # ... and the K = 1 predictor is still in force
fresh((64, 64, 24, 1))
assert predictor(n_points=2)[0] == 0                                         # 64 x 3 = 192
expect(quiet(lambda: predictor(n_points=3)), "above 192", code=CAP)          # 64 x 4 = 256
fresh((65, 1, 24, 1))
expect(quiet(lambda: predictor(n_points=2)), "planner 0", code=CAP)          # 65 x 3 = 195
fresh((1, 1, 24, 25))
expect(quiet(lambda: predictor(n_points=7)), "planner 3", code=CAP)          # 24 x 8 = 192 fits, 25 x 8 = 200 does not
fresh((1, 1, 24, 24))
assert predictor(n_points=7)[0] == 0                                         # 24 x 8 = 192
expect(quiet(lambda: predictor(n_points=8)), "planner 2", code=CAP)          # 24 x 9 = 216
fresh((1, 1, 24, 25))
expect(quiet(lambda: predictor(n_points=8)), "above 192", code=CAP)
expect(quiet(read), "the predictor is off")                                  # refused from the start: nothing was set

# races: the staging follows the new slot counts at the predictor's stride; a race that breaks the bound is refused and changes nothing
fresh((47, 47, 47, 1))
assert predictor(n_points=3)[0] == 0                                         # 47 x 4 = 188
fleet.sim_race([2, 2])                                                       # 48 x 4 = 192: accepted, the predictor stays
assert read()[0] == 0 and launches(run1) == plain + 1 and named(run1) == (1, 0)       # (the mates' kernel besides)
fresh((47, 47, 47, 1))
assert predictor(n_points=3)[0] == 0
try:
    quiet(lambda: fleet.sim_race([3, 1]))                                    # 49 x 4 = 196
    raise AssertionError("a race above the bound was accepted")
except _capi.BackendError as e:
    assert "above 192" in str(e), e
    print("refused: %s" % e)
assert launches(run1) == plain and named(run1) == (1, 0) and read()[0] == 0   # no mates kernel appeared: the races are what they were
fresh((47, 47, 47, 1))
fleet.sim_race([3, 1])                                                       # without the predictor the same race is fine ...
expect(quiet(lambda: predictor(n_points=3)), "planner 0", code=CAP)          # ... and the predictor is refused behind it

# telemetry, noise, sensor and tracker next to it: the same number of launches, whatever else runs
fresh()
fleet.sim_race([1, 3])
fleet.sim_telemetry()
fleet.sim_noise(seed=5, pos=0.1, obj_pos=0.3)
fleet.sim_sensor(range=100.0, fov_deg=120.0, occl=1.0, p_drop=0.1, seed=3)
fleet.sim_tracker()
busy = launches(run1)
fleet.sim_predictor(n_points=4)
assert launches(run1) == busy and named(run1) == (1, 0)
fresh()                                                                      # sim_setup switches the predictor off
assert launches(run1) == plain and named(run1) == (0, 1)
expect(quiet(read), "the predictor is off")

# an allocation failing at each allocation of ltpl_fleet_sim_predictor: setting, replacing and clearing
for what, call, ok_after in (("setting", lambda: predictor(n_points=2), (0, 1)), ("replacing", lambda: predictor(n_points=5, horizon=9.0), (1, 0)),
                             ("clearing", lambda: (lib.ltpl_fleet_sim_predictor(h, None), msg()), (1, 0))):
    def still(k, _):
        assert launches(run1) == plain and named(run1) == ok_after, (what, k)        # the previous state: still off / still the old predictor
        assert (read()[0] == 0) == (ok_after == (1, 0)), (what, k)
    failures = common.alloc_sweep("ltpl_fleet_sim_predictor", call, 40, still)
    assert failures == (14 if what == "clearing" else 16), (what, failures)
    print("%s: allocation failure at each of the %d allocations of ltpl_fleet_sim_predictor: the fleet runs on" % (what, failures))
assert named(run1) == (0, 1)

# the hook
M = 2
par = np.tile(np.array([2.0, 2.0, 0.5, 6.0]), (M, 1))
objs, pts, oc, rec = np.zeros((200, 5)), np.zeros((200, 9, 2)), np.zeros(200, np.int32), np.zeros((M, sim.PREDICTOR_DOUBLES))


def hook(n=M, K=4, off=(0, 1, 2), hole=None, params=par):
    o = np.array(off, np.int32)
    args = [params.ctypes.data, o.ctypes.data, objs.ctypes.data, pts.ctypes.data, oc.ctypes.data, rec.ctypes.data]
    if hole is not None:
        args[hole] = None
    return lib.ltpl_fleet_sim_predictor_eval(h, n, K, *args), msg()


expect(quiet(lambda: hook(n=-1)), "n_cases")
for bad in (0, 9):
    expect(quiet(lambda: hook(K=bad)), "n_points")
for hole in range(6):
    expect(quiet(lambda: hook(hole=hole)), "missing")
expect(quiet(lambda: hook(off=(1, 2, 3))), "start at 0")
expect(quiet(lambda: hook(off=(0, 97, 98))), "0 .. 96 objects")
expect(quiet(lambda: hook(off=(0, 3, 2))), "0 .. 96 objects")
for c, bad, text in ((0, 3.0, "mode"), (0, 0.5, "mode"), (1, 0.0, "horizon"), (1, np.nan, "horizon"), (2, 1.5, "relax"), (3, -1.0, "d_max")):
    q = par.copy()
    q[1, c] = bad
    expect(quiet(lambda: hook(params=q)), "case 1: " + text)
assert quiet(lambda: lib.ltpl_fleet_sim_predictor_eval(h, 0, 1, *([None] * 6))) == 0
assert launches(lambda: hook(off=(0, 96, 192))) == 1 and launches(lambda: hook(off=(0, 0, 0), hole=2)) == 1
print("launches per tick: %d without the predictor, %d with it (k_fleet_sim_predict in k_fleet_sim_compact's place); %d with races, telemetry, "
      "noise, sensor and tracker, with and without it" % (plain, with_pred, busy))
common.finish("sim predictor args OK")
