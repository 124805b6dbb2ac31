"""TEST TOOL: argument checks of ltpl_fleet_sim_noise / ltpl_fleet_sim_estimate / ltpl_fleet_sim_noise_draws (seeded sensor noise of the
fleet simulation) without a device. The library's host code built against the stand-in runtime without sanitizers (FAKEHIP_SAN=none
tools/fakehip/build.sh); kernels do nothing, so no draw is looked at -- only the return codes, the messages, the estimate's copies and the
number of kernel launches:
  - every refused call (null fleet, no simulation, a negative / NaN / infinite sigma, a missing seed array, a negative tick0; null or
    negative arguments of the draws) returns LTPL_ERR_INVALID_ARG before any device allocation and launches nothing;
  - a tick of ltpl_fleet_sim_run launches the same NUMBER of kernels with the noise on, off and never set, with and without races and
    telemetry (the noisy forms replace k_fleet_sim_step / k_fleet_sim_mates, nothing is added);
  - the estimate is the true state while the noise is off and until the first noisy tick;
  - an allocation failing at each allocation of ltpl_fleet_sim_noise is LTPL_ERR_HIP, and the fleet runs on."""
import ctypes

import numpy as np

import sim_args_common as common
from sim_args_common import expect, launches, msg, quiet
from graphbasedlocaltrajectoryplanner_amd.fleet import SimNoiseIn

N = 4
lib, fleet, table = common.start(N)
lib.ltpl_fleet_sim_noise.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.ltpl_fleet_sim_estimate.argtypes = [ctypes.c_void_p] * 4
lib.ltpl_fleet_sim_noise_draws.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
h = fleet.handle


def noise(seed=True, tick0=0, **sig):
    keep = [np.arange(N, dtype=np.uint64)]
    ni = SimNoiseIn()
    ni.seed, ni.tick0 = keep[0].ctypes.data if seed else None, tick0
    for k, v in sig.items():
        keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (N,))))
        setattr(ni, "sigma_" + k, keep[-1].ctypes.data)
    return lib.ltpl_fleet_sim_noise(h, ctypes.byref(ni)), msg()


POS = [(10.0 + p, -3.0 * p) for p in range(N)]


def fresh():
    common.fresh(common.moving_entries(N, static=[(1.0, 2.0, 0.0, 0.0, 4.0)]))


def estimate_is_truth():
    st, est = fleet.sim_state(), fleet.sim_estimate()
    assert np.array_equal(est["pos_est"], st["pos_est"]) and np.array_equal(est["vel_est"], st["vel_est"])
    assert np.array_equal(est["pos_est"], np.array(POS)) and np.array_equal(est["vel_est"], 1.5 * np.arange(N))


# null fleet, no simulation
assert lib.ltpl_fleet_sim_noise(None, None) == 1 and lib.ltpl_fleet_sim_estimate(None, None, None, None) == 1
assert lib.ltpl_fleet_sim_noise_draws(None, None, None, None, None, 0, None, None) == 1
expect(quiet(lambda: noise(pos=0.1)), "ltpl_fleet_sim_setup first")
expect(quiet(lambda: (lib.ltpl_fleet_sim_noise(h, None), msg())), "ltpl_fleet_sim_setup first")
expect(quiet(lambda: (lib.ltpl_fleet_sim_estimate(h, None, None, None), msg())), "ltpl_fleet_sim_setup first")

fresh()
estimate_is_truth()
plain = launches(lambda: fleet.sim_run(1, trace=False))
fresh()
for name in ("pos", "vel", "obj_pos", "obj_theta", "obj_vel"):
    for bad in (-0.5, np.nan, np.inf, [0.0, 0.0, 0.0, -1e-300]):
        expect(quiet(lambda: noise(**{name: bad})), "a sigma must be finite and not negative")
expect(quiet(lambda: noise(tick0=-1, pos=0.1)), "tick0 must not be negative")
expect(quiet(lambda: noise(seed=False, pos=0.1)), "seed missing")
assert quiet(lambda: lib.ltpl_fleet_sim_noise(h, None)) == 0               # switching off what is off: nothing to do
assert noise(pos=0.0, obj_vel=-0.0)[0] == 0                                 # zeros (and -0.0) are sigmas
assert noise()[0] == 0                                                      # every sigma array NULL: all zero
assert noise(tick0=2 ** 31 - 1, pos=0.1, vel=0.2, obj_pos=0.3, obj_theta=0.02, obj_vel=0.5)[0] == 0
estimate_is_truth()                                                          # until the first noisy tick
assert launches(lambda: fleet.sim_run(2, trace=False)) == 2 * plain          # (the tick counter wraps past 2^31 - 1 as an unsigned word)
fleet.sim_noise(None)
assert launches(lambda: fleet.sim_run(1, trace=False)) == plain

# races and telemetry: the same number of launches with and without noise
fresh()
fleet.sim_race([1, 3])
fleet.sim_telemetry()
with_mates = launches(lambda: fleet.sim_run(1, trace=False))
assert with_mates == plain + 3                                               # mates, telemetry, rank
fleet.sim_noise(seed=5, pos=0.1, obj_pos=0.3)
assert launches(lambda: fleet.sim_run(1, trace=False)) == with_mates
fresh()                                                                      # sim_setup switches the noise off
estimate_is_truth()
assert launches(lambda: fleet.sim_run(1, trace=False)) == plain

# an allocation failing at each allocation of ltpl_fleet_sim_noise
fresh()
assert noise(pos=0.1)[0] == 0
def runs_on(k, _):
    assert launches(lambda: fleet.sim_run(1, trace=False)) == plain


failures = common.alloc_sweep("ltpl_fleet_sim_noise", lambda: noise(pos=0.2, tick0=7), 10, runs_on)
assert failures == 2, failures
print("allocation failure at each of the %d allocations of ltpl_fleet_sim_noise: the fleet runs on" % failures)

# the draws
z = np.zeros(4, np.uint64)
g = np.zeros(4)
a = z.ctypes.data
expect(quiet(lambda: (lib.ltpl_fleet_sim_noise_draws(h, a, a, a, a, -1, g.ctypes.data, None), msg())), "n must not be negative")
for hole in range(5):
    args = [a, a, a, a, g.ctypes.data]
    args[hole] = None
    expect(quiet(lambda: (lib.ltpl_fleet_sim_noise_draws(h, args[0], args[1], args[2], args[3], 2, args[4], None), msg())), "missing")
assert quiet(lambda: lib.ltpl_fleet_sim_noise_draws(h, None, None, None, None, 0, None, None)) == 0
assert launches(lambda: fleet.sim_noise_draws(z, 0, 0, 0)) == 1 and launches(lambda: fleet.sim_noise_draws(z, 0, 0, 0, words=True)) == 1
print("launches per tick: %d with the noise on, off and never set (%d with races and telemetry)" % (plain, with_mates))
common.finish("sim noise args OK")
