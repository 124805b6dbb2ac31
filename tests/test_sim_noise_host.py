"""
CPU: the seeded sensor noise of the fleet's simulation (ltpl_fleet_sim_noise) off the device --

  1. sim.philox4x32 reproduces the three published known answers of Philox4x32-10;
  2. csrc/fleet_noise.hpp, compiled with the host compiler, equals the Python mirror bit for bit: words, sample and perturbation on the
     tuples of sim_noise_util.draw_tuples (seed 0 and 2^64 - 1, tick 0 and 2^31 - 1, all three obj ranges);
  3. moments of 65 536 samples of a fixed seed: |mean| < 0.02, |var - 1| < 0.03 -- five standard errors (1 / 256 for the mean;
     sqrt(1.9 / n) for the variance with the sum's kurtosis of 2.9); the samples are deterministic;
  4. neighbouring ticks, objects and components are uncorrelated (|r| < 0.02: five standard errors of 1 / 256) and every |g| < 6;
  5. the noisy host loop (sim_noise_util.NoisySimLoop) with all sigmas 0 equals HostSimLoop exactly; with the sigmas of the issue it runs
     200 ticks on Monteblanco behind an opponent without a failure and plans differently from the noise-free run.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import sim_noise_util as nu
from graphbasedlocaltrajectoryplanner_amd import sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        assert tuple(int(v) for v in sim.philox4x32(ctr, key)) == out
    # arrays: the three vectors in one call
    got = sim.philox4x32([np.array([k[0][i] for k in kat]) for i in range(4)], [np.array([k[1][i] for k in kat]) for i in range(2)])
    assert np.array_equal(np.stack(got, axis=1), np.array([k[2] for k in kat], np.uint32))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("noise") / "sim_noise_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "sim_noise_shim.cpp")],
                   check=True)
    lib = ctypes.CDLL(so)
    P = ctypes.c_void_p
    lib.noise_draws_host.argtypes = [P, P, P, P, ctypes.c_int, P, P]
    lib.philox_host.argtypes = [P, P, P]
    lib.noise_add_host.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]
    lib.noise_add_host.restype = ctypes.c_double
    return lib


def test_header_equals_the_mirror_bit_for_bit(shim):
    ctr, key, out = np.array([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], np.uint32), np.array([0xa4093822, 0x299f31d0], np.uint32), np.zeros(4, np.uint32)
    shim.philox_host(ctr.ctypes.data, key.ctypes.data, out.ctypes.data)
    assert out.tolist() == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    seed, tick, obj, comp = (np.ascontiguousarray(a) for a in nu.draw_tuples())
    n = seed.size
    assert n >= 4000 and {0, 2 ** 64 - 1} <= set(seed.tolist()) and {0, 2 ** 31 - 1} <= set(tick.tolist())
    assert np.any(obj == sim.NOISE_EGO) and np.any(obj < 96) and np.any((obj >= sim.NOISE_MATE) & (obj < sim.NOISE_MATE + 96))
    g, words = np.zeros(n), np.zeros((n, 12), np.uint32)
    shim.noise_draws_host(seed.ctypes.data, tick.ctypes.data, obj.ctypes.data, comp.ctypes.data, n, g.ctypes.data, words.ctypes.data)
    assert np.array_equal(words, sim.noise_words(seed, tick, obj, comp))
    ref = sim.noise_gauss(seed, tick, obj, comp)
    assert np.array_equal(g.view(np.uint64), ref.view(np.uint64))
    # scalars take the same path as arrays
    for i in (0, 1, n // 2, n - 1):
        assert sim.noise_gauss(int(seed[i]), int(tick[i]), int(obj[i]), int(comp[i])) == g[i]
    # the perturbation: one multiply and one add; sigma 0 hands the value through (negative speeds and -0.0 included); speeds clamp at 0
    nm = sim.NoiseModel(1, 77, pos=0.25, vel=3.0)
    for k in range(200):
        v = (-1.0, 0.3, 1234.56789)[k % 3]
        (ex, ey), ev = nm.ego(0, k, (v, -v), v)
        assert ex == shim.noise_add_host(v, 0.25, 77, k, sim.NOISE_EGO, 0, 0) and ey == shim.noise_add_host(-v, 0.25, 77, k, sim.NOISE_EGO, 1, 0)
        assert ev == shim.noise_add_host(v, 3.0, 77, k, sim.NOISE_EGO, 2, 1) and ev >= 0.0
    assert any(nm.ego(0, k, (0.0, 0.0), 0.3)[1] == 0.0 for k in range(200))       # (the clamp is reached)
    for v in (-2.5, -0.0, 7.0):
        got = shim.noise_add_host(v, 0.0, 77, 3, 0, 3, 1)
        assert got == v and np.signbit(got) == np.signbit(v)
    assert sim.NoiseModel(1, 77).ego(0, 3, (1.5, -0.0), -2.5) == ([1.5, -0.0], -2.5)


@pytest.fixture(scope="module")
def samples():
    return sim.noise_gauss(0x5EED5EED5EED, np.arange(65536), 0, 0)


def test_moments(samples):
    g = samples
    mean, var = float(np.mean(g)), float(np.var(g))
    print("mean %.6f var %.6f" % (mean, var))
    assert abs(mean) < 0.02 and abs(var - 1.0) < 0.03
    assert np.array_equal(g, sim.noise_gauss(0x5EED5EED5EED, np.arange(65536), 0, 0))


def test_independence_and_range(samples):
    n = 65536
    t = np.arange(n)

    def corr(a, b):
        return float(np.corrcoef(a, b)[0, 1])
    pairs = {"ticks": (samples[:-1], samples[1:]),
             "objects": (samples, sim.noise_gauss(0x5EED5EED5EED, t, 1, 0)),
             "components": (samples, sim.noise_gauss(0x5EED5EED5EED, t, 0, 1)),
             "ego / object 0": (samples, sim.noise_gauss(0x5EED5EED5EED, t, sim.NOISE_EGO, 0)),
             "object 0 / mate 0": (samples, sim.noise_gauss(0x5EED5EED5EED, t, sim.NOISE_MATE, 0)),
             "seeds": (samples, sim.noise_gauss(0x5EED5EED5EEE, t, 0, 0))}
    for name, (a, b) in pairs.items():
        r = corr(a, b)
        print(name, r)
        assert abs(r) < 0.02, (name, r)
        assert np.all(np.abs(b) < 6.0)
    assert np.all(np.abs(samples) < 6.0)
    # the extremes of the formula: K = 0 and K = 12 (2^32 - 1)
    assert (0.0 + 6.0) * 2.0 ** -32 - 6.0 > -6.0 and (12.0 * (2 ** 32 - 1) + 6.0) * 2.0 ** -32 - 6.0 < 6.0


# ---- the host loop ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    return sim.RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


def run_loop(lat, oracle, table, cls, start, ticks, noise=None):
    from oracle.planner_host import HostPlannerBackend
    pl = [HostPlannerBackend(lat).planner(1)]
    if noise is None:
        loop = sl.HostSimLoop(lat, table, [cls["entry"]], pl, oracle=oracle)
    else:
        loop = nu.NoisySimLoop(lat, table, [cls["entry"]], pl, oracle=oracle, noise=noise)
    assert loop.set_start(0, start['pos'], start['heading'], start['vel'], start['max_heading_offset'])[0]
    loop.sim_vel(**cls["vel"])
    return [loop.tick(want_paths=True)[0] for _ in range(ticks)]


@pytest.fixture(scope="module")
def one_class(table):
    start = pr.load_ticks("c2")[0]['start']
    track = np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz"))
    return sl.monteblanco_classes(table, track, tuple(start['pos']))["one"], start


@pytest.fixture(scope="module")
def plain_run(monteblanco, oracle_backend, table, one_class):
    return run_loop(monteblanco, oracle_backend, table, one_class[0], one_class[1], 200)


def same_tick(a, b):
    if a["failed"] or b["failed"]:
        return a["failed"] == b["failed"]
    if (a["sel"], a["now"], a["pos"], a["vel"], a["theta"], a["cnt"], a["opp_s"]) != (b["sel"], b["now"], b["pos"], b["vel"], b["theta"], b["cnt"], b["opp_s"]):
        return False
    if a["paths"]["nodes"] != b["paths"]["nodes"] or list(a["traj"][0]) != list(b["traj"][0]):
        return False
    return all(np.array_equal(a["traj"][0][k][0], b["traj"][0][k][0]) for k in a["traj"][0])


def test_noisy_loop_with_all_sigmas_zero_is_the_host_loop(monteblanco, oracle_backend, table, one_class, plain_run):
    recs = run_loop(monteblanco, oracle_backend, table, one_class[0], one_class[1], 60, noise=sim.NoiseModel(1, 42))
    for k, (a, b) in enumerate(zip(recs, plain_run)):
        assert same_tick(a, b), k
        assert a["est_pos"] == a["pos"] and a["est_vel"] == a["vel"] and a["objects"] == a["true_objects"]
    assert np.array_equal(np.array([sl.trace_rows([r]) for r in recs]), np.array([sl.trace_rows([r]) for r in plain_run[:60]]), equal_nan=True)


def test_noisy_loop_runs_200_ticks_and_plans_differently(monteblanco, oracle_backend, table, one_class, plain_run):
    recs = run_loop(monteblanco, oracle_backend, table, one_class[0], one_class[1], 200, noise=sim.NoiseModel(1, 42, **nu.SIGMAS))
    assert not any(r["failed"] for r in recs), [k for k, r in enumerate(recs) if r["failed"]][:3]
    assert all(r["est_pos"] != r["pos"] and r["objects"] != r["true_objects"] for r in recs)
    nodes = [k for k, (a, b) in enumerate(zip(recs, plain_run)) if a["paths"]["nodes"] != b["paths"]["nodes"]]
    vx = [k for k, (a, b) in enumerate(zip(recs, plain_run)) if list(a["traj"][0]) != list(b["traj"][0]) or
          any(not np.array_equal(a["traj"][0][key][0][:, 5], b["traj"][0][key][0][:, 5]) for key in a["traj"][0])]
    print("ticks whose node lists differ from the noise-free run: %d, whose vx differs: %d" % (len(nodes), len(vx)))
    assert nodes or vx


# ---- the entry points -------------------------------------------------------------------------------------------------------------------
def test_noise_entry_points_check_their_arguments_without_a_device():
    """tools/fakehip/sim_noise_args.py on the stand-in runtime (plain build): refused calls allocate and launch nothing, a tick launches
    the same number of kernels with the noise on, off and never set, the estimate is the true state until the first noisy tick."""
    import sys
    env = dict(os.environ, FAKEHIP_SAN="none", LTPL_NO_SELFTEST="1")
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "sim_noise_args.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and "sim noise args OK" in p.stdout, p.stdout[-3000:]
    assert "launches per tick" in p.stdout and "the fleet runs on" in p.stdout, p.stdout[-3000:]


def test_python_binding_and_header_declare_the_entry_points():
    from graphbasedlocaltrajectoryplanner_amd import fleet
    for name in ("sim_noise", "sim_estimate", "sim_noise_draws"):
        assert callable(getattr(fleet.Fleet, name)), name
    with open(os.path.join(ROOT, "include", "ltpl_hip.h")) as fh:
        hdr = fh.read()
    for name in ("ltpl_fleet_sim_noise(", "ltpl_fleet_sim_estimate(", "ltpl_fleet_sim_noise_draws(", "#define LTPL_ABI_VERSION 9"):
        assert name in hdr, name
    assert sim.NOISE_EGO == 0xFFFFFFFF and sim.NOISE_MATE == 0x80000000
