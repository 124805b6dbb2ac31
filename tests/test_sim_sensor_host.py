"""
CPU: the sensor model of the fleet's simulation (ltpl_fleet_sim_sensor) off the device --

  1. csrc/fleet_sensor.hpp, compiled alone with the host compiler (-ffp-contract=off), equals the Python mirror sim.SensorModel bit for bit
     on the cases of sim_sensor_util.cases: every decision boundary straddled with nextafter steps (both outcomes must occur on every
     straddle), the constructed scenes of the rule (chain, lost occluders, near field, the order of the causes), seeded scenes with 0, 1,
     63, 64, 65 and 96 objects and losses on both sides of slot 64; the mirror is the arbiter;
  2. the constructed scenes give the causes the rule states;
  3. dropout: the published Philox known answers give u; p_drop = 0 draws nothing; over 65 536 draws the dropped share lies within five
     standard errors of p_drop; counter word 3 separates the block from every block of noise_gauss under the same seed, tick and object;
  4. SensorSimLoop with the open sensor equals HostSimLoop record for record over 200 ticks on the Monteblanco scenario classes;
  5. a closed loop with a car hidden behind another and a forward cone: all four causes occur, the planner's actions differ from the
     all-seeing run, blind_clear_min is finite;
  6. on every scenario of the device differential (sim_sensor_util.scenarios) no object lies within 1e-9 sqrt(L2) of the cone's boundary
     in any tick: the device's sin / cos against libm's cannot change a decision there;
  7. the entry points check their arguments without a device.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import sim_sensor_util as su
from graphbasedlocaltrajectoryplanner_amd import sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sensor") / "sim_sensor_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                    os.path.join(ROOT, "tests", "sim_sensor_shim.cpp")], check=True)
    lib = ctypes.CDLL(so)
    D, P = ctypes.c_double, ctypes.c_void_p
    lib.sensor_eval_host.argtypes = [D, D, D, D, P, ctypes.c_uint64, ctypes.c_uint32, P, ctypes.c_int, P, P, P]
    lib.sensor_uniform_host.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, P]
    lib.sensor_uniform_host.restype = D
    lib.noise_words_host.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, P]
    return lib


def header(shim, c):
    """(causes, u, clearances) of a case by the compiled header."""
    n = len(c["objs"])
    o = np.ascontiguousarray(np.array(c["objs"] or [(0.0, 0.0, 0.0)], float))
    par = np.array(c["params"], float)
    cause, u, clear = np.zeros(n + 1, np.int32), np.zeros(n + 1), np.zeros(n + 1)
    shim.sensor_eval_host(c["pose"][0], c["pose"][1], c["f"][0], c["f"][1], par.ctypes.data, c["seed"], c["tick"], o.ctypes.data, n,
                          cause.ctypes.data, u.ctypes.data, clear.ctypes.data)
    return cause[:n].tolist(), u[:n], clear[:n]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


# ---- 1. header against mirror -------------------------------------------------------------------------------------------------------------
def test_header_equals_the_mirror_bit_for_bit_and_every_boundary_is_straddled(shim):
    cs, groups = su.cases()
    counts, causes, lost_low, lost_high, drawn = set(), [], 0, 0, 0
    for i, c in enumerate(cs):
        hc, hu, hclear = header(shim, c)
        mc, mu = su.mirror(c)
        assert hc == mc, "case %d: header %s, mirror %s" % (i, hc, mc)
        assert np.array_equal(bits(hu), bits(mu)), "case %d: u" % i
        for (x, y, r), cl in zip(c["objs"], hclear):
            dx, dy = x - c["pose"][0], y - c["pose"][1]
            assert cl == math.sqrt(dx * dx + dy * dy) - r, i
        # a draw is made exactly where the object reached test 5
        assert [not math.isnan(v) for v in mu] == [c["params"][4] > 0.0 and k in (sim.SENSOR_SEEN, sim.SENSOR_DROP) for k in mc], i
        causes.append(mc)
        counts.add(len(mc))
        drawn += sum(not math.isnan(v) for v in mu)
        if len(mc) > 64:
            lost_low += sum(k != 0 for k in mc[:64])
            lost_high += sum(k != 0 for k in mc[64:])
    su.check_straddles(cs, groups, causes)
    assert len(groups) >= 16 and {0, 1, 63, 64, 65, 96} <= counts
    assert lost_low > 0 and lost_high > 0 and drawn > 500
    assert {k for mc in causes for k in mc} == {0, 1, 2, 3, 4}


# ---- 2. the rule on constructed scenes ----------------------------------------------------------------------------------------------------
def causes_of(objs, **par):
    return su.mirror(su.case(objs, **par))[0]


def test_the_rule_on_constructed_scenes():
    S, R, F, O, D = sim.SENSOR_SEEN, sim.SENSOR_RANGE, sim.SENSOR_FOV, sim.SENSOR_OCCL, sim.SENSOR_DROP
    # range at equality is seen; +inf keeps an overflowing L2
    assert causes_of([(0.0, 10.0, 1.0)], range=10.0) == [S] and causes_of([(0.0, 10.0, 1.0)], range=su.down(10.0)) == [R]
    assert causes_of([(0.0, 1e300, 1.0)], range=su.INF) == [S]
    # the cone: exactly abeam with fov_cos = 0 is seen, the smallest step behind is not; -1 switches the test off
    assert causes_of([(5.0, 0.0, 1.0)], fov_cos=0.0) == [S] and causes_of([(5.0, -5e-324, 1.0)], fov_cos=0.0) == [F]
    assert causes_of([(0.0, -5.0, 1.0)], fov_cos=-1.0) == [S] and causes_of([(0.0, -5.0, 1.0)], fov_cos=su.up(-1.0)) == [F]
    # an object at the pose itself lies in every near field
    assert causes_of([(3.0, -4.0, 1.0)], pose=(3.0, -4.0), fov_cos=0.9, occl=1.0, range=0.0) == [S]
    # occlusion: 625 <= 625 hides, one ulp out does not; equal distances and identical positions never hide; d_j . d_k = 0 does not hide
    assert causes_of([(0.0, 10.0, 1.0), (2.5, 5.0, 2.5)], occl=1.0) == [O, S]
    assert causes_of([(0.0, 10.0, 1.0), (su.up(2.5), 5.0, 2.5)], occl=1.0) == [S, S]
    assert causes_of([(3.0, 4.0, 9.0), (4.0, 3.0, 9.0)], occl=1.0) == [S, S]
    assert causes_of([(0.0, 5.0, 2.0)] * 3, occl=3.0) == [S, S, S]
    assert causes_of([(0.0, 10.0, 1.0), (5.0, 0.0, 100.0)], occl=1.0) == [S, S]
    assert causes_of([(0.0, 10.0, 1.0), (2.5, 5.0, 2.5)], occl=0.0) == [S, S]
    # a chain: A hides B; A alone does not hide C, B (itself lost) does
    chain = [(0.0, 5.0, 0.3), (0.4, 10.0, 1.0), (1.2, 15.0, 1.0)]
    assert causes_of(chain, occl=1.0) == [S, O, O] and causes_of([chain[0], chain[2]], occl=1.0) == [S, S]
    # an occluder outside the cone, and a dropped one, still occlude
    assert causes_of([(3.0, 5.0, 3.5), (0.0, 12.0, 1.0)], occl=1.0, fov_cos=math.cos(math.radians(20.0))) == [F, O]
    assert causes_of([(0.0, 5.0, 1.0), (0.0, 12.0, 1.0)], occl=1.0, p_drop=0.999999) == [D, O]
    # the near field exempts cone and occlusion, not the draw
    near = [(0.0, -3.0, 1.0), (0.0, -1.0, 5.0)]
    assert causes_of(near, fov_cos=0.5, occl=1.0, r_near=4.0) == [S, S] and causes_of(near, fov_cos=0.5, occl=1.0, r_near=2.0) == [F, S]
    assert causes_of(near, fov_cos=0.5, occl=1.0, r_near=4.0, p_drop=0.999999) == [D, D]
    # the first failing test is the cause
    many = [(0.0, -30.0, 1.0), (0.0, -10.0, 5.0)]
    assert causes_of(many, range=20.0, fov_cos=0.5, occl=1.0, p_drop=0.999999) == [R, F]
    assert causes_of(many, range=40.0, fov_cos=0.5, occl=1.0, p_drop=0.999999) == [F, F]
    assert causes_of(many, range=40.0, occl=1.0, p_drop=0.999999) == [O, D]
    assert causes_of(many, range=40.0, p_drop=0.999999) == [D, D]


def test_statistics_of_the_mirror():
    m = sim.SensorModel(2, range=20.0, fov_deg=180.0, occl=1.0)
    assert m.fov_cos[0] == math.cos(math.pi / 2) and sim.SensorModel(1, fov_deg=360.0).fov_cos == [-1.0]
    d0 = m.as_dict()
    assert d0["blind_clear_min"][0] == np.inf and d0["blind_clear_tick"][0] == -1 and d0["ticks"][0] == 0
    objs = [(0.0, 30.0, 1.0), (3.0, -4.0, 1.5), (0.0, 5.0, 1.0), (0.0, 9.0, 1.0)]
    assert m.sense(0, 7, (0.0, 0.0), 0.0, objs) == [1, 2, 0, 3]
    m.sense(0, 8, (0.0, 0.0), 0.0, [(0.0, 5.0, 1.0)])
    m.sense(0, 9, (0.0, 0.0), 0.0, [(3.0, -4.0, 1.5), (-3.0, -4.0, 1.5)])          # the same clearance again: the first smallest stays
    d = m.as_dict()
    assert [d[k][0] for k in ("ticks", "n_obj", "n_seen", "n_range", "n_fov", "n_occl", "n_drop", "blind_ticks")] == [3, 7, 2, 1, 3, 1, 0, 2]
    assert d["blind_clear_min"][0] == 3.5 and d["blind_clear_tick"][0] == 7 and d["ticks"][1] == 0


# ---- 3. dropout ---------------------------------------------------------------------------------------------------------------------------
def test_dropout_draws(shim):
    kat = [((0, 0, 0, 0), (0, 0), 0x6627e8d5), ((0xffffffff,) * 4, (0xffffffff,) * 2, 0x408f276d),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 0xd16cfe09)]
    for ctr, key, w0 in kat:                      # the published known answers of Philox4x32-10, and the u their first word gives
        assert int(sim.philox4x32(ctr, key)[0]) == w0
        assert (float(w0) + 0.5) * 2.0 ** -32 == (w0 * 2 + 1) / 2.0 ** 33 and 0.0 < (float(w0) + 0.5) * 2.0 ** -32 < 1.0
    rng = np.random.default_rng(5)
    words = np.zeros(4, np.uint32)
    for seed, tick, k in [(0, 0, 0), (2 ** 64 - 1, 2 ** 31 - 1, 95), (0x0123456789ABCDEF, 199, 64)] + [
            (int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 2 ** 31)), int(rng.integers(0, 96))) for _ in range(200)]:
        u = shim.sensor_uniform_host(seed, tick, k, words.ctypes.data)
        ref = sim.philox4x32((tick, k, 0, 1), (seed & 0xFFFFFFFF, seed >> 32))
        assert words.tolist() == [int(v) for v in ref]
        assert u == sim.sensor_uniform(seed, tick, k) == (float(ref[0]) + 0.5) * 2.0 ** -32 and 0.0 < u < 1.0
        # counter word 3 separates the block from the twelve blocks noise_gauss uses under the same seed, tick and object
        nw = np.zeros(12, np.uint32)
        for comp in range(4):
            shim.noise_words_host(seed, tick, k, comp, nw.ctypes.data)
            assert np.array_equal(nw, sim.noise_words(seed, tick, k, comp))
            for b in range(3):
                assert nw[4 * b:4 * b + 4].tolist() == [int(v) for v in sim.philox4x32((tick, k, 3 * comp + b, 0), (seed & 0xFFFFFFFF, seed >> 32))]
                assert nw[4 * b:4 * b + 4].tolist() != words.tolist()
    assert np.array_equal(sim.sensor_uniform(np.uint64(9), np.arange(5), 3), [sim.sensor_uniform(9, t, 3) for t in range(5)])
    # p_drop = 0 draws nothing
    causes, u = su.mirror(su.case([(0.0, 5.0, 1.0), (1.0, 6.0, 1.0)], p_drop=0.0))
    assert causes == [0, 0] and all(math.isnan(v) for v in u)
    assert all(math.isnan(v) for v in header(shim, su.case([(0.0, 5.0, 1.0)], p_drop=0.0))[1])
    # the dropped share over 65 536 draws
    n = 65536
    for p_drop, seed in ((0.1, 0x5EED5EED5EED), (0.5, 3), (0.93, 2 ** 63)):
        share = float(np.mean(sim.sensor_uniform(np.uint64(seed), np.arange(n) // 96, np.arange(n) % 96) < p_drop))
        se = math.sqrt(p_drop * (1.0 - p_drop) / n)
        print("p_drop %.2f: dropped share %.5f (standard error %.5f)" % (p_drop, share, se))
        assert abs(share - p_drop) < 5.0 * se


# ---- the host loop ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    return sim.RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


@pytest.fixture(scope="module")
def track():
    return np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz"))


@pytest.fixture(scope="module")
def c2_start():
    return pr.load_ticks("c2")[0]['start']


def run_loop(lat, oracle, table, cls, start, ticks, sensor="plain"):
    from oracle.planner_host import HostPlannerBackend
    pl = [HostPlannerBackend(lat).planner(1)]
    if isinstance(sensor, str):
        loop = sl.HostSimLoop(lat, table, [cls["entry"]], pl, oracle=oracle)
    else:
        loop = su.SensorSimLoop(lat, table, [cls["entry"]], pl, oracle=oracle, sensor=sensor)
    assert loop.set_start(0, start['pos'], start['heading'], cls.get("start_vel", start['vel']), start['max_heading_offset'])[0]
    loop.sim_vel(**cls["vel"])
    return [loop.tick(want_paths=True)[0] for _ in range(ticks)], loop


def same_tick(a, b):
    if a["failed"] or b["failed"]:
        return a["failed"] == b["failed"] and a["sel"] == b["sel"]
    if (a["sel"], a["now"], a["pos"], a["vel"], a["theta"], a["cnt"], a["opp_s"]) != (b["sel"], b["now"], b["pos"], b["vel"], b["theta"], b["cnt"], b["opp_s"]):
        return False
    if len(a["veh"]) != len(b["veh"]) or any(x[0] != y[0] or x[1] != y[1] or not np.array_equal(x[2], y[2]) for x, y in zip(a["veh"], b["veh"])):
        return False
    if a["paths"]["nodes"] != b["paths"]["nodes"] or list(a["traj"][0]) != list(b["traj"][0]):
        return False
    return all(np.array_equal(a["traj"][0][k][0], b["traj"][0][k][0]) for k in a["traj"][0])


@pytest.mark.parametrize("name", ["one", "crowded", "crowded70", "statics", "emerg_first", "failing"])
def test_open_sensor_is_the_host_loop(monteblanco, oracle_backend, table, track, c2_start, name):
    cls = sl.monteblanco_classes(table, track, tuple(c2_start['pos']))[name]
    plain, _ = run_loop(monteblanco, oracle_backend, table, cls, c2_start, 200)
    recs, loop = run_loop(monteblanco, oracle_backend, table, cls, c2_start, 200, sensor=sim.SensorModel(1))
    for k, (a, b) in enumerate(zip(recs, plain)):
        assert same_tick(a, b), "%s tick %d" % (name, k)
    assert np.array_equal(np.array([sl.trace_rows([r]) for r in recs]), np.array([sl.trace_rows([r]) for r in plain]), equal_nan=True)
    d = loop.sensor.as_dict()
    live = sum(not r["failed"] for r in recs)
    assert d["ticks"][0] == live and d["n_seen"][0] == d["n_obj"][0] == sum(r["cnt"] for r in recs if not r["failed"])
    assert d["blind_ticks"][0] == 0 and d["blind_clear_min"][0] == np.inf


# ---- 5. a closed loop ---------------------------------------------------------------------------------------------------------------------
def hidden_car_class(table, start):
    """The ego behind a slow car with a second one hidden behind it (both on the race line, 45 m and 75 m ahead of the start, at
    walking pace), a car that starts 15 m behind the ego and a parked one 600 m ahead."""
    i0 = int(np.argmin((table.x - start['pos'][0]) ** 2 + (table.y - start['pos'][1]) ** 2))
    s0, lap = float(table.s_rl[i0]), float(table.s_rl[-1])
    opp = [(s0 + 45.0, 0.04, 5.0), (s0 + 75.0, 0.04, 5.0), ((s0 - 15.0) % lap, 0.02, 5.0), (s0 + 600.0, 0.0, 5.0)]
    return dict(entry=dict(opponents=opp, static=[], pref=sl.DEFAULT_PREF, pos_est=tuple(start['pos']), vel_est=0.0, zone_gids=[]), vel=sl.C2_VEL)


def test_closed_loop_with_a_hidden_car_and_a_forward_cone(monteblanco, oracle_backend, table, c2_start):
    cls = hidden_car_class(table, c2_start)
    ticks = 120
    plain, _ = run_loop(monteblanco, oracle_backend, table, cls, c2_start, ticks)
    sensor = sim.SensorModel(1, range=300.0, fov_deg=120.0, r_near=3.0, occl=3.0, p_drop=0.1, seed=2026)
    recs, loop = run_loop(monteblanco, oracle_backend, table, cls, c2_start, ticks, sensor=sensor)
    d = loop.sensor.as_dict()
    print({k: v[0] for k, v in d.items()})
    print("all-seeing actions:", [r["sel"] for r in plain][::6])
    print("sensor actions:    ", [r["sel"] for r in recs][::6])
    assert not any(r["failed"] for r in recs) and not any(r["failed"] for r in plain)
    assert d["n_range"][0] > 0 and d["n_fov"][0] > 0 and d["n_occl"][0] > 0 and d["n_drop"][0] > 0
    assert d["n_obj"][0] == d["n_seen"][0] + d["n_range"][0] + d["n_fov"][0] + d["n_occl"][0] + d["n_drop"][0] == sum(len(r["veh_all"]) for r in recs)
    assert [r["sel"] for r in recs] != [r["sel"] for r in plain]
    assert np.isfinite(d["blind_clear_min"][0]) and 0 <= d["blind_clear_tick"][0] < ticks and 0 < d["blind_ticks"][0] <= ticks
    # the hidden car is the second of the list: lost to occlusion while the first one is in front of it
    assert any(r["causes"][1] == sim.SENSOR_OCCL for r in recs)


# ---- 6. trigonometry is not an excuse -----------------------------------------------------------------------------------------------------
def test_no_object_of_the_device_scenarios_lies_on_the_cone(monteblanco, oracle_backend, table, track, c2_start):
    import test_gpu_sim_differential as gd
    total = np.zeros(5, int)
    for name, units, kw, ticks, kind in su.scenarios(table, track, c2_start):
        sc = gd.Scenario(monteblanco, table, units)
        loop = su.host_loop(sc, oracle_backend, kw, kind)
        worst, lost = su.INF, 0
        for k in range(ticks):
            recs = loop.tick()
            assert not any(r["failed"] for r in recs), (name, k)
            worst = min(worst, su.fov_margins(loop, recs))
            lost += sum(c != 0 for r in recs for c in r["causes"])
        print("%s: smallest distance to the cone's boundary %.3g (relative to the object's distance); %d objects lost" % (name, worst, lost))
        assert worst > 1e-9, name
        assert lost > 0, name
        total += loop.sensor.rec[:, 2:7].sum(axis=0).astype(int)
    assert np.all(total > 0), "seen / range / cone / occlusion / dropout over the scenarios: %s" % total


# ---- 7. the entry points ------------------------------------------------------------------------------------------------------------------
def test_sensor_entry_points_check_their_arguments_without_a_device():
    """The real library refuses a null fleet; tools/fakehip/sim_sensor_args.py on the stand-in runtime (plain build): every bad argument is
    refused with a message that names it, without allocation or launch; one more launch per tick while the sensor is set."""
    import sys
    lib = ctypes.CDLL(os.path.join(ROOT, "graphbasedlocaltrajectoryplanner_amd", "csrc", "libltpl_hip.so"))
    assert lib.ltpl_fleet_sim_sensor(None, None) == 1 and lib.ltpl_fleet_sim_sensor_read(None, None, 10) == 1
    assert lib.ltpl_fleet_sim_sensor_eval(None, 0, None, None, None, None, None, None, None, None) == 1
    env = dict(os.environ, FAKEHIP_SAN="none", LTPL_NO_SELFTEST="1")
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "sim_sensor_args.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and "sim sensor args OK" in p.stdout, p.stdout[-3000:]
    assert "launches per tick" in p.stdout, p.stdout[-3000:]


def test_python_binding_and_header_declare_the_entry_points():
    from graphbasedlocaltrajectoryplanner_amd import fleet
    for name in ("sim_sensor", "sim_sensor_read", "sim_sensor_eval"):
        assert callable(getattr(fleet.Fleet, name)), name
    with open(os.path.join(ROOT, "include", "ltpl_hip.h")) as fh:
        hdr = fh.read()
    for name in ("ltpl_fleet_sim_sensor(", "ltpl_fleet_sim_sensor_read(", "ltpl_fleet_sim_sensor_eval(", "#define LTPL_ABI_VERSION 9",
                 "#define LTPL_FLEET_SIM_SENSOR_DOUBLES 10"):
        assert name in hdr, name
    assert sim.SENSOR_DOUBLES == 10 == len(sim.SENSOR_FIELDS) and fleet.SENSOR_FIELDS is sim.SENSOR_FIELDS
    assert float(sim.sensor_fov_cos(360.0)) == -1.0 and float(sim.sensor_fov_cos(180.0)) == math.cos(math.pi / 2)
