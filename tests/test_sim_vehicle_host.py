"""
CPU: the vehicle model of the fleet's simulation (ltpl_fleet_sim_vehicle) off the device --

  1. csrc/fleet_vehicle.hpp, compiled with the host compiler and -ffp-contract=off, equals the Python mirror sim.VehicleModel bit for
     bit: state and statistics after a tick of the seeded and the constructed cases of sim_vehicle_util.cases (which are shown to reach
     the boundaries they are named after), and single plant steps;
  2. physics neither implementation defines: a car on a straight constant-speed trajectory stays on it (e exactly 0, (c, s) bitwise
     unchanged); with kappa and v held constant 10 000 plant steps lie on the circle of radius 1 / kappa within 1e-10 R; c c + s s stays
     within 1e-13 of 1 inside a tick; a step in a_cmd reaches 63 % after tau_a within the discretisation error h / (2 tau_a);
  3. closed loop on the host (sim_vehicle_util.VehicleSimLoop over the oracle's planner): with sim.VEHICLE_DEFAULTS the classes 'empty'
     and 'one' run 600 ticks on Monteblanco without a planner error and on the track in every tick, 'one' takes at least three
     different actions; with the grip lowered until ax_lim = ay_lim = 5 (the planner's own gg: no headroom) the car leaves the track
     within 1 500 ticks.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import sim_vehicle_util as vu
from graphbasedlocaltrajectoryplanner_amd import sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vehicle") / "sim_vehicle_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "sim_vehicle_shim.cpp")],
                   check=True)
    lib = ctypes.CDLL(so)
    P = ctypes.c_void_p
    lib.veh_tick_host.argtypes = [P, P, P, ctypes.c_int, ctypes.c_double, ctypes.c_int, P]
    lib.veh_plant_host.argtypes = [P, P, ctypes.c_double, ctypes.c_double, ctypes.c_int]
    return lib


def shim_tick(shim, c):
    state, par, rows, stats = np.array(c["state"]), np.array(c["par"]), np.ascontiguousarray(c["rows"]), np.zeros(7)
    shim.veh_tick_host(state.ctypes.data, par.ctypes.data, rows.ctypes.data, rows.shape[0], c["dt"], c["ctl"], stats.ctypes.data)
    return np.concatenate((state, stats))


@pytest.fixture(scope="module")
def cases():
    return vu.cases()


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_header_equals_the_mirror_bit_for_bit(shim, cases):
    assert len(cases) >= 60 and sum(c["name"].startswith("seeded") for c in cases) == 40
    for c in cases + vu.stride_cases():
        ref, _, _ = vu.mirror_tick(c)
        got = shim_tick(shim, c)
        assert np.array_equal(bits(got), bits(ref)), "%s: %s vs %s" % (c["name"], got, ref)
    # single plant steps with held commands
    par = np.array(vu.PAR0)
    for kc, ac, steps in ((0.05, 2.0, 1), (-0.11, -3.0, 17), (0.0, 0.0, 5)):
        m = sim.VehicleModel(3.0, -2.0, 0.7, 12.0)
        st = np.array(m.state())
        shim.veh_plant_host(st.ctypes.data, par.ctypes.data, kc, ac, steps)
        for _ in range(steps):
            m.plant(kc, ac)
        assert np.array_equal(bits(st), bits(m.state()))


def test_the_constructed_cases_reach_their_boundaries(cases):
    by = {c["name"]: c for c in cases}
    res = {k: vu.mirror_tick(c) for k, c in by.items()}

    def first_control(name):
        """(d2 and u of every segment at the case's start pose, the statistics of the tick)"""
        c = by[name]
        cols = sim.VehicleModel.columns(c["rows"])
        segs = [sim.VehicleModel._seg(cols[1], cols[2], i, c["state"][0], c["state"][1]) for i in range(len(cols[0]) - 1)]
        return segs, res[name][2].stats
    segs, _ = first_control("tie_two_segments")
    assert segs[0][0] == segs[1][0] == 4.0 and segs[2][0] > 4.0
    segs, st = first_control("foot_on_knot")
    assert segs[0][0] == segs[1][0] == 9.0 and segs[0][1] == 1.0 and segs[1][1] == 0.0
    assert first_control("u_clamped_low")[0][0][1] == 0.0 and first_control("u_clamped_high")[0][-1][1] == 1.0
    for name, where in (("zero_length_start", 0), ("zero_length_middle", 1), ("zero_length_end", -1)):
        segs, st = first_control(name)
        assert segs[where] is None and st["ctl_steps"] == 5, name
    # no usable trajectory: the steering is held, the car brakes with -ax_lim, no statistic moves
    for name in ("all_degenerate", "rows0", "rows1", "rows2"):
        rec, _, m = res[name]
        assert m.stats == dict(e=0.0, e_max=0.0, e2_sum=0.0, dv_max=0.0, ctl_steps=0, sat_lat=0, sat_lon=0, off_track_ticks=0), name
        assert rec[5] < 0.0 and rec[4] < 10.0 and rec[6] == 0.01, name
    assert res["rows3"][2].stats["ctl_steps"] == 5
    for name in ("lookahead_beyond_end", "lookahead_beyond_end_last_degenerate"):
        c = by[name]
        assert c["rows"][-1, 0] < 0.5 + sim.VEHICLE_DEFAULTS["ld_min"] and res[name][2].stats["ctl_steps"] == 5
    assert res["standstill"][0][4] == 0.0 and res["standstill"][0][0] == 1.0 and res["standstill_pulls_away"][0][4] > 0.0
    # |kappa_cmd| v^2 = 2 against ay_lim = 2 and its neighbours: the clamp takes hold strictly above
    assert [res["sat_lat_%s" % t][2].stats["sat_lat"] for t in ("below", "at", "above")] == [1, 0, 0]
    assert res["sat_lon_accel"][2].stats["sat_lon"] == 5 and res["sat_lon_brake"][2].stats["sat_lon"] == 5
    assert res["sat_lon_accel"][0][5] > 0.0 > res["sat_lon_brake"][0][5]
    c = by["q2_above_one"]
    v2, ay = c["state"][4] ** 2, c["par"][1] * c["par"][2]
    assert ((ay / v2) * v2) / ay > 1.0 and res["q2_above_one"][2].stats["sat_lat"] == 1 and np.all(np.isfinite(res["q2_above_one"][0]))
    # plant steps of a tick: ctl_steps 1 counts them
    steps = {name: res[name][2].stats["ctl_steps"] for name in ("dt0.0495", "dt0.05", "dt0.0505")}
    assert {50, 51} <= set(steps.values()) and steps["dt0.0495"] == 50 and steps["dt0.0505"] == 51, steps
    assert [res["ctl%d" % k][2].stats["ctl_steps"] for k in (1, 7, 60)] == [steps["dt0.05"], -(-steps["dt0.05"] // 7), 1]


# ---- physics ----------------------------------------------------------------------------------------------------------------------------
def test_a_car_on_a_straight_constant_speed_trajectory_stays_on_it():
    # along the four axis directions the line is exact in fp64, for any spacing of the rows: e is exactly 0, (c, s) bitwise unchanged
    for c0, s0 in ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)):
        rows = vu.line_rows([(3.0 + d * c0, -7.0 + d * s0) for d in (0.0, 0.7, 5.0, 111.0, 300.0)], v=15.0)
        m = sim.VehicleModel(0.0, 0.0, 0.0, 0.0)
        m.set_state([3.0, -7.0, c0, s0, 15.0, 0.0, 0.0])
        for _ in range(100):
            m.tick(rows, 0.05)
            assert m.stats["e"] == 0.0 and (m.c, m.s, m.v, m.a, m.kappa) == (c0, s0, 15.0, 0.0, 0.0)
            assert (m.y == -7.0) if s0 == 0.0 else (m.x == 3.0)
        assert m.stats["e_max"] == 0.0 and abs(math.hypot(m.x - 3.0, m.y + 7.0) - 75.0) < 1e-9
    # (an oblique line's rows are rounded products and not collinear in fp64: no exact statement there)
    # the heading is the library's, measured from the y axis: heading 0 drives along +y, a quarter turn to the left along -x
    for th, (dx, dy) in ((0.0, (0.0, 1.0)), (math.pi / 2, (-1.0, 0.0)), (-2.5, (-math.sin(-2.5), math.cos(-2.5)))):
        m = sim.VehicleModel(0.0, 0.0, th, 10.0)
        m.plant(0.0, 0.0)
        assert abs(m.x - 0.01 * dx) < 1e-15 and abs(m.y - 0.01 * dy) < 1e-15 and abs(m.theta - th) < 1e-15


def test_constant_curvature_and_speed_stay_on_the_circle():
    """10 000 plant steps (10 s, 2.4 turns at R = 12.5 m, v = 19 m/s) with kappa and v held: every point within 1e-10 R of the circle."""
    for kappa, v in ((0.08, 19.0), (-0.02, 40.0), (0.2, 5.0)):
        R = 1.0 / abs(kappa)
        m = sim.VehicleModel(1.0, 2.0, 0.3, v, tau_kappa=0.001)
        m.kappa = kappa
        cx, cy = m.x - m.s / kappa, m.y + m.c / kappa              # the centre: 1 / kappa to the left
        worst = 0.0
        for _ in range(10000):
            m.plant(kappa, 0.0)                                     # (a = 0, kappa_cmd = kappa: neither moves)
            worst = max(worst, abs(math.hypot(m.x - cx, m.y - cy) - R))
        assert m.kappa == kappa and m.v == v
        assert worst <= 1e-10 * R, (kappa, v, worst / R)


def test_the_heading_stays_a_unit_vector_inside_a_tick():
    rng = np.random.default_rng(3)
    rows, psi = vu.arc_rows(115, rng)
    m = sim.VehicleModel(0.0, 0.0, 0.0, 0.0)
    m.set_state(vu.state_at(rows, psi, 0, lat=0.5, dpsi=0.1, v=15.0))
    cols = m.columns(rows)
    worst = 0.0
    for _ in range(40):                                             # 40 ticks, looked at after every plant step
        t, k, cmd = 0.0, 0, None
        while t < 0.05:
            if k % m.ctl_steps == 0:
                cmd = m.control(cols)
            m.plant(*cmd)
            worst = max(worst, abs(m.c * m.c + m.s * m.s - 1.0))
            t += sim.VEH_STEP
            k += 1
        r = math.sqrt(m.c * m.c + m.s * m.s)
        m.c, m.s = m.c / r, m.s / r
    assert 0.0 < m.stats["e_max"] and worst <= 1e-13, worst


def test_a_step_in_a_cmd_reaches_63_percent_after_tau_a():
    for tau in (0.1, 0.02, 0.25):
        m = sim.VehicleModel(0.0, 0.0, 0.0, 10.0, tau_a=tau)
        steps = int(round(tau / sim.VEH_STEP))
        for _ in range(steps):
            m.plant(0.0, 4.0)
        # the explicit Euler step of a first-order lag: (1 - h / tau)^(tau / h) against exp(-1), relative error h / (2 tau) + O(h^2)
        assert abs(m.a / 4.0 - (1.0 - math.exp(-1.0))) <= sim.VEH_STEP / (2.0 * tau), (tau, m.a)


# ---- closed loop on the host ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    return sim.RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


@pytest.fixture(scope="module")
def classes(table):
    start = pr.load_ticks("c2")[0]['start']
    return sl.monteblanco_classes(table, np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")), tuple(start['pos'])), start


def run_loop(lat, oracle, table, cls, start, ticks, stop_off_track=False, **vehicle):
    from oracle.planner_host import HostPlannerBackend
    loop = vu.VehicleSimLoop(lat, table, [cls["entry"]], [HostPlannerBackend(lat).planner(1)], oracle=oracle)
    assert loop.set_start(0, start['pos'], start['heading'], start['vel'], start['max_heading_offset'])[0]
    loop.theta = [float(start['heading'])]
    loop.sim_vel(**cls["vel"])
    loop.sim_vehicle(**vehicle)
    recs = []
    for _ in range(ticks):
        recs.append(loop.tick()[0])
        if recs[-1]["failed"] or (stop_off_track and loop.veh[0].stats["off_track_ticks"] > 0):
            break
    return recs, loop.veh[0]


@pytest.mark.parametrize("name", ["empty", "one"])
def test_defaults_drive_600_ticks_on_the_track(monteblanco, oracle_backend, table, classes, name):
    cls, start = classes
    assert cls[name]["vel"]["local_gg"] == (5.0, 5.0) and sim.VEHICLE_DEFAULTS["ax_max"] * sim.VEHICLE_DEFAULTS["grip"] == 6.0    # 20 % headroom
    recs, veh = run_loop(monteblanco, oracle_backend, table, cls[name], start, 600)
    assert len(recs) == 600 and not any(r["failed"] for r in recs), [r.get("error") for r in recs if r["failed"]][:1]
    assert veh.stats["off_track_ticks"] == 0 and veh.stats["ctl_steps"] >= 599 * 5
    acts = sorted(set(r["sel"] for r in recs))
    print("%s: actions %s, e_max %.3f m, rms e %.3f m, dv_max %.2f m/s, sat_lat %d, sat_lon %d of %d control steps, v at the end %.1f m/s" %
          (name, acts, veh.stats["e_max"], math.sqrt(veh.stats["e2_sum"] / veh.stats["ctl_steps"]), veh.stats["dv_max"], veh.stats["sat_lat"],
           veh.stats["sat_lon"], veh.stats["ctl_steps"], veh.v))
    if name == "one":
        assert len(acts) >= 3, acts


def test_without_headroom_the_car_leaves_the_track(monteblanco, oracle_backend, table, classes):
    cls, start = classes
    recs, veh = run_loop(monteblanco, oracle_backend, table, cls["empty"], start, 1500, stop_off_track=True, grip=5.0 / 6.0)
    print("no headroom: off the track in tick %d, sat_lat %d, sat_lon %d, e_max %.2f m" % (len(recs) - 1, veh.stats["sat_lat"], veh.stats["sat_lon"],
                                                                                         veh.stats["e_max"]))
    assert veh.stats["off_track_ticks"] > 0 and veh.stats["sat_lat"] + veh.stats["sat_lon"] > 0


def test_python_binding_and_header_declare_the_entry_points():
    from graphbasedlocaltrajectoryplanner_amd import fleet
    for name in ("sim_vehicle", "sim_vehicle_read", "sim_vehicle_step"):
        assert callable(getattr(fleet.Fleet, name)), name
    with open(os.path.join(ROOT, "include", "ltpl_hip.h")) as fh:
        hdr = fh.read()
    for name in ("ltpl_fleet_sim_vehicle(", "ltpl_fleet_sim_vehicle_read(", "ltpl_fleet_sim_vehicle_step(", "#define LTPL_ABI_VERSION 9",
                 "#define LTPL_FLEET_SIM_VEH_DOUBLES %d" % sim.VEHICLE_DOUBLES):
        assert name in hdr, name
    assert [f[1] for f in sim.VEHICLE_FIELDS] == list(range(sim.VEHICLE_DOUBLES)) and len(sim.VEHICLE_PARAMS) == 9
    d = sim.vehicle_dict(np.vstack((np.arange(15.0), np.full(15, np.nan))))
    assert d["off_track_ticks"].tolist() == [14, -1] and d["kappa"][0] == 6.0 and np.isnan(d["x"][1])
