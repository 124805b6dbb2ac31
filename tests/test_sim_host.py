"""
CPU: the host mirrors of the closed-loop simulation (graphbasedlocaltrajectoryplanner_amd/sim.py) against the tick recordings of the
unmodified reference -- opponents (ObjectlistDummy) bit for bit on every tick, the ideal ego tracker (vdc_dummy) bit for bit from every tick
whose recording holds the full trajectory the next tick tracks -- the scalar np.interp restatement against np.interp, and the argument checks
of the ltpl_fleet_sim_* entry points (host code only, linked against the stand-in runtime of tools/fakehip).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import planner_replay as pr
from graphbasedlocaltrajectoryplanner_amd import sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRED_DT = 0.2
# recording -> opponents (s0, vel_scale) as oracle/gen_golden.py drives them; the fake clock and every opponent's tic start at 1e6
OPPONENTS = {
    "c2": [(250.0 + 280.0 * k, 0.30 + 0.05 * (k % 4)) for k in range(8)],
    "car2": [(140.0, 0.4)],
    "overtake": [(120.0, 0.5)],
    "filt5": [(200.0, 0.4)],
    "zonewall": [(180.0, 0.15)],
}


@pytest.fixture(scope="module")
def table():
    return sim.RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


@pytest.mark.parametrize("name", sorted(OPPONENTS))
def test_opponents_reproduce_the_recording_bit_for_bit(table, name):
    ticks = pr.load_ticks(name)
    lists = table.lists()
    opp = OPPONENTS[name]
    state = [(s0, 1.0e6) for s0, _ in opp]
    now = 1.0e6
    for k, t in enumerate(ticks):
        now += 0.05                                      # FakeClock.advance: an fp64 accumulation
        assert now == t['t'], "tick %d: clock" % k
        assert len(t['obj_radius']) == len(opp)
        for q, (_, scale) in enumerate(opp):
            s, tic, x, y, psi, v = sim.opponent_step(table, state[q][0], state[q][1], now, scale, lists)
            state[q] = (s, tic)
            assert (x, y) == tuple(t['obj_pos'][q]) and v == t['obj_vel'][q], "tick %d opponent %d: %r vs %r" % (k, q, (x, y, v), t['obj_pos'][q])
            pred = (x - np.sin(psi) * v * PRED_DT, y + np.cos(psi) * v * PRED_DT)
            assert pred == tuple(np.asarray(t['obj_pred'][q]).reshape(-1)), "tick %d opponent %d: prediction" % (k, q)


@pytest.mark.parametrize("name", ["c2", "car2", "overtake", "filt5", "zonewall", "c1"])
def test_ego_tracker_reproduces_the_next_pose_bit_for_bit(name):
    ticks = pr.load_ticks(name)
    n = 0
    for i in range(len(ticks) - 1):
        full, sel = ticks[i]['full'], ticks[i + 1]['action_id_sel']
        if full is None or sel not in full.get('traj', {}):
            continue
        pos, vel = sim.vdc_step(ticks[i]['pos_est'], full['traj'][sel][:115], 0.05)      # exported rows: nmbr_export_points = 115
        nxt = ticks[i + 1]
        assert pos == list(nxt['pos_est']) and vel == nxt['vel_args']['vel_est'], "tick %d -> %d" % (i, i + 1)
        n += 1
    assert n >= 20, n


def test_short_trajectory_keeps_the_pose():
    traj = np.array([[0.0, 1.0, 2.0, 0.0, 0.0, 7.5, 0.0], [1.0, 1.0, 3.0, 0.0, 0.0, 8.0, 0.0]])
    assert sim.vdc_step([4.0, 5.0], traj, 0.05) == ([4.0, 5.0], 7.5)


def test_interp_equals_numpy_bit_for_bit():
    rng = np.random.default_rng(7)
    xp = np.cumsum(rng.uniform(0.0, 3.0, 200)) + 5.0
    xp[50] = xp[49]                                      # a repeated knot
    fp = rng.normal(size=200) * 40.0
    xl, fl = xp.tolist(), fp.tolist()
    xs = np.concatenate((rng.uniform(xp[0] - 10.0, xp[-1] + 10.0, 4000), xp, [xp[0], xp[-1], xp[0] - 1e-9, xp[-1] + 1e-9, 0.0, -1e30, 1e30],
                         np.nextafter(xp, -np.inf), np.nextafter(xp, np.inf)))
    for x in xs:
        a, b = sim.interp(float(x), xl, fl), float(np.interp(x, xp, fp))
        assert a == b or (np.isnan(a) and np.isnan(b)), (x, a, b)
    assert np.isnan(sim.interp(float("nan"), xl, fl))
    # NaN fallback: an infinite slope where both ends are equal infinities
    assert sim.interp(1.5, [1.0, 2.0], [np.inf, np.inf]) == float(np.interp(1.5, [1.0, 2.0], [np.inf, np.inf]))


def test_race_line_table(table):
    rows = table.rows()
    assert rows.shape[1] == 5 and rows[0, 0] > 0.0 and np.all(np.diff(rows[:, 0]) > 0.0)       # s_rl = cumsum(length_rl): no 0 in front
    assert np.all(rows[:, 3] >= 0.0) and np.all(rows[:, 3] < 2 * np.pi)


# ---- argument checks of the C ABI without a device ------------------------------------------------------------------------------------
def _fake_lib():
    lib = os.path.join(ROOT, "tools", "fakehip", "build_plain", "libltpl_hip_fake.so")
    src = [os.path.join(ROOT, "graphbasedlocaltrajectoryplanner_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "graphbasedlocaltrajectoryplanner_amd", "csrc"))
           if f.endswith((".hip", ".hpp"))] + [os.path.join(ROOT, "include", "ltpl_hip.h")]
    if not os.path.isfile(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in src):
        env = dict(os.environ, FAKEHIP_SAN="none")
        subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    return lib


def test_sim_entry_points_check_their_arguments_without_a_device(monteblanco, monkeypatch):
    from graphbasedlocaltrajectoryplanner_amd import _capi
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet, SimIn
    import __graft_entry__ as ge
    real = ctypes.CDLL(ge.build_hip())
    for name in ("ltpl_fleet_sim_setup", "ltpl_fleet_sim_vel", "ltpl_fleet_sim_run", "ltpl_fleet_sim_state"):
        getattr(real, name).restype = ctypes.c_int
    assert real.ltpl_fleet_sim_setup(None, None) == 1 and real.ltpl_fleet_sim_vel(None, None) == 1
    assert real.ltpl_fleet_sim_run(None, 1, None, 0, None) == 1 and real.ltpl_fleet_sim_state(None, *([None] * 7)) == 1

    monkeypatch.setenv("LTPL_NO_SELFTEST", "1")                           # (kernels do nothing on the stand-in runtime)
    hip = _capi.HipBackend(monteblanco, lib_path=_fake_lib())
    fleet = Fleet(hip, 2)
    table = sim.RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))
    good = dict(opponents=[(250.0, 0.3, 5.0)], pref=("right", "straight"), pos_est=(0.0, 0.0), zone_gids=[3])
    fleet.sim_setup(table, [good, good])                                  # (host side only: the stand-in runtime copies, kernels do nothing)
    fleet.sim_vel()
    for bad, what in (([good, dict(good, pref=())], "1 .. 5 entries"), ([good, dict(good, pref=("left",) * 6)], "1 .. 5 entries"),
                      ([good, dict(good, zone_gids=[10 ** 6])], "zone node id"),
                      ([good, dict(good, opponents=[(0.0, 0.1, 5.0)] * 97)], "more than 96 objects")):
        with pytest.raises(_capi.BackendError, match=what):
            fleet.sim_setup(table, bad)
    with pytest.raises(_capi.BackendError, match="s_rl"):
        fleet.sim_setup(table.rows()[::-1], [good, good])
    with pytest.raises(_capi.BackendError, match="n_export"):
        fleet.sim_setup(table, [good, good], n_export=0)
    # bad CSR offsets straight through the struct
    si = SimIn()
    rows = table.rows()
    off_bad = np.array([0, 2, 1], np.int32)
    off0 = np.zeros(3, np.int32)
    one = np.zeros(4, np.float64)
    pref_off, pref = np.array([0, 1, 2], np.int32), np.zeros(2, np.int32)
    si.n_rl, si.race = rows.shape[0], rows.ctypes.data
    si.opp_off, si.opp_s0, si.opp_vel_scale, si.opp_length = off_bad.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data
    si.static_off, si.pref_off, si.pref_action, si.zone_off = off0.ctypes.data, pref_off.ctypes.data, pref.ctypes.data, off0.ctypes.data
    si.pos_est_x = si.pos_est_y = si.vel_est = one.ctypes.data
    si.dt, si.n_export = 0.05, 115
    hip.lib.ltpl_fleet_last_error.restype = ctypes.c_char_p
    hip.lib.ltpl_fleet_last_error.argtypes = [ctypes.c_void_p]
    f = hip.lib.ltpl_fleet_sim_setup
    f.argtypes = [ctypes.c_void_p, ctypes.POINTER(SimIn)]
    assert f(fleet.handle, ctypes.byref(si)) == 1 and b"must not decrease" in hip.lib.ltpl_fleet_last_error(fleet.handle)
    off_bad[:] = (1, 1, 1)
    assert f(fleet.handle, ctypes.byref(si)) == 1 and b"start at 0" in hip.lib.ltpl_fleet_last_error(fleet.handle)
    # local_gg as a dict (rows per path) is not supported by the simulation; a trace of the wrong record size is refused
    from graphbasedlocaltrajectoryplanner_amd.planner import PlannerVelIn
    vi, _keep = fleet._pack_vel_in([(0.0, 0.0)] * 2, 0.0)
    rows_gg = np.zeros(2, np.float64)
    vi.gg_row_off, vi.gg_rows = rows_gg.ctypes.data, rows_gg.ctypes.data
    g = hip.lib.ltpl_fleet_sim_vel
    g.argtypes = [ctypes.c_void_p, ctypes.POINTER(PlannerVelIn)]
    assert g(fleet.handle, ctypes.byref(vi)) == 5                         # LTPL_ERR_UNSUPPORTED
    r = hip.lib.ltpl_fleet_sim_run
    r.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    buf = np.zeros(64, np.float64)
    assert r(fleet.handle, 1, buf.ctypes.data, 7, None) == 1 and r(fleet.handle, 0, None, 0, None) == 1
    fleet.close()
    hip.close()
