"""
CPU: friction maps (graphbasedlocaltrajectoryplanner_amd/friction.py, ltpl_fleet_friction*).

  1. The host mirror ``FrictionGrid``: nodes reproduce exactly, clamping outside the grid, exactness on linear fields, ``local_gg`` against
     ``rows``, ``from_function`` / ``save`` / ``load``.
  2. The recordings of the unmodified reference driven with the grid's dict (tools/gen_golden_friction.py: 'gridmap', 'gridmapdrop'):
     replayed by the oracle's host planner under ``planner_replay.replay``'s rules, and reproduced free running by the host loop of
     tests/sim_loop.py around a planner proxy that builds the dict from its own paths, under the checks of tests/test_sim_loop_host.py.
  3. The argument checks of the three entry points on the stand-in runtime (tools/fakehip/friction_args.py), plain and under ASan + UBSan.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import friction_replay as fr
import planner_replay as pr
import sim_loop as sl
import test_gpu_fleet_sim as gs
from graphbasedlocaltrajectoryplanner_amd import sim
from graphbasedlocaltrajectoryplanner_amd.friction import FrictionGrid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seeded_grid(nx=7, ny=5, seed=3):
    rng = np.random.default_rng(seed)
    return FrictionGrid(-12.5, 30.0, 2.5, 4.0, rng.uniform(2.0, 6.0, (ny, nx)), rng.uniform(2.0, 6.0, (ny, nx)))


# ---- 1. the mirror -------------------------------------------------------------------------------------------------------------------
def test_nodes_reproduce_exactly():
    for g in (seeded_grid(), seeded_grid(2, 2, 4), fr.load_grid()):
        ix, iy = np.meshgrid(np.arange(g.nx), np.arange(g.ny))
        xy = np.column_stack((g.x0 + g.dx * ix.reshape(-1), g.y0 + g.dy * iy.reshape(-1)))
        got = g.rows(xy)
        assert np.array_equal(got[:, 0], g.ax.reshape(-1)) and np.array_equal(got[:, 1], g.ay.reshape(-1))
        assert np.array_equal(g.rows(xy, 0.5), got * 0.5)


def test_clamping_outside_the_grid():
    g = seeded_grid()
    x1, y1 = g.x0 + g.dx * (g.nx - 1), g.y0 + g.dy * (g.ny - 1)
    ys = np.linspace(g.y0, y1, 23)
    xs = np.linspace(g.x0, x1, 29)
    for off in (1e-9, 0.3, 1e6, 1e300):
        # left / right of the grid: the border column at the same y; below / above: the border row at the same x
        assert np.array_equal(g.rows(np.column_stack((np.full_like(ys, g.x0 - off), ys))), g.rows(np.column_stack((np.full_like(ys, g.x0), ys))))
        assert np.array_equal(g.rows(np.column_stack((np.full_like(ys, x1 + off), ys))), g.rows(np.column_stack((np.full_like(ys, x1), ys))))
        assert np.array_equal(g.rows(np.column_stack((xs, np.full_like(xs, g.y0 - off)))), g.rows(np.column_stack((xs, np.full_like(xs, g.y0)))))
        assert np.array_equal(g.rows(np.column_stack((xs, np.full_like(xs, y1 + off)))), g.rows(np.column_stack((xs, np.full_like(xs, y1)))))
    # the corners
    got = g.rows([[g.x0 - 5.0, g.y0 - 5.0], [x1 + 5.0, g.y0 - 5.0], [g.x0 - 5.0, y1 + 5.0], [x1 + 5.0, y1 + 5.0]])
    assert np.array_equal(got[:, 0], [g.ax[0, 0], g.ax[0, -1], g.ax[-1, 0], g.ax[-1, -1]])
    assert np.array_equal(got[:, 1], [g.ay[0, 0], g.ay[0, -1], g.ay[-1, 0], g.ay[-1, -1]])
    inside = g.inside([[g.x0, g.y0], [x1, y1], [g.x0 - 1e-9, g.y0], [x1, y1 + 1e-9]])
    assert inside.tolist() == [True, True, False, False]


def test_linear_fields_are_exact():
    # node values and sample points on a dyadic lattice: every product and sum of the interpolation is exact in fp64
    def f(xy):
        return np.column_stack((8.0 + 0.25 * xy[:, 0] + 0.5 * xy[:, 1], 16.0 - 0.125 * xy[:, 0] + 0.25 * xy[:, 1]))
    g = FrictionGrid.from_function(f, (-8.0, -4.0, 8.0, 12.0), (2.0, 4.0))
    assert (g.nx, g.ny) == (9, 5)
    rng = np.random.default_rng(5)
    xy = np.column_stack((rng.integers(-8 * 64, 8 * 64 + 1, 4000) / 64.0, rng.integers(-4 * 64, 12 * 64 + 1, 4000) / 64.0))
    assert np.array_equal(g.rows(xy), f(xy))
    # any point: to rounding
    xy = np.column_stack((rng.uniform(-8.0, 8.0, 4000), rng.uniform(-4.0, 12.0, 4000)))
    assert np.max(np.abs(g.rows(xy) - f(xy))) <= 64 * np.finfo(float).eps * 32.0


def test_local_gg_against_rows(tmp_path):
    g = seeded_grid()
    rng = np.random.default_rng(9)
    paths = {"straight": rng.uniform(-20.0, 60.0, (40, 5)), "left": [rng.uniform(-20.0, 60.0, (17, 5))], "follow": np.zeros((0, 5))}
    lgg = g.local_gg(paths, 0.7)
    assert list(lgg) == ["straight", "left", "follow"]
    for k, v in paths.items():
        pp = v[0] if isinstance(v, list) else v
        assert isinstance(lgg[k], list) and len(lgg[k]) == 1 and lgg[k][0].shape == (pp.shape[0], 2)
        assert np.array_equal(lgg[k][0], g.rows(pp[:, 0:2], 0.7))
    g.save(str(tmp_path / "g.npz"))
    h = FrictionGrid.load(str(tmp_path / "g.npz"))
    assert (h.x0, h.y0, h.dx, h.dy) == (g.x0, g.y0, g.dx, g.dy) and np.array_equal(h.ax, g.ax) and np.array_equal(h.ay, g.ay)
    assert np.array_equal(h.nodes().reshape(g.ny, g.nx, 2)[:, :, 1], g.ay)


@pytest.mark.parametrize("kw", [dict(ax=np.ones((1, 4)), ay=np.ones((1, 4))), dict(ax=np.ones((3, 1)), ay=np.ones((3, 1))),
                                dict(ax=np.ones((3, 3)), ay=np.ones((3, 4))), dict(dx=0.0), dict(dy=-1.0), dict(x0=np.nan), dict(dx=np.inf),
                                dict(ax=np.array([[1.0, 2.0], [0.0, 1.0]])), dict(ay=np.array([[1.0, 2.0], [np.nan, 1.0]])),
                                dict(ay=np.array([[1.0, -2.0], [1.0, 1.0]]))])
def test_invalid_grids_are_refused(kw):
    args = dict(x0=0.0, y0=0.0, dx=1.0, dy=1.0, ax=np.ones((2, 2)), ay=np.ones((2, 2)))
    with pytest.raises(ValueError):
        FrictionGrid(**dict(args, **kw))


def test_host_build_of_the_device_code_equals_the_mirror(tmp_path):
    """csrc/fleet_core.hpp's ``friction_at`` -- the function the kernels run -- compiled for the host (one lane, -ffp-contract=off like the
    library) against the mirror, bit for bit; the same translation unit instantiates stage A with the map compiled in (vel_a<HostX, true>)."""
    import ctypes
    so = str(tmp_path / "friction_core_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "friction_core_shim.cpp")],
                   check=True, timeout=600)
    lib = ctypes.CDLL(so)
    D, I, P = ctypes.c_double, ctypes.c_int, ctypes.c_void_p
    lib.friction_rows_host.argtypes = [D, D, D, D, I, I, P, P, P, I, D, P]
    rng = np.random.default_rng(23)
    for g, scale in ((seeded_grid(), 1.0), (seeded_grid(2, 2, 8), 0.3), (fr.load_grid(), 0.77)):
        w, h = g.dx * (g.nx - 1), g.dy * (g.ny - 1)
        ix, iy = np.meshgrid(np.arange(g.nx), np.arange(g.ny))
        pts = np.concatenate([np.column_stack((g.x0 + g.dx * ix.reshape(-1), g.y0 + g.dy * iy.reshape(-1))),
                              np.column_stack((rng.uniform(g.x0 - w, g.x0 + 2 * w, 20000), rng.uniform(g.y0 - h, g.y0 + 2 * h, 20000))),
                              np.array([[-1e300, 1e300], [1e300, -1e300]])])
        x, y, nodes = np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1]), g.nodes()
        out = np.zeros((len(pts), 2))
        lib.friction_rows_host(g.x0, g.y0, g.dx, g.dy, g.nx, g.ny, nodes.ctypes.data, x.ctypes.data, y.ctypes.data, len(pts), scale, out.ctypes.data)
        assert np.array_equal(out, g.rows(pts, scale))


# ---- 2. the recordings --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(monteblanco):
    from oracle.planner_host import HostPlannerBackend
    return HostPlannerBackend(monteblanco)


@pytest.fixture(scope="module")
def table():
    return sim.RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


@pytest.mark.parametrize("name,must_see", [("gridmap", {"follow", "emergency"}), ("gridmapdrop", {"straight", "emergency"})])
def test_host_planner_replays_the_grid_recordings(host, monteblanco, name, must_see):
    ticks, grid = pr.load_ticks(name), fr.load_grid()
    seen = fr.replay(host.planner(1), monteblanco, ticks, grid)
    assert must_see <= seen['keys'] and seen['full'] >= 15, seen
    assert seen.get('ggmap', 0) == len(ticks)                 # every tick ran with the dict form, its first rows equal to the recorded ones
    if name == "gridmap":
        assert seen['keys'] & {"left", "right"}
        assert all(('emergency' in t['vel']['keys']) == (100 <= t['tick'] < 200) for t in ticks)


@pytest.mark.parametrize("name", sorted(fr.SPECS))
def test_host_loop_reproduces_the_grid_recordings(monteblanco, oracle_backend, host, table, name):
    """Free running: the loop of tests/sim_loop.py around a planner that builds the dict from its own paths (``GridPlanner``) -- the
    checks of tests/test_sim_loop_host.py's recording test."""
    ticks, grid = pr.load_ticks(name), fr.load_grid()
    gp = fr.GridPlanner(host.planner(1), grid)
    loop = sl.HostSimLoop(monteblanco, table, [fr.planner_entry(monteblanco, name, ticks)], [gp], oracle=oracle_backend)
    st = ticks[0]['start']
    assert loop.set_start(0, st['pos'], st['heading'], st['vel'], st['max_heading_offset']) == (st['in_track'], st['cor_heading'])
    rows = []
    for t in ticks:
        gp.scale = t['grid_scale']
        loop.sim_vel(**fr.vel_of(t))
        rec = loop.tick()
        rows.append(sl.trace_rows(rec))
        assert not rec[0]["failed"], (t['tick'], rec[0].get("error"))
        pr.check_trajectories(*rec[0]["traj"], t, "%s tick %d" % (name, t['tick']))
        pr.assert_close_rel(gp.first_rows, t['vel_args']['local_gg_first'], what="%s tick %d: rows of the first key" % (name, t['tick']))
    gs.check_trace(np.array(rows), ticks, [0], name)


# ---- 3. the entry points' argument checks ----------------------------------------------------------------------------------------------
def test_friction_entry_points_check_their_arguments_without_a_device():
    env = dict(os.environ, FAKEHIP_SAN="none", LTPL_NO_SELFTEST="1")
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "friction_args.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and "friction args OK" in p.stdout, p.stdout[-3000:]
    assert "map_idx out of range" in p.stdout and "previous maps kept" in p.stdout, p.stdout[-3000:]


def test_friction_entry_points_under_the_sanitizers():
    """The same driver on the ASan + UBSan build of the host code (the sanitizer run-time preloaded as tools/fakehip/run.sh does)."""
    env = {k: v for k, v in os.environ.items() if k != "FAKEHIP_SAN"}
    env["LTPL_NO_SELFTEST"] = "1"
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    rt = subprocess.check_output([clang, "-print-file-name=libclang_rt.asan-x86_64.so"], universal_newlines=True).strip()
    if not os.path.isfile(rt):
        import glob
        rt = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))[0]
    # (the sanitizer run-time goes IN FRONT of whatever the environment preloads already)
    env.update(LD_PRELOAD=" ".join([rt] + env.get("LD_PRELOAD", "").replace(":", " ").split()), ASAN_OPTIONS="detect_leaks=0:halt_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "friction_args.py"), "--san"], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=1200)
    assert p.returncode == 0 and "friction args OK" in p.stdout, p.stdout[-3000:]
    assert ": runtime error:" not in p.stdout and "ERROR: AddressSanitizer" not in p.stdout, p.stdout[-3000:]
