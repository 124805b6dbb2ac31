"""
CPU: the prediction model of the fleet's simulation (ltpl_fleet_sim_predictor) off the device --

  1. csrc/fleet_predict.hpp, compiled alone with the host compiler (-ffp-contract=off), equals the Python mirror sim.PredictorModel bit for
     bit on the case list of sim_predictor_util.cases (seeded cases plus the boundaries: on a row, rows 0 and n - 1, equidistant segments,
     clamped foot points, |d| == d_max and one double above, against the track, v = 0 / NaN, s_j on and around S[n - 1], K = 1 and 8, the
     object counts of the device's pass edges) and on a table with a duplicated row; every boundary group shows the outcome it is there for;
  2. the header's own stand-alone program under -fsanitize=address,undefined (a plain executable) exits 0;
  3. properties of the mirror on the Monteblanco table: an opponent on the race line is predicted onto the race line (bound derived
     below), mode 1 with K = 1 and T = 0.2 is the written expression, mode 0 repeats (px, py);
  4. a closed loop on Monteblanco under the oracle: behind race-line opponents the planner computes something else with the prediction
     along the track over 2 s than with the ingested point, and mode 0 computes what the loop without a predictor computes;
  5. the entry points check their arguments without a device (tools/fakehip/sim_predictor_args.py on the plain stand-in build).
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import planner_replay as pr
import sim_predictor_util as pu
import test_gpu_sim_differential as gd
from graphbasedlocaltrajectoryplanner_amd import sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "sim_predictor_shim.cpp")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("predictor") / "sim_predictor_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, SHIM], check=True)
    lib = ctypes.CDLL(so)
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.predictor_eval_host.argtypes = [P, P, P, P, I, I, P, I, P, P, P]
    return lib


@pytest.fixture(scope="module")
def table():
    return sim.RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


@pytest.fixture(scope="module")
def track():
    return np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz"))


@pytest.fixture(scope="module")
def c2_start():
    return pr.load_ticks("c2")[0]['start']


def header(shim, tab, c):
    """A case by the compiled header, in the form of sim_predictor_util.mirror."""
    n, K = c["objs"].shape[0], c["K"]
    par, objs = np.array(c["params"], float), np.ascontiguousarray(np.concatenate((c["objs"], np.zeros((1, 5)))))
    pts, oc, rec = np.zeros((n + 1, K, 2)), np.zeros(n + 1, np.int32), np.zeros(sim.PREDICTOR_DOUBLES)
    shim.predictor_eval_host(par.ctypes.data, tab.s_rl.ctypes.data, tab.x.ctypes.data, tab.y.ctypes.data, len(tab.s_rl), K, objs.ctypes.data, n,
                             pts.ctypes.data, oc.ctypes.data, rec.ctypes.data)
    return dict(pos=np.concatenate((c["objs"][:, None, :2], pts[:n]), axis=1), outcome=oc[:n].copy(), rec=rec)


# ---- 1. header against mirror -------------------------------------------------------------------------------------------------------------
def test_header_equals_the_mirror_bit_for_bit(shim, table):
    cs, groups = pu.cases(table)
    ref = [pu.mirror(table, c) for c in cs]
    for i, (c, r) in enumerate(zip(cs, ref)):
        pu.compare(header(shim, table, c), r, "case %d" % i)
    total = np.sum([r["rec"] for r in ref], axis=0)
    print("case list: %d cases, %d objects; counters %s" % (len(cs), int(total[1]), dict(zip([f[0] for f in sim.PREDICTOR_FIELDS], total.tolist()))))
    assert np.all(total[[2, 3, 4, 5, 6, 8, 10]] > 0)         # every outcome a Monteblanco object can have, and wraps
    dtab = pu.dup_table(table)
    assert dtab.x[pu.DUP_ROW] == dtab.x[pu.DUP_ROW + 1] and dtab.s_rl[pu.DUP_ROW] == dtab.s_rl[pu.DUP_ROW + 1]
    for i, c in enumerate(pu.dup_cases(dtab)):
        pu.compare(header(shim, dtab, c), pu.mirror(dtab, c), "duplicated row, case %d" % i)
    # a table of two coinciding rows has no segment at all: straight line, counted as such
    point = sim.RaceLineTable([1.0, 1.0], [5.0, 5.0], [7.0, 7.0], [0.0, 0.0], [10.0, 10.0])
    c = pu.case(2, [[4.0, 7.5, 4.5, 7.5, 12.0]])
    r = pu.mirror(point, c)
    pu.compare(header(shim, point, c), r, "no segment")
    assert r["outcome"].tolist() == [sim.PRED_STRAIGHT_NOSEG] and r["rec"][7] == 1


def test_every_boundary_group_shows_its_outcome(table):
    cs, groups = pu.cases(table)
    ref = [pu.mirror(table, c) for c in cs]
    n = len(table.s_rl)
    m = pu.model(table, 4)

    def oc(name):
        return [ref[i]["outcome"].tolist() for i in groups[name]]
    T = sim.PRED_TRACK
    assert all(o == T for l in oc("on a row") for o in l)
    # rows 0 and n - 1: the objects are nearest to them and the one existing segment is taken
    for name, row, seg in (("row 0", 0, 0), ("row n-1", n - 1, n - 2)):
        for o in cs[groups[name][0]]["objs"]:
            assert m.nearest(o[0], o[1]) == row and m.project(0, *o)[3] == seg, name
    # equidistant: the vertex itself ties exactly (q2 = 0 on both) and goes to the lower segment
    c = cs[groups["equidistant"][0]]
    i_star = m.nearest(c["objs"][0][0], c["objs"][0][1])
    lo, hi = m._candidate(i_star - 1, c["objs"][0][0], c["objs"][0][1]), m._candidate(i_star, c["objs"][0][0], c["objs"][0][1])
    assert lo[1] == hi[1] == 0.0 and m.project(0, *c["objs"][0])[3] == i_star - 1
    for o in c["objs"][1:]:                                   # outside the bend both feet clamp: t = 1 below, t = 0 above
        i_star = m.nearest(o[0], o[1])
        assert m._candidate(i_star - 1, o[0], o[1])[0] == 1.0 and m._candidate(i_star, o[0], o[1])[0] == 0.0
    c = cs[groups["clamp"][0]]
    assert m._candidate(0, *c["objs"][0][:2])[0] == 0.0 and m._candidate(n - 2, *c["objs"][1][:2])[0] == 1.0
    assert oc("d_max") == [[T], [sim.PRED_STRAIGHT_DMAX], [T]]
    assert oc("direction") == [[sim.PRED_STRAIGHT_DIR, T]]
    assert oc("still") == [[sim.PRED_INGESTED] * 4, [sim.PRED_STILL] * 3 + [sim.PRED_STRAIGHT_MODE], [sim.PRED_STILL] * 3 + [T]]
    # the wrap: exactly on the end the point wraps to s = 0, below S[0]: the table's first row; one double below it does not wrap
    on, below, under = (ref[groups[k][0]] for k in ("wrap / on the end", "wrap / below the end", "wrap / below S[0]"))
    assert on["rec"][10] == 1 and below["rec"][10] == 0 and under["rec"][10] == 1
    d = m.project(0, *cs[groups["wrap / on the end"][0]]["objs"][0])[2]
    assert abs(on["pos"][0, 1, 0] - table.x[0]) <= 2 * abs(d) + 1e-9 and abs(below["pos"][0, 1, 0] - table.x[-1]) <= 2 * abs(d) + 1e-6
    assert abs(under["pos"][0, 1, 0] - table.x[0]) <= 2 * abs(d) + 1e-9
    assert ref[groups["wrap / below S[0]"][1]]["rec"][10] >= 1
    seen = {(len(cs[i]["objs"]), cs[i]["K"]) for i in groups["counts"]}
    assert {(0, 4), (1, 4), (13, 5), (16, 8), (43, 3), (96, 1), (64, 2)} <= seen


# ---- 2. sanitizers ------------------------------------------------------------------------------------------------------------------------
def test_the_stand_alone_program_runs_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sim_predictor_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DSIM_PREDICTOR_SHIM_MAIN", "-o", exe, SHIM], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert p.returncode == 0 and "predictor shim:" in p.stdout, p.stdout[-3000:]


# ---- 3. properties of the mirror ----------------------------------------------------------------------------------------------------------
def test_an_opponent_on_the_race_line_is_predicted_onto_the_race_line(table):
    """An opponent of sim.opponent_step sits at (X(s), Y(s)) of the table's own interpolation. Mode 2 with relax = 0 puts point j at
    (X(s_j) - d uy, Y(s_j) + d ux), s_j = s0 + v t_j, where X(s_j), Y(s_j) are the SAME interpolation: the distance to it is |d| up to
    the rounding of the two products and two sums, and d is what rounding leaves of a point on the line.
    The bound on |d|: the interpolated coordinate c = slope (s - S_a) + C_a carries at most 1.5 ulp(C) (the product rounds to half an ulp
    of a value below |C_b - C_a| <= ulp-scale of C, the quotient likewise, the sum to half an ulp of C), C = the table's largest
    |coordinate|; the offset d = (ex gy - ey gx) / L with |g| <= L sees that error once per coordinate (sqrt 2 together) plus four
    roundings relative to L = the longest segment: |d| <= D = 1.5 sqrt(2) ulp(C) + 4 eps L, doubled for the rounding of gx, gy themselves.
    The point then adds half an ulp(C) per coordinate: distance <= |d| (1 + 4 eps) + ulp(C)."""
    lists = table.lists()
    eps = 2.0 ** -52
    C = float(max(np.max(np.abs(table.x)), np.max(np.abs(table.y))))
    L = float(np.max(np.hypot(np.diff(table.x), np.diff(table.y))))
    D = 2.0 * (1.5 * math.sqrt(2.0) * math.ulp(C) + 4.0 * eps * L)
    K = 4
    m = pu.model(table, K, horizon=3.0, relax=0.0)
    lap = float(table.s_rl[-1])
    worst_d, worst = 0.0, 0.0
    for s in np.concatenate((np.linspace(float(table.s_rl[0]), lap - 1e-3, 97), [lap - 30.0, lap - 5.0])):
        s = float(s)
        j = sim.segment(s, lists[0])
        x, y, v = sim.interp_at(s, lists[0], lists[1], j), sim.interp_at(s, lists[0], lists[2], j), 0.5 * sim.interp_at(s, lists[0], lists[4], j)
        q = min(max(j, 0), len(lists[0]) - 2)
        ex, ey = lists[1][q + 1] - lists[1][q], lists[2][q + 1] - lists[2][q]
        ln = math.hypot(ex, ey)
        obj = (x, y, x + 0.2 * v * ex / ln, y + 0.2 * v * ey / ln, v)
        oc, s0, d, _ = m.project(0, *obj)
        assert oc == sim.PRED_TRACK and abs(d) <= D, (s, oc, d, D)
        assert abs(s0 - s) <= 1e-9 * lap
        worst_d = max(worst_d, abs(d))
        for jj in range(1, K + 1):
            px, py, _ = m.point(0, jj, (oc, s0, d), *obj)
            sj = s0 + v * ((3.0 * jj) / K)
            if sj >= lap:
                sj -= lap
            g = sim.segment(sj, lists[0])
            rx, ry = sim.interp_at(sj, lists[0], lists[1], g), sim.interp_at(sj, lists[0], lists[2], g)
            dist = math.hypot(px - rx, py - ry)
            assert dist <= abs(d) * (1.0 + 4.0 * eps) + math.ulp(C), (s, jj, dist, d)
            worst = max(worst, dist)
    print("largest |d| of an opponent on the line %.3g (bound %.3g); largest distance of a point from the line's own interpolation %.3g" % (worst_d, D, worst))


def test_modes_0_and_1_are_the_written_expressions(table):
    rng = np.random.default_rng(5)
    objs = pu.random_objs(rng, table, 30)
    m1 = pu.model(table, 1, mode=1, horizon=0.2)
    c1 = ((0.2 * 1.0) / 1.0) / 0.2
    assert c1 == 1.0
    pts, ocs = m1.predict(0, objs)
    for o, p, oc in zip(objs, pts, ocs):
        x, y, px, py, v = o
        if oc == sim.PRED_STILL:
            assert p[0, 0] == px and p[0, 1] == py
        else:
            assert oc == sim.PRED_STRAIGHT_MODE and p[0, 0] == x + (px - x) * c1 and p[0, 1] == y + (py - y) * c1
    for K in (1, 4, 8):
        pts, ocs = pu.model(table, K, mode=0, horizon=3.0).predict(0, objs)
        assert set(ocs) == {sim.PRED_INGESTED}
        for o, p in zip(objs, pts):
            assert np.all(p[:, 0] == o[2]) and np.all(p[:, 1] == o[3])
    # straight line at a longer horizon: point j lies (t_j / 0.2) ingestion steps ahead
    pts, _ = pu.model(table, 4, mode=1, horizon=2.0).predict(0, [[1.0, 2.0, 1.5, 2.25, 10.0]])
    assert pts[0].tolist() == [[1.0 + 0.5 * (((2.0 * j) / 4.0) / 0.2), 2.0 + 0.25 * (((2.0 * j) / 4.0) / 0.2)] for j in (1, 2, 3, 4)]
    with pytest.raises(ValueError):
        sim.PredictorModel(1, table, n_points=9)


# ---- 4. the closed loop under the oracle --------------------------------------------------------------------------------------------------
def run_host(monteblanco, oracle_backend, table, c2_start, pkw, ticks):
    sc = gd.Scenario(monteblanco, table, [pu.bend_unit(table, c2_start)])
    loop = pu.host_loop(sc, oracle_backend, None, None, pkw)
    recs = [loop.tick(want_paths=True)[0] for _ in range(ticks)]
    assert not any(r["failed"] for r in recs)
    return recs, loop


def same_tick(a, b):
    ta, tb = a["traj"][0], b["traj"][0]
    return a["sel"] == b["sel"] and a["pos"] == b["pos"] and list(ta) == list(tb) and all(np.array_equal(ta[k][0], tb[k][0]) for k in ta)


def paths_of(r):
    p = r["paths"]
    return p["keys"], p["start_node"], [p["nodes"][k] for k in p["keys"]]


def test_the_prediction_changes_what_the_planner_computes(monteblanco, oracle_backend, table, c2_start):
    ticks = 25
    bare, _ = run_host(monteblanco, oracle_backend, table, c2_start, None, ticks)
    as_ingested, l0 = run_host(monteblanco, oracle_backend, table, c2_start, dict(pu.A_PRED, mode=0), ticks)
    along, l2 = run_host(monteblanco, oracle_backend, table, c2_start, pu.A_PRED, ticks)
    assert all(r["cnt"] == 3 for r in bare)
    # mode 0: the same positions in the mask, the same last position: the planner computes what it computes without a predictor
    assert all(same_tick(a, b) for a, b in zip(bare, as_ingested))
    differ = [k for k, (a, b) in enumerate(zip(as_ingested, along)) if not same_tick(a, b)]
    paths_differ = [k for k, (a, b) in enumerate(zip(as_ingested, along)) if paths_of(a) != paths_of(b)]
    print("ticks whose trajectories differ between mode 0 and mode 2 over 2 s:", differ, "; whose paths differ:", paths_differ)
    print("actions, as ingested:", [r["sel"] for r in as_ingested][::3], "along the track:", [r["sel"] for r in along][::3])
    assert differ and paths_differ, "the prediction along the track changed nothing"
    d0, d2 = l0.predictor.as_dict(), l2.predictor.as_dict()
    assert d0["n_ingested"][0] == 3 * ticks == d2["n_track"][0] + d2["n_still"][0] and d2["n_track"][0] > 0 and d2["ticks"][0] == ticks


# ---- 5. the entry points ------------------------------------------------------------------------------------------------------------------
def test_predictor_entry_points_check_their_arguments_without_a_device():
    """The real library refuses a null fleet; tools/fakehip/sim_predictor_args.py on the stand-in runtime (plain build): every bad argument
    is refused with a message that names it, without allocation or launch; the capacity bound at exactly 192 and above; a failing
    allocation keeps the previous state; k_fleet_sim_predict in k_fleet_sim_compact's place while the predictor is set."""
    import sys
    lib = ctypes.CDLL(os.path.join(ROOT, "graphbasedlocaltrajectoryplanner_amd", "csrc", "libltpl_hip.so"))
    assert lib.ltpl_fleet_sim_predictor(None, None) == 1 and lib.ltpl_fleet_sim_predictor_read(None, None, 11) == 1
    assert lib.ltpl_fleet_sim_predictor_eval(None, 0, 1, *([None] * 6)) == 1
    env = dict(os.environ, FAKEHIP_SAN="none", LTPL_NO_SELFTEST="1")
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "sim_predictor_args.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and "sim predictor args OK" in p.stdout, p.stdout[-3000:]
    assert "launches per tick" in p.stdout, p.stdout[-3000:]


def test_python_binding_and_header_declare_the_entry_points():
    from graphbasedlocaltrajectoryplanner_amd import fleet
    for name in ("sim_predictor", "sim_predictor_read", "sim_predictor_eval"):
        assert callable(getattr(fleet.Fleet, name)), name
    with open(os.path.join(ROOT, "include", "ltpl_hip.h")) as fh:
        hdr = fh.read()
    for name in ("ltpl_fleet_sim_predictor(", "ltpl_fleet_sim_predictor_read(", "ltpl_fleet_sim_predictor_eval(", "#define LTPL_ABI_VERSION 9",
                 "#define LTPL_FLEET_SIM_PREDICTOR_DOUBLES 11", "#define LTPL_FLEET_SIM_PREDICTOR_MAX_POINTS 8"):
        assert name in hdr, name
    assert sim.PREDICTOR_DOUBLES == 11 == len(sim.PREDICTOR_FIELDS) and fleet.PREDICTOR_FIELDS is sim.PREDICTOR_FIELDS
    assert set(sim.PREDICTOR_PARAMS) | {"n_points"} == set(sim.PREDICTOR_DEFAULTS)
