"""
TEST INFRASTRUCTURE (no test functions): the prediction model of the fleet's simulation (ltpl_fleet_sim_predictor; csrc/fleet_predict.hpp,
sim.PredictorModel) for tests/test_sim_predictor_host.py and tests/test_gpu_sim_predictor.py --

  ``cases``            the case list both files evaluate on a race-line table (header against mirror on the CPU, the device's hook against
                       the mirror on the GPU). A case is ONE evaluation of one planner: n_points, parameters and the objects
                       [x, y, px, py, v]; ``groups`` names the case indices of every boundary;
  ``dup_table``        the Monteblanco table with one row duplicated (a segment of length 0) and its cases;
  ``mirror``           what sim.PredictorModel makes of a case;
  ``Predicting``       mixin over a tracking host loop (sim_tracker_util.Tracking): a sim.PredictorModel behind sensor and tracker, in the
                       device's place: every vehicle's position array is rewritten to own position + K points before the planner sees it;
  ``scenarios``        the scenarios of the device's seated lockstep with their sensor, tracker and predictor parameters, ``host_loop``
                       their host loop.
"""
import math

import numpy as np

import sim_loop as sl
import sim_tracker_util as tu
from graphbasedlocaltrajectoryplanner_amd import sim

INF = float("inf")
NAN = float("nan")
PAR = dict(mode=2, horizon=2.0, relax=0.0, d_max=INF)


def model(table, n_points, n=1, **par):
    return sim.PredictorModel(n, table, n_points=n_points, **dict(PAR, **par))


def seg_obj(tab, a, t, d, v, along=1.0, step=None):
    """An object on segment (a, a + 1) of the table at parameter ``t`` and lateral offset ``d`` (left positive), moving along the segment
    (``along`` = -1: against it) at speed ``v``: its 0.2 s point lies ``step`` (default 0.2 v) m ahead."""
    ex, ey = float(tab.x[a + 1] - tab.x[a]), float(tab.y[a + 1] - tab.y[a])
    ln = math.hypot(ex, ey)
    ux, uy = ex / ln, ey / ln
    x, y = float(tab.x[a]) + t * ex - d * uy, float(tab.y[a]) + t * ey + d * ux
    w = along * (0.2 * v if step is None else step)
    return [x, y, x + w * ux, y + w * uy, float(v)]


def find_v(s0, t_j, target):
    """A speed v with s0 + v t_j == target exactly (searched among the neighbours of (target - s0) / t_j)."""
    v = (target - s0) / t_j
    for cand in [v] + [f(v, k) for k in range(1, 64) for f in (lambda a, k: _step(a, k), lambda a, k: _step(a, -k))]:
        if s0 + cand * t_j == target:
            return cand
    raise AssertionError("no speed reaches %r from %r" % (target, s0))


def _step(a, k):
    for _ in range(abs(k)):
        a = math.nextafter(a, INF if k > 0 else -INF)
    return a


def case(K, objs, **par):
    p = dict(PAR, **par)
    return dict(K=int(K), params=[float(p["mode"]), float(p["horizon"]), float(p["relax"]), float(p["d_max"])],
                objs=np.asarray(objs, np.float64).reshape(-1, 5))


def random_objs(rng, tab, n, spread=6.0):
    """``n`` seeded objects around the race line: most within ``spread`` m of it and moving roughly along it, some far off, some
    against the track, some standing."""
    out = []
    rows = len(tab.s_rl)
    for _ in range(n):
        a = int(rng.integers(0, rows - 1))
        kind = rng.integers(0, 10)
        d = float(rng.uniform(-spread, spread)) if kind < 8 else float(rng.uniform(-60.0, 60.0))
        v = 0.0 if kind == 7 else float(rng.uniform(0.5, 90.0))
        o = seg_obj(tab, a, float(rng.uniform(0.0, 1.0)), d, v, along=-1.0 if kind == 6 else 1.0)
        o[2] += float(rng.uniform(-0.3, 0.3))
        o[3] += float(rng.uniform(-0.3, 0.3))
        out.append(o)
    return out


def cases(tab, n_random=40, seed=20261021):
    """(cases, groups) on table ``tab`` (a sim.RaceLineTable): ``groups`` = {name: [case indices]}."""
    out, groups = [], {}
    n = len(tab.s_rl)
    S_end, S0 = float(tab.s_rl[-1]), float(tab.s_rl[0])

    def add(name, *cs):
        groups.setdefault(name, []).extend(range(len(out), len(out) + len(cs)))
        out.extend(cs)

    def on_row(i, v=20.0):
        a = min(i, n - 2)
        o = seg_obj(tab, a, 0.0, 0.0, v)
        o[0], o[1] = float(tab.x[i]), float(tab.y[i])
        o[2], o[3] = o[0] + (o[2] - float(tab.x[a])), o[1] + (o[3] - float(tab.y[a]))
        return o
    mid = n // 3
    # exactly on a row; nearest to row 0 and to row n - 1 (the one existing segment is the only candidate there)
    add("on a row", case(4, [on_row(mid)]), case(1, [on_row(mid + 1), on_row(mid + 7)]))
    add("row 0", case(4, [on_row(0), seg_obj(tab, 0, 0.2, 1.0, 30.0)]))
    add("row n-1", case(4, [on_row(n - 1), seg_obj(tab, n - 2, 0.9, -1.0, 30.0)]))
    # equidistant from both neighbour segments: on the vertex, and on the bisector outside the bend (both feet clamp to the vertex)
    bend = int(np.argmax(np.abs(np.diff(np.unwrap(np.arctan2(np.diff(tab.y), np.diff(tab.x))))))) + 1
    e0 = np.array([tab.x[bend] - tab.x[bend - 1], tab.y[bend] - tab.y[bend - 1]])
    e1 = np.array([tab.x[bend + 1] - tab.x[bend], tab.y[bend + 1] - tab.y[bend]])
    u0, u1 = e0 / np.linalg.norm(e0), e1 / np.linalg.norm(e1)
    turn = float(u0[0] * u1[1] - u0[1] * u1[0])
    outward = (u0 - u1) / np.linalg.norm(u0 - u1) if np.linalg.norm(u0 - u1) > 0 else np.array([-u0[1], u0[0]])
    if turn == 0.0:
        outward = np.array([-u0[1], u0[0]])
    eq = []
    for w in (0.0, 0.5, 2.0):
        x, y = float(tab.x[bend] + w * outward[0]), float(tab.y[bend] + w * outward[1])
        eq.append([x, y, x + 4.0 * u1[0], y + 4.0 * u1[1], 20.0])
    add("equidistant", case(3, eq))
    # the foot point clamps at t = 0 (behind row 0) and at t = 1 (beyond row n - 1)
    add("clamp", case(2, [seg_obj(tab, 0, -0.5, 0.7, 25.0), seg_obj(tab, n - 2, 1.5, -0.7, 25.0)]))
    # |d| == d_max stays along the track; the next double above it falls back
    o = seg_obj(tab, mid, 0.4, 1.75, 30.0)
    d = model(tab, 4).project(0, *o)[2]
    assert d != 0.0
    add("d_max", case(4, [o], d_max=abs(d)), case(4, [o], d_max=math.nextafter(abs(d), 0.0)),
        case(4, [seg_obj(tab, mid, 0.4, -1.75, 30.0)], d_max=abs(model(tab, 4).project(0, *seg_obj(tab, mid, 0.4, -1.75, 30.0))[2])))
    # against the track; exactly across it (the product is not negative: stays)
    add("direction", case(4, [seg_obj(tab, mid, 0.5, 0.5, 20.0, along=-1.0), seg_obj(tab, mid, 0.5, 0.5, 20.0, step=0.0)]))
    # v = 0, v = NaN, v < 0 in every mode
    still = [seg_obj(tab, mid, 0.5, 0.5, 0.0, step=1.0), seg_obj(tab, mid, 0.5, 0.5, NAN, step=1.0), seg_obj(tab, mid, 0.5, 0.5, -3.0, step=1.0),
             seg_obj(tab, mid, 0.5, 0.5, 10.0)]
    add("still", *[case(3, still, mode=m) for m in (0, 1, 2)])
    # s_j exactly on S[n - 1] (wraps to 0: below S[0]), just below it (no wrap: the last segment), and below S[0] after the wrap
    o = seg_obj(tab, n - 6, 0.5, 0.0, 1.0)
    s0 = model(tab, 1).project(0, *o)[1]
    T = 1.0
    for name, target in (("wrap / on the end", S_end), ("wrap / below the end", math.nextafter(S_end, 0.0))):
        v = find_v(s0, T, target)
        add(name, case(1, [o[:4] + [v]], horizon=T))
    add("wrap / below S[0]", case(1, [o[:4] + [(S_end - s0 + 0.5 * S0) / T]], horizon=T), case(8, [o[:4] + [(S_end - s0) / T]], horizon=2.0 * T))
    # relax, K = 1 and K = 8, modes 0 and 1
    rng = np.random.default_rng(seed)
    add("modes", *[case(K, random_objs(rng, tab, 9), mode=m, horizon=h, relax=r) for K in (1, 8) for m in (0, 1, 2) for h, r in ((0.2, 0.0), (3.0, 0.5), (1.0, 1.0))])
    # object counts: none, one, the pass edges of cnt K pairs (65, 128, 129) and the capacity edge cnt (1 + K) = 192
    for cnt, K in ((0, 4), (1, 4), (13, 5), (16, 8), (43, 3), (96, 1), (64, 2), (32, 5), (63, 1), (65, 1)):
        add("counts", case(K, random_objs(rng, tab, cnt), relax=0.25, d_max=8.0))
    for _ in range(n_random):
        add("random", case(int(rng.integers(1, 9)), random_objs(rng, tab, int(rng.integers(0, 40))), mode=int(rng.integers(0, 3)),
                           horizon=float(rng.uniform(0.1, 5.0)), relax=float(rng.choice([0.0, 0.3, 1.0])), d_max=float(rng.choice([INF, 4.0, 0.0]))))
    return out, groups


DUP_ROW = 100


def dup_table(tab, row=DUP_ROW):
    """``tab`` with row ``row`` duplicated: a segment of length 0 between rows ``row`` and ``row + 1``."""
    idx = list(range(row + 1)) + list(range(row, len(tab.s_rl)))
    return sim.RaceLineTable(tab.s_rl[idx], tab.x[idx], tab.y[idx], tab.psi[idx], tab.vel_rl[idx])


def dup_cases(dtab, row=DUP_ROW, seed=7):
    """Cases around the duplicated row of ``dup_table``'s table: objects nearest to either copy, on it, and points that land on it."""
    rng = np.random.default_rng(seed)
    objs = [seg_obj(dtab, row - 1, 1.0, 0.5, 20.0), seg_obj(dtab, row - 1, 0.98, -0.5, 20.0), seg_obj(dtab, row + 1, 0.02, 0.5, 20.0),
            seg_obj(dtab, row + 1, 0.0, 0.0, 20.0), seg_obj(dtab, row - 2, 0.5, 0.3, 25.0)]
    o = seg_obj(dtab, row - 3, 0.5, 0.4, 1.0)
    s0 = model(dtab, 1).project(0, *o)[1]
    land = o[:4] + [find_v(s0, 1.0, float(dtab.s_rl[row]))]
    return [case(4, objs), case(1, [land], horizon=1.0), case(8, objs + [land], relax=0.5, d_max=0.45)] + \
        [case(3, [seg_obj(dtab, row + int(rng.choice([-3, -2, -1, 1, 2])), float(rng.uniform(0, 1)), float(rng.uniform(-2, 2)), float(rng.uniform(1, 60))) for _ in range(20)])]


def mirror(tab_or_model, c):
    """dict(pos [n, 1 + K, 2], outcome [n], rec [11]) of a case by sim.PredictorModel."""
    par = dict(zip(sim.PREDICTOR_PARAMS, c["params"]))
    m = sim.PredictorModel(1, tab_or_model, n_points=c["K"], **par)
    objs = c["objs"].tolist()
    pts, ocs = m.predict(0, objs)
    return dict(pos=np.concatenate((c["objs"][:, None, :2], pts), axis=1), outcome=np.asarray(ocs, np.int32), rec=m.counters(objs, ocs))


def equal_bits(a, b):
    return tu.equal_bits(a, b)


def compare(got, ref, what):
    """``got``, ``ref``: dicts in the form of ``mirror``; bit for bit."""
    assert list(got["outcome"]) == list(ref["outcome"]), "%s: outcomes %s, mirror %s" % (what, list(got["outcome"]), list(ref["outcome"]))
    assert equal_bits(got["pos"], ref["pos"]), "%s: positions differ; largest deviation %g" % (
        what, float(np.nanmax(np.abs(np.asarray(got["pos"]) - np.asarray(ref["pos"])))) if np.asarray(ref["pos"]).size else 0.0)
    assert equal_bits(got["rec"], ref["rec"]), "%s: counters %s, mirror %s" % (what, got["rec"], ref["rec"])


# ---- the predicting host loop -------------------------------------------------------------------------------------------------------------
class Predicting(tu.Tracking):
    """Mixin: ``predictor`` = a sim.PredictorModel over THIS loop's planners (or None: the loop of the base class). Behind sensor and
    tracker every vehicle's position array becomes [own, point 1 .. point K]; the records gain ``pred_outcome``."""

    def init_predictor(self, predictor):
        self.predictor = predictor

    def sense(self, h, veh):
        out = super(Predicting, self).sense(h, veh)
        if self.predictor is None:
            return out
        objs = [(float(v[2][0, 0]), float(v[2][0, 1]), float(v[2][1, 0]), float(v[2][1, 1]), float(v[1])) for v in out]
        pts, ocs = self.predictor.step(h, objs)
        new = [(v[0], v[1], np.concatenate((np.asarray(v[2], float)[:1], pts[i]), axis=0)) for i, v in enumerate(out)]
        self._rec[h].update(veh=new, cnt=len(new), pred_outcome=list(ocs))
        return new


def _loop_class(base):
    class Loop(Predicting, base):
        def __init__(self, *args, **kw):
            sensor, tick0 = kw.pop("sensor", None), kw.pop("sensor_tick0", 0)
            trackers, ttick0 = kw.pop("trackers", None), kw.pop("tracker_tick0", 0)
            predictor = kw.pop("predictor", None)
            base.__init__(self, *args, **kw)
            self.init_sensor(sensor, tick0)
            self.init_tracker(trackers, ttick0)
            self.init_predictor(predictor)
    Loop.__name__ = "Predicting" + base.__name__
    return Loop


PredictingSimLoop = _loop_class(sl.HostSimLoop)


def host_loop(sc, oracle, sensor_kw, tracker_kw, predictor_kw):
    """The predicting host loop of scenario ``sc`` (test_gpu_sim_differential.Scenario; every planner on the host); a ``*_kw`` of None:
    without that stage."""
    from oracle.planner_host import HostPlannerBackend
    assert sc.hmap == list(range(sc.n))
    backend = HostPlannerBackend(sc.lat)
    sensor = None if sensor_kw is None else sim.SensorModel(sc.n, **sensor_kw)
    trackers = None if tracker_kw is None else tu.trackers_for(tu.slots_of(sc), tracker_kw, sc.dt)
    predictor = None if predictor_kw is None else sim.PredictorModel(sc.n, sc.tab, **predictor_kw)
    loop = PredictingSimLoop(sc.lat, sc.tab, sc.entries, [backend.planner(1, **sc.config) for _ in range(sc.n)], oracle=oracle, dt=sc.dt,
                             n_export=sc.n_export, sensor=sensor, trackers=trackers, predictor=predictor)
    for p in range(sc.n):
        pos, heading, vel, mho = sc.starts[p]
        assert loop.set_start(p, pos, heading, vel, mho)[0], p
        loop.sim_vel(p, **sc.vels[p])
    if max(sc.sizes) > 1:
        loop.sim_race(sc.sizes, length=5.0)
    return loop


def beside_static(table, s, d, v):
    """A static-list object (x, y, theta, v, length) ``d`` m to the left of the race line at arc length ``s``, heading along it at ``v``."""
    pos, h = sl.race_line_pose(table, s)
    f = (-math.sin(h), math.cos(h))                   # forward of the library's heading (measured from the y axis); left of it: (-f_y, f_x)
    return (pos[0] - d * f[1], pos[1] + d * f[0], h, float(v), 4.0)


def bend_unit(table, start, ahead=(200.0, -40.0), scale=(0.5, 0.3), beside=(30.0, -4.0, 15.0), start_vel=15.0):
    """Scenario A: the ego on a flying start at ``start_vel``; two opponents on the race line, one far ahead and one behind it (any
    race-line object within the planning horizon leaves the planner nothing but 'follow'), and one car ``beside`` = (m ahead, lateral
    offset to the left, speed) the race line that drives along it: as ingested the planner overtakes it on the free side; with
    relax > 0 its prediction merges onto the race line in front of the ego and blocks the overtaking path."""
    import test_gpu_sim_differential as gd
    i0 = int(np.argmin((table.x - start['pos'][0]) ** 2 + (table.y - start['pos'][1]) ** 2))
    s_ego = float(table.s_rl[i0])
    opp = [(s_ego + a, s, 5.0) for a, s in zip(ahead, scale)]
    static = [] if beside is None else [beside_static(table, s_ego + beside[0], beside[1], beside[2])]
    e = dict(opponents=opp, static=static, pref=sl.DEFAULT_PREF, pos_est=tuple(start['pos']), vel_est=start_vel, zone_gids=[])
    return gd.single("bend", dict(entry=e, vel=sl.C2_VEL, start_vel=start_vel), start)


A_PRED = dict(n_points=4, mode=2, horizon=2.0, relax=0.5, d_max=INF)


def scenarios(table, track, start):
    """[(name, units, sensor keywords or None, tracker keywords or None, predictor keywords, ticks)]."""
    import test_gpu_sim_differential as gd
    import test_gpu_sim_noise as gn
    singles = gn.singles(table, track, start)
    lossy = dict(range=300.0, fov_deg=360.0, r_near=0.0, occl=0.0, p_drop=0.2, seed=np.uint64(91))
    entries, poses = sl.big_race(table, 2, gap=25.0, own=[(250.0, 0.3, 5.0)])
    for e in entries:                                 # a car 4 m beside the race line ahead of both: beyond d_max, predicted straight
        e["static"] = [beside_static(table, 120.0, -4.0, 10.0)]
    race2 = gd.race_unit("race2", entries, poses)
    return [("A: race-line opponents, along the track", [bend_unit(table, start)], None, None, A_PRED, 25),
            ("B: race of 2 behind sensor and tracker, d_max", [race2], lossy, dict(gate=6.0, w_pos=0.5, w_vel=0.5, n_confirm=2, n_coast=3),
             dict(n_points=3, mode=2, horizon=1.5, relax=0.5, d_max=0.5), 25),
            ("C: mixed modes", singles, None, None, dict(n_points=3, mode=[0, 1, 2], horizon=[1.0, 0.8, 2.5], relax=[0.0, 0.0, 1.0], d_max=[INF, INF, 3.0]), 20)]
