"""
GPU: friction maps resident on the device (ltpl_fleet_friction / _scale / _rows, csrc/fleet_friction.hpp; the third source of friction
rows in stage A of the fleet's velocity stage, csrc/fleet_core.hpp vel_a<X, true>).

  - the lookup kernel against the host mirror ``FrictionGrid.rows``, bit for bit;
  - the map against the ROW form that 'ggmap' and its siblings pin to the reference: a fleet with the map set and a fleet that is handed
    the mirror's rows through gg_rows agree bitwise on every tick, through the backup ticks of 'gridmapdrop' as well;
  - ``sim_run`` reproduces the recordings of the unmodified reference driven with the grid's dict ('gridmap', 'gridmapdrop',
    tools/gen_golden_friction.py) under the rules of tests/test_gpu_fleet_sim.py -- the closed-loop simulation could not run a dict before;
  - mixed fleets, a lockstep differential against the host loop on a race with per-planner grip, the tape, clearing the maps, and the
    emergency profile on a backup plan.
Every test needs an entry point the parent commit does not have.
"""
import os

import numpy as np
import pytest

import friction_replay as fr
import planner_replay as pr
import sim_loop as sl
import test_gpu_fleet_sim as gs
import test_gpu_sim_differential as gd
from graphbasedlocaltrajectoryplanner_amd.friction import FrictionGrid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUPLE = (5.0, 5.0)                  # the constant tuple handed over next to a map: not read for a planner with a map


@pytest.fixture(scope="module")
def hip(monteblanco):
    from graphbasedlocaltrajectoryplanner_amd import _capi
    return _capi.HipBackend(monteblanco)


@pytest.fixture(scope="module")
def race():
    from graphbasedlocaltrajectoryplanner_amd.sim import RaceLineTable
    return RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


@pytest.fixture(scope="module")
def grid():
    return fr.load_grid()


def new_fleet(hip, n, **cfg):
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    return Fleet(hip, n, **cfg)


# ---- the lookup ---------------------------------------------------------------------------------------------------------------------
def lookup_points(g, n, seed):
    """``n`` points: every node, points on cell borders (one coordinate on a node line), points outside on all four sides and far
    outside, the rest uniform over the grid plus a margin."""
    rng = np.random.default_rng(seed)
    x1, y1 = g.x0 + g.dx * (g.nx - 1), g.y0 + g.dy * (g.ny - 1)
    ix, iy = np.meshgrid(np.arange(g.nx), np.arange(g.ny))
    nodes = np.column_stack((g.x0 + g.dx * ix.reshape(-1), g.y0 + g.dy * iy.reshape(-1)))
    m = 2000
    bx = np.column_stack((g.x0 + g.dx * rng.integers(0, g.nx, m), rng.uniform(g.y0, y1, m)))
    by = np.column_stack((rng.uniform(g.x0, x1, m), g.y0 + g.dy * rng.integers(0, g.ny, m)))
    w, h = x1 - g.x0, y1 - g.y0
    out = np.concatenate([np.column_stack((g.x0 - rng.uniform(0.0, w, m), rng.uniform(g.y0 - h, y1 + h, m))),
                          np.column_stack((x1 + rng.uniform(0.0, w, m), rng.uniform(g.y0 - h, y1 + h, m))),
                          np.column_stack((rng.uniform(g.x0 - w, x1 + w, m), g.y0 - rng.uniform(0.0, h, m))),
                          np.column_stack((rng.uniform(g.x0 - w, x1 + w, m), y1 + rng.uniform(0.0, h, m))),
                          np.array([[-1e300, 1e300], [1e300, -1e300], [g.x0, 1e18], [-1e18, y1]])])
    pts = np.concatenate([nodes, bx, by, out])
    assert len(pts) < n
    rest = np.column_stack((rng.uniform(g.x0 - 0.1 * w, x1 + 0.1 * w, n - len(pts)), rng.uniform(g.y0 - 0.1 * h, y1 + 0.1 * h, n - len(pts))))
    pts = np.concatenate([pts, rest])
    ins = g.inside(pts)
    assert ins.sum() > n // 2 and (~ins).sum() > 4 * m
    return pts


def test_friction_rows_equal_the_mirror_bit_for_bit(hip, grid):
    rng = np.random.default_rng(17)
    small = FrictionGrid(3.0, -7.0, 0.37, 12.5, rng.uniform(1.0, 9.0, (2, 2)), rng.uniform(1.0, 9.0, (2, 2)))       # the minimum size
    odd = FrictionGrid(-1.0e3, 2.0e3, 3.3, 0.7, rng.uniform(0.5, 12.0, (31, 57)), rng.uniform(0.5, 12.0, (31, 57)))
    maps = [grid, small, odd]
    fleet = new_fleet(hip, 2)
    fleet.friction(maps, map_idx=[0, -1])
    for m, (g, scale) in enumerate(zip(maps, (1.0, 0.3, 0.77))):
        pts = lookup_points(g, 100000, 40 + m)
        got, exp = fleet.friction_rows(m, pts, scale), g.rows(pts, scale)
        assert got.shape == exp.shape == (100000, 2)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, "map %d: %d values differ, first at point %s: device %r mirror %r" % (
            m, len(bad), pts[bad[0, 0]], got[tuple(bad[0])], exp[tuple(bad[0])])
    fleet.close()


# ---- per-call fleet: map against rows --------------------------------------------------------------------------------------------------
def drive_map_against_rows(hip, lat, ticks, grid, n_ticks, what):
    """Fleet A drives the recording with the map set (constant tuple in the call), fleet B gets the mirror's rows of ITS paths through
    gg_rows: trajectories, digests and error words bitwise equal on every tick; both follow the recording."""
    n = 2
    a, b = new_fleet(hip, n), new_fleet(hip, n)
    a.friction(grid, scale=ticks[0]['grid_scale'])
    st = ticks[0]['start']
    for f in (a, b):
        for p in range(n):
            f.set_start(p, st['pos'], st['heading'], st['vel'], st['max_heading_offset'])
    seen, scale = set(), ticks[0]['grid_scale']
    for t in ticks[:n_ticks]:
        w = "%s tick %d" % (what, t['tick'])
        if t['grid_scale'] != scale:
            scale = t['grid_scale']
            a.friction_scale(scale)
        veh, zg, va = pr.vehicles_of_tick(t), pr.zone_gids_of_tick(lat, t), t['vel_args']
        kw = dict(vel_max=va['vel_max'], gg_scale=va['gg_scale'], ax_max_machines=va['ax_max_machines'], safety_d=va['safety_d'],
                  incl_emerg_traj=va['incl_emerg_traj'])
        for f in (a, b):
            f.calc_paths([t['action_id_sel']] * n, [t['t']] * n, [veh] * n, [zg] * n)
        a.calc_vel_profile([t['pos_est']] * n, va['vel_est'], local_gg=TUPLE, **kw)
        rows = [grid.local_gg(b.paths(p)['path_param'], scale) for p in range(n)]
        pr.assert_close_rel(rows[0][b.paths(0)['keys'][0]][0], va['local_gg_first'], what="%s: rows of the first key" % w)
        b.calc_vel_profile([t['pos_est']] * n, va['vel_est'], local_gg=rows, **kw)
        da, db = a.digest(), b.digest()
        assert np.array_equal(da, db), "%s: digests differ at %s" % (w, np.argwhere(da != db)[:4])
        assert np.all(da[:, 0] == 0), "%s: error words %s" % (w, da[:, 0])
        for p in range(n):
            (ta, ia, ra), (tb, ib, rb) = a.trajectories(p), b.trajectories(p)
            assert list(ta.keys()) == list(tb.keys()) and ia == ib and ra['cut_index_pos'] == rb['cut_index_pos'], w
            for k in ta:
                assert np.array_equal(ta[k][0], tb[k][0]), "%s planner %d / %s" % (w, p, k)
        pr.check_trajectories(ta, ia, ra, t, w)
        seen.update(ta.keys())
    a.close(); b.close()
    return seen


def test_map_equals_rows_per_call_on_gridmap(hip, monteblanco, grid):
    seen = drive_map_against_rows(hip, monteblanco, pr.load_ticks("gridmap"), grid, 500, "gridmap")
    assert {"follow", "emergency"} <= seen and seen & {"left", "right"}, seen


def test_map_equals_rows_per_call_on_gridmapdrop_through_the_backup_ticks(hip, monteblanco, grid):
    ticks = pr.load_ticks("gridmapdrop")
    assert ticks[279]['grid_scale'] == 1.0 and ticks[280]['grid_scale'] == 0.3
    seen = drive_map_against_rows(hip, monteblanco, ticks, grid, 400, "gridmapdrop")
    assert {"straight", "emergency"} <= seen, seen


# ---- the closed-loop simulation -------------------------------------------------------------------------------------------------------
def set_vel(fleet, recs, groups_idx, k):
    """``test_gpu_fleet_sim.set_vel`` for recordings of which some were made with a dict (no tuple recorded: ``TUPLE``)."""
    n = fleet.n_scen
    cols = {key: [None] * n for key in ("vel_max", "gg_scale", "safety_d", "incl_emerg_traj")}
    lgg, tab_idx, tables = [TUPLE] * n, [0] * n, []
    for r, idx in zip(recs, groups_idx):
        va = r[k]['vel_args']
        tables.append(np.asarray(va["ax_max_machines"], float).reshape(-1, 2))
        for p in idx:
            for key in cols:
                cols[key][p] = va[key]
            lgg[p] = TUPLE if va.get('local_gg') is None else tuple(va['local_gg'])
            tab_idx[p] = len(tables) - 1
    cols["incl_emerg_traj"] = [bool(e) for e in cols["incl_emerg_traj"]]
    fleet.sim_vel(local_gg=lgg, ax_tables=tables, ax_table_idx=tab_idx, **cols)


def cuts_of(recs, n_ticks):
    """Runs are split only where the sim_vel arguments or a grid's scale change."""
    def changed(r, k):
        a, b = r[k - 1], r[k]
        if a.get('grid_scale', 1.0) != b.get('grid_scale', 1.0):
            return True
        va, vb = a['vel_args'], b['vel_args']
        return not all(np.array_equal(np.asarray(va[key]), np.asarray(vb[key])) for key in fr.VEL_KEYS + ("local_gg",)
                       if va.get(key) is not None or vb.get(key) is not None)
    cuts = [0] + [k for k in range(1, n_ticks) if any(changed(r, k) for r in recs)] + [n_ticks]
    return list(zip(cuts[:-1], cuts[1:]))


@pytest.mark.parametrize("name,n,must_see,n_runs", [("gridmap", 3, {"follow", "emergency"}, 4), ("gridmapdrop", 2, {"straight", "emergency"}, 4)])
def test_sim_run_reproduces_the_grid_recordings(hip, monteblanco, race, grid, name, n, must_see, n_runs):
    ticks = pr.load_ticks(name)
    fleet = new_fleet(hip, n)
    gs.start(fleet, [(ticks, range(n))])
    fleet.sim_setup(race, [fr.planner_entry(monteblanco, name, ticks)] * n)
    fleet.friction(grid)
    segs = cuts_of([ticks], len(ticks))
    assert len(segs) == n_runs, segs                   # gridmap: emergency on / off, gg_scale; gridmapdrop: emergency on / off, the grid's scale
    traces = []
    for a, b in segs:
        set_vel(fleet, [ticks], [range(n)], a)
        fleet.friction_scale(ticks[a]['grid_scale'])
        traces.append(fleet.sim_run(b - a)[0])
    seen = gs.check_trace(np.concatenate(traces), ticks, list(range(n)), name)
    assert must_see <= seen, seen
    traj, ids, ref = fleet.trajectories(n - 1)
    pr.check_trajectories(traj, ids, ref, ticks[-1], "%s last tick" % name)
    fleet.close()


def test_mixed_fleet_maps_next_to_constant_tuples(hip, monteblanco, race, grid):
    """One fleet: 'gridmap' planners on map 0, 'c2' planners without a map (map_idx -1), 'gridmapdrop' planners on a SECOND map with another
    scale (the grid's values doubled, scale 0.5: every product is the first map's bit for bit, so the group follows its recording). Each
    group follows its own recording; the c2 group is bitwise the c2 group of the same fleet (same planners, same sim_vel arguments, hence
    the same kernel variants for the three machine tables) that never had a map."""
    T = 400
    names = ("gridmap", "c2", "gridmapdrop")
    recs = [pr.load_ticks(nm)[:T] for nm in names]
    idx = [[0, 3, 6], [1, 4, 7], [2, 5]]
    doubled = FrictionGrid(grid.x0, grid.y0, grid.dx, grid.dy, 2.0 * grid.ax, 2.0 * grid.ay)
    entries = [None] * 8
    for nm, r, ix in zip(names, recs, idx):
        for p in ix:
            entries[p] = gs.planner_entry(monteblanco, "c2", r) if nm == "c2" else fr.planner_entry(monteblanco, nm, r)
    map_idx = np.array([0, -1, 1, 0, -1, 1, 0, -1])

    def scales(k):
        return np.where(map_idx == 1, 0.5 * recs[2][k]['grid_scale'], 1.0)
    fleet = new_fleet(hip, 8)
    gs.start(fleet, list(zip(recs, idx)))
    fleet.sim_setup(race, entries)
    fleet.friction([grid, doubled], map_idx=map_idx, scale=scales(0))
    plain = new_fleet(hip, 8)                          # the same fleet, no map ever (its other planners drive on the constant tuple)
    gs.start(plain, list(zip(recs, idx)))
    plain.sim_setup(race, entries)
    traces, ptraces = [], []
    for a, b in cuts_of(recs, T):
        set_vel(fleet, recs, idx, a)
        fleet.friction_scale(scales(a))
        traces.append(fleet.sim_run(b - a)[0])
        set_vel(plain, recs, idx, a)
        ptraces.append(plain.sim_run(b - a)[0])
    trace, ptrace = np.concatenate(traces), np.concatenate(ptraces)
    for nm, r, ix in zip(names, recs, idx):
        gs.check_trace(trace, r, ix, "mixed " + nm)
    assert np.array_equal(trace[:, idx[1]], ptrace[:, idx[1]], equal_nan=True)
    assert not np.array_equal(trace[:, idx[0]], ptrace[:, idx[0]], equal_nan=True)     # (the map planners do drive differently)
    fleet.close(); plain.close()


def test_maps_set_and_cleared_leave_no_trace(hip, monteblanco, race, grid):
    ticks = pr.load_ticks("c2")
    out = []
    for with_maps in (False, True):
        fleet = new_fleet(hip, 2)
        gs.start(fleet, [(ticks, range(2))])
        fleet.sim_setup(race, [gs.planner_entry(monteblanco, "c2", ticks)] * 2)
        if with_maps:
            fleet.friction([grid, grid], map_idx=[1, 0], scale=[0.5, 0.7])
            assert fleet.friction_rows(1, [[0.0, 0.0]]).shape == (1, 2)
            fleet.friction(None)
        gs.set_vel(fleet, [ticks], [range(2)], 0)
        out.append((fleet.sim_run(80)[0], fleet.digest(), fleet.sim_state()))
        fleet.close()
    (ta, da, sa), (tb, db, sb) = out
    assert np.array_equal(ta, tb, equal_nan=True) and np.array_equal(da, db)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    gs.check_trace(tb, ticks, [0, 1], "cleared maps")


def test_maps_cleared_after_a_run_equal_rows_then_tuples(hip, monteblanco, grid):
    """Clearing AFTER ticks on the map. Fleet A drives 'gridmap' on the map for 150 ticks, clears the maps (n_maps = 0) and drives on with
    the call's constant tuple; fleet B is handed the mirror's rows for the same 150 ticks and the tuple from then on. Digests and
    trajectories are bitwise equal on every tick, across the clearing and through the ticks in which a planner's memory still holds
    rows of the time on the map. (Both fleets keep the rows form of their brake / emergency launches from the first tick with rows on:
    a backup plan carries its own rows. The emergency profile is asked for on ticks 100 .. 199, on both sides of the clearing.)"""
    K, T, n = 150, 260, 2
    ticks = pr.load_ticks("gridmap")
    a, b = new_fleet(hip, n), new_fleet(hip, n)
    a.friction(grid)
    st = ticks[0]['start']
    for f in (a, b):
        f.set_start_range(0, n, st['pos'], st['heading'], st['vel'], st['max_heading_offset'])
    for t in ticks[:T]:
        w = "tick %d" % t['tick']
        if t['tick'] == K:
            a.friction(None)
        veh, zg, va = pr.vehicles_of_tick(t), pr.zone_gids_of_tick(monteblanco, t), t['vel_args']
        kw = dict(vel_max=va['vel_max'], gg_scale=va['gg_scale'], ax_max_machines=va['ax_max_machines'], safety_d=va['safety_d'],
                  incl_emerg_traj=va['incl_emerg_traj'])
        for f in (a, b):
            f.calc_paths([t['action_id_sel']] * n, [t['t']] * n, [veh] * n, [zg] * n)
        a.calc_vel_profile([t['pos_est']] * n, va['vel_est'], local_gg=TUPLE, **kw)
        lgg = [grid.local_gg(b.paths(p)['path_param']) for p in range(n)] if t['tick'] < K else TUPLE
        b.calc_vel_profile([t['pos_est']] * n, va['vel_est'], local_gg=lgg, **kw)
        da, db = a.digest(), b.digest()
        assert np.array_equal(da, db), "%s: digests differ at %s" % (w, np.argwhere(da != db)[:4])
        for p in range(n):
            (ta, ia, ra), (tb, ib, rb) = a.trajectories(p), b.trajectories(p)
            assert list(ta.keys()) == list(tb.keys()) and ia == ib and ra['cut_index_pos'] == rb['cut_index_pos'], w
            for k in ta:
                assert np.array_equal(ta[k][0], tb[k][0]), "%s planner %d / %s" % (w, p, k)
        if t['tick'] < K:
            assert np.all(da[:, 0] == 0), "%s: error words %s" % (w, da[:, 0])
            pr.check_trajectories(ta, ia, ra, t, w)
    a.close(); b.close()


# ---- lockstep differential: a race on the map -------------------------------------------------------------------------------------------
class MapScenario(gd.Scenario):
    """``test_gpu_sim_differential.Scenario`` with a friction map: every planner on ``grid`` with its own grip factor; the host side's
    planners build the dict from their own paths (``friction_replay.GridPlanner``)."""

    def __init__(self, lat, tab, units, grid, scales):
        gd.Scenario.__init__(self, lat, tab, units)
        self.grid, self.scales = grid, [float(s) for s in scales]
        assert len(self.scales) == self.n

    def fleet(self, hip):
        fleet = gd.Scenario.fleet(self, hip)
        fleet.friction(self.grid, scale=self.scales)
        return fleet

    def host(self, oracle):
        loop = gd.Scenario.host(self, oracle)
        loop.pl = [fr.GridPlanner(pl, self.grid, self.scales[p]) for pl, p in zip(loop.pl, self.hmap)]
        return loop


def test_lockstep_race_on_the_map_with_per_planner_grip(hip, monteblanco, oracle_backend, race, grid):
    """A race of 9 cars on the map, grip factors 1.0 down to 0.6 (every car its own), 200 ticks: discrete results exact, pose / speed /
    heading within 1e-12, paths and trajectories under the differential's rules; then one sim_run(200), bitwise the lockstep run."""
    n = 9
    entries, poses = sl.big_race(race, n)
    sc = MapScenario(monteblanco, race, [gd.race_unit("maprace", entries, poses)], grid, np.linspace(1.0, 0.6, n))
    assert sc.hmap == list(range(n))                   # every car is compared in full
    worst, stats = gd.both(sc, hip, oracle_backend, 200, "race on the map")
    assert stats['errors'] == 0 and stats['compared_in_full'] == 200 * n and {"follow", "straight"} <= stats['keys'], stats


# ---- tape ---------------------------------------------------------------------------------------------------------------------------
def test_a_tape_with_the_map_equals_the_per_call_run(hip, monteblanco, grid):
    T, n = 240, 3
    ticks = pr.load_ticks("gridmap")
    a, b = new_fleet(hip, n), new_fleet(hip, n)
    st = ticks[0]['start']
    for f in (a, b):
        f.friction(grid)
        f.set_start_range(0, n, st['pos'], st['heading'], st['vel'], st['max_heading_offset'])
    for t in ticks[:T]:
        va = t['vel_args']
        g = dict(prev_action=t['action_id_sel'], t_now=t['t'], vehicles=pr.vehicles_of_tick(t), zone_gids=pr.zone_gids_of_tick(monteblanco, t),
                 pos_est=t['pos_est'], vel_est=va['vel_est'], vel_max=va['vel_max'], gg_scale=va['gg_scale'], local_gg=TUPLE,
                 safety_d=va['safety_d'], incl_emerg_traj=va['incl_emerg_traj'])
        pi, vi, keep = a.pack_groups([(n, g)], ax_max_machines=va['ax_max_machines'])
        a.calc_paths_packed(pi)
        a.calc_vel_profile_packed(vi)
        b.tape_append_packed(pi, vi)
    assert b.tape_run(0, 100) > 0.0 and b.tape_run(100, T - 100) > 0.0          # (ticks 100 .. 199 carry the emergency profile: both tails)
    assert np.array_equal(a.digest(), b.digest())
    for p in range(n):
        (ta, ia, ra), (tb, ib, rb) = a.trajectories(p), b.trajectories(p)
        assert list(ta.keys()) == list(tb.keys()) and ia == ib and ra['cut_index_pos'] == rb['cut_index_pos']
        for k in ta:
            assert np.array_equal(ta[k][0], tb[k][0]), (p, k)
        pa, pb = a.paths(p), b.paths(p)
        assert pa['keys'] == pb['keys'] and all(np.array_equal(pa['path_param'][k], pb['path_param'][k]) for k in pa['keys'])
        pr.check_trajectories(tb, ib, rb, ticks[T - 1], "tape planner %d" % p)
    a.close(); b.close()


# ---- the emergency profile on a backup plan ------------------------------------------------------------------------------------------------
def test_emergency_profile_on_a_backup_tick_of_a_map_planner(hip, monteblanco, grid):
    """The text the row form gives (tests/test_gpu_fleet.py): planner 0 asks for the emergency profile on a tick whose first trajectory is
    the backup plan; its neighbour, which does not, is served."""
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    ticks = pr.load_ticks("gridmapdrop")
    n = 2
    fleet = new_fleet(hip, n)
    fleet.friction(grid)
    st = ticks[0]['start']
    fleet.set_start_range(0, n, st['pos'], st['heading'], st['vel'], st['max_heading_offset'])

    def call(t, emerg):
        va = t['vel_args']
        fleet.calc_paths([t['action_id_sel']] * n, [t['t']] * n, [pr.vehicles_of_tick(t)] * n, [pr.zone_gids_of_tick(monteblanco, t)] * n)
        fleet.calc_vel_profile([t['pos_est']] * n, va['vel_est'], vel_max=va['vel_max'], gg_scale=va['gg_scale'], local_gg=TUPLE,
                               ax_max_machines=va['ax_max_machines'], safety_d=va['safety_d'], incl_emerg_traj=emerg)
    for t in ticks[:300]:                                  # 20 ticks into the loss of grip: the backup branch is active
        if t['tick'] == 280:
            fleet.friction_scale(0.3)
        call(t, [bool(t['vel_args']['incl_emerg_traj'])] * n)
    with pytest.raises(BackendError, match="planner 0: emergency profile.*Length of loc_gg and kappa must be equal"):
        call(ticks[300], [True, False])
    traj, ids, ref = fleet.trajectories(1)
    pr.check_trajectories(traj, ids, ref, ticks[300], "the neighbour of the failing planner")
    fleet.close()
