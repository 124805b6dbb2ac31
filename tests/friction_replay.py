"""
TEST INFRASTRUCTURE (no test functions): helpers shared by tests/test_friction_host.py and tests/test_gpu_friction.py for the recordings
of tools/gen_golden_friction.py ('gridmap', 'gridmapdrop': the unmodified reference driven with ``FrictionGrid.local_gg`` of
tests/golden/friction_grid.npz).
"""
import os

import numpy as np

import planner_replay as pr
from graphbasedlocaltrajectoryplanner_amd.friction import FrictionGrid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEFT_FIRST = ("left", "right", "straight", "follow")
DEFAULT_PREF = ("right", "left", "straight", "follow")
# recording -> (opponents (s0, vel_scale, length), preference)   [tools/gen_golden_friction.py SCENARIOS]
SPECS = {"gridmap": ([(150.0, 0.45, 5.0)], LEFT_FIRST), "gridmapdrop": ([], DEFAULT_PREF)}
VEL_KEYS = ("vel_max", "gg_scale", "safety_d", "ax_max_machines", "incl_emerg_traj")


def load_grid():
    return FrictionGrid.load(os.path.join(ROOT, "tests", "golden", "friction_grid.npz"))


def vel_of(t):
    """calc_vel_profile keywords of a recorded tick without local_gg (the map's business)."""
    return {k: t['vel_args'][k] for k in VEL_KEYS}


def same_vel(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in VEL_KEYS)


def segments(ticks, n_ticks):
    """Tick ranges over which the velocity arguments AND the grid's scale stay the same."""
    cuts = [0] + [k for k in range(1, n_ticks)
                  if not same_vel(vel_of(ticks[k - 1]), vel_of(ticks[k])) or ticks[k - 1]['grid_scale'] != ticks[k]['grid_scale']] + [n_ticks]
    return list(zip(cuts[:-1], cuts[1:]))


def planner_entry(lat, name, ticks):
    """The recording's entry of ``Fleet.sim_setup`` / ``HostSimLoop``."""
    opp, pref = SPECS[name]
    st = ticks[0]['start']
    return dict(opponents=opp, static=[], pref=pref, pos_est=st['pos'], vel_est=0.0, zone_gids=pr.zone_gids_of_tick(lat, ticks[0]))


class GridPlanner(object):
    """A planner (n_scen = 1, interface of planner.Planner) whose ``calc_vel_profile`` builds ``local_gg`` as the dict of the grid's rows on
    ITS OWN paths of the tick -- what a caller of the reference does with a friction map (OTH.py:633-666). ``scale``: the grid's factor,
    changed between ticks by assignment."""

    def __init__(self, planner, grid, scale=1.0):
        self.pl, self.grid, self.scale = planner, grid, scale
        self.first_rows = None

    def __getattr__(self, name):
        return getattr(self.pl, name)

    def calc_vel_profile(self, pos_est, vel_est, **kw):
        kw.pop("local_gg", None)
        paths = self.pl.paths(0)
        lgg = self.grid.local_gg(paths['path_param'], self.scale)
        self.first_rows = lgg[paths['keys'][0]][0]
        return self.pl.calc_vel_profile(pos_est, vel_est, local_gg=[lgg], **kw)


def replay(planner, lat, ticks, grid, n_ticks=None):
    """The rules of ``planner_replay.replay`` for one planner (n_scen = 1) with the friction rows taken from ``grid`` instead of the
    analytic ``friction_map``: the same calls and the same checks on every tick -- start node, keys, node lists, node indices, rows and
    reduced flags exactly, the full paths and coefficients where the recording holds them, trajectories through
    ``check_trajectories`` -- plus the rows of the first key against the rows the reference was handed (``local_gg_first``)."""
    from helpers import assert_close_rel, assert_xy_close, assert_coeff_close, REL_TOL, KAPPA_FLOOR
    st = ticks[0]['start']
    assert planner.set_start(0, st['pos'], st['heading'], st['vel'], st['max_heading_offset']) == (st['in_track'], st['cor_heading'])
    p0 = planner.paths(0)
    assert p0['start_node'] == st['start_node']
    assert_xy_close(p0['path_param']['straight'][:, 0:2], st['path_param'][:, 0:2], what="start spline xy")
    assert_close_rel(p0['path_param']['straight'][:, 4], st['path_param'][:, 4], what="start spline el")
    if p0['coeff']['straight'].size:
        assert_coeff_close(p0['coeff']['straight'], st['coeff'], what="start spline coeff")
    seen = {'full': 0, 'keys': set(), 'dropped': 0, 'emergency': 0, 'ggmap': 0}
    for t in ticks[:n_ticks]:
        what = "tick %d" % t['tick']
        planner.calc_paths([t['action_id_sel']], [t['t']], [pr.vehicles_of_tick(t)], [pr.zone_gids_of_tick(lat, t)])
        got, exp = planner.paths(0), t['paths']
        assert got['start_node'] == exp['start_node'], "%s: start node %s vs %s" % (what, got['start_node'], exp['start_node'])
        assert got['keys'] == exp['keys'], "%s: keys %s vs %s" % (what, got['keys'], exp['keys'])
        assert got['const_rows'] == exp['const_rows'], "%s: const rows %d vs %d" % (what, got['const_rows'], exp['const_rows'])
        assert got['closest_obj_index'] == exp['closest_obj_index'], "%s: closest object" % what
        for k in exp['keys']:
            assert got['nodes'][k] == exp['nodes'][k], "%s/%s: node list" % (what, k)
            assert got['node_idx'][k] == exp['node_idx'][k], "%s/%s: node_idx" % (what, k)
            assert got['path_param'][k].shape[0] == exp['n_rows'][k], "%s/%s: rows" % (what, k)
            if k in exp['red_len']:
                assert got['red_len'][k] == exp['red_len'][k], "%s/%s: reduced flag" % (what, k)
        full = t['full']
        if full is not None:
            for k in exp['keys']:
                pp, epp = got['path_param'][k], full['path_param'][k]
                assert_xy_close(pp[:, 0:2], epp[:, 0:2], what="%s/%s xy" % (what, k))
                d = np.abs(np.mod(pp[:, 2] - epp[:, 2] + np.pi, 2 * np.pi) - np.pi)
                assert float(d.max()) <= REL_TOL * np.pi, "%s/%s psi" % (what, k)
                assert_close_rel(pp[:, 3], epp[:, 3], what="%s/%s kappa" % (what, k), floor=KAPPA_FLOOR)
                assert_close_rel(pp[:, 4], epp[:, 4], what="%s/%s el" % (what, k))
                assert_coeff_close(got['coeff'][k], full['coeff'][k], what="%s/%s coeff" % (what, k))
            seen['full'] += 1
        va = t['vel_args']
        lgg = grid.local_gg(got['path_param'], t['grid_scale'])
        assert_close_rel(lgg[got['keys'][0]][0], va['local_gg_first'], what="%s: friction rows of '%s'" % (what, got['keys'][0]))
        seen['ggmap'] += 1
        planner.calc_vel_profile([t['pos_est']], va['vel_est'], vel_max=va['vel_max'], gg_scale=va['gg_scale'], local_gg=[lgg],
                                 ax_max_machines=va['ax_max_machines'], safety_d=va['safety_d'], incl_emerg_traj=va['incl_emerg_traj'])
        traj, ids, ref = planner.trajectories(0)
        pr.check_trajectories(traj, ids, ref, t, what)
        ev = t['vel']
        seen['keys'].update(ev['keys'])
        seen['dropped'] += len([k for k in exp['keys'] if k not in ev['keys']])
        seen['emergency'] += int('emergency' in ev['keys'])
    return seen
