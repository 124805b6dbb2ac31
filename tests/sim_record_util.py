"""
TEST INFRASTRUCTURE (no test functions) of the fleet simulation's flight recorder (ltpl_fleet_sim_record, csrc/fleet_sim.hpp):

  ``PathsTap`` / ``host_record``   the host loop of tests/sim_loop.py made to yield records in the dict form of ``Fleet.sim_record_read``:
                                   a proxy around the planner object takes ``paths(0)`` at the start of ``calc_vel_profile``, i.e. at the
                                   recorder's capture P, between the tick's two calls
  ``check_paths`` ...              a record against a tick of a recording of the reference
"""
import numpy as np

import planner_replay as pr
from helpers import assert_xy_close


class PathsTap(object):
    """A planner object that remembers ``paths(0)`` as they stand when ``calc_vel_profile`` begins."""

    def __init__(self, planner):
        self._pl = planner
        self.snap = None

    def __getattr__(self, name):
        return getattr(self._pl, name)

    def calc_vel_profile(self, *args, **kwargs):
        self.snap = self._pl.paths(0)
        return self._pl.calc_vel_profile(*args, **kwargs)


def host_record(rec, tap, tick, planner, n_export):
    """Record of ``HostSimLoop.tick()`` (``rec``, planner object ``tap``) in the dict form of ``Fleet.sim_record_read``."""
    out = {"tick": tick, "planner": planner, "error": 1 if rec["failed"] else 0, "sel": rec["sel"], "t_now": rec["now"],
           "pos_est": list(rec["pos"]), "vel_est": rec["vel"], "heading": rec["theta"], "vehicles": [],
           "paths": {"keys": [], "nodes": {}, "n_rows": {}, "red_len": {}, "start_node": [-1, -1], "const_rows": -1,
                     "closest_obj_index": None, "const_path_seg": None},
           "traj": ({}, {}, {"cut_index_pos": 0, "cut_layer": 0, "vel_plan": 0.0, "acc_plan": 0.0, "vel_course": np.zeros(0)})}
    if rec["failed"]:
        return out
    p = tap.snap
    const = None
    if p["const_rows"] >= 0 and p["keys"]:
        const = p["path_param"][p["keys"][0]][:max(p["const_rows"], 0), 0:2].copy()
    out["vehicles"] = list(rec["veh"])
    out["paths"] = {"keys": list(p["keys"]), "nodes": dict(p["nodes"]), "n_rows": {k: p["path_param"][k].shape[0] for k in p["keys"]},
                    "red_len": dict(p["red_len"]), "start_node": list(p["start_node"]), "const_rows": p["const_rows"],
                    "closest_obj_index": p["closest_obj_index"], "const_path_seg": const}
    traj, ids, ref = rec["traj"]
    out["traj"] = ({k: [v[0][:n_export]] for k, v in traj.items()}, dict(ids), dict(ref, vel_course=np.zeros(0)))
    return out


def check_paths(rec, t, what):
    """What capture P holds against ``t['paths']`` of the recording: exact."""
    got, exp = rec["paths"], t["paths"]
    assert list(got["start_node"]) == exp["start_node"], "%s: start node %s vs %s" % (what, got["start_node"], exp["start_node"])
    assert got["keys"] == exp["keys"], "%s: keys %s vs %s" % (what, got["keys"], exp["keys"])
    assert got["const_rows"] == exp["const_rows"], "%s: const rows %d vs %d" % (what, got["const_rows"], exp["const_rows"])
    assert got["closest_obj_index"] == exp["closest_obj_index"], "%s: closest object" % what
    for k in exp["keys"]:
        assert got["nodes"][k] == exp["nodes"][k], "%s/%s: node list" % (what, k)
        assert got["n_rows"][k] == exp["n_rows"][k], "%s/%s: rows" % (what, k)
        if k in exp["red_len"]:
            assert got["red_len"][k] == exp["red_len"][k], "%s/%s: reduced flag" % (what, k)
    full = t["full"]
    if full is not None and exp["const_rows"] >= 0 and exp["keys"]:
        seg = full["path_param"][exp["keys"][0]][:exp["const_rows"], 0:2]
        assert got["const_path_seg"].shape == seg.shape, "%s: constant segment rows" % what
        if seg.shape[0]:
            assert_xy_close(got["const_path_seg"], seg, what="%s const_path_seg" % what)
        return 1
    return 0


def check_record_trajectories(rec, t, n_export, what):
    """``tick_replay.check_trajectories`` restated for a record: the same quantities under the same bounds, where the record holds them. It
    has no vel_course, and its rows end at ``n_export``: a digest entry that reads the last row (s_end, vx[-1], sum of vx) is compared
    where the trajectory was not trimmed."""
    traj, ids, ref = rec["traj"]
    er, ev, full = t["ref_idx"], t["vel"], t["full"]
    assert ref["cut_index_pos"] == er["cut_index_pos"] and ref["cut_layer"] == er["cut_layer"], "%s: cut" % what
    assert abs(ref["vel_plan"] - er["vel_plan"]) <= 1e-5 * max(abs(er["vel_plan"]), 1.0), "%s: vel_plan" % what
    assert abs(ref["acc_plan"] - er["acc_plan"]) <= 1e-5 * max(abs(er["acc_plan"]), 5.0), "%s: acc_plan" % what
    assert list(traj.keys()) == ev["keys"], "%s: trajectory keys %s vs %s" % (what, list(traj.keys()), ev["keys"])
    assert ids == ev["traj_id"], "%s: trajectory ids" % what
    untrimmed = 0
    for k in ev["keys"]:
        dg, tr = ev["digest"][k], traj[k][0]
        assert tr.shape == (min(dg[0], n_export), 7), "%s/%s: trajectory rows %s vs %d" % (what, k, tr.shape, dg[0])
        vs = max(abs(dg[4]) / max(dg[0], 1), 1.0)
        assert abs(tr[0, 5] - dg[2]) <= 1e-5 * max(vs, abs(dg[2])), "%s/%s: vx[0]" % (what, k)
        if dg[0] <= n_export:
            untrimmed += 1
            assert abs(tr[-1, 0] - dg[1]) <= 1e-5 * max(abs(dg[1]), 1.0), "%s/%s: s_end" % (what, k)
            assert abs(tr[-1, 5] - dg[3]) <= 1e-5 * max(vs, abs(dg[3])), "%s/%s: vx[-1]" % (what, k)
            assert abs(float(np.sum(tr[:, 5])) - dg[4]) <= 1e-5 * max(abs(dg[4]), 1.0), "%s/%s: sum vx" % (what, k)
        if full is not None:
            pr.check_traj(tr, full["traj"][k][:n_export], "%s/%s" % (what, k))
    return untrimmed


def check_vehicles(rec, t, what, n_own=None):
    """``vehicles`` against ``vehicles_of_tick(t)``: count exact, positions to the 1e-12 m tests/test_gpu_fleet_sim.py applies to the first
    vehicle (opponent poses depend on the clock and the race line alone)."""
    exp = pr.vehicles_of_tick(t)
    got = rec["vehicles"]
    assert len(got) == len(exp), "%s: vehicles %d vs %d" % (what, len(got), len(exp))
    for k, ((r, v, pos), (er, evel, epos)) in enumerate(zip(got, exp)):
        if n_own is not None and k >= n_own:
            break
        assert pos.shape == (2, 2)
        assert np.max(np.abs(pos[0] - epos[0])) <= 1e-12, "%s: vehicle %d at %s vs %s" % (what, k, pos[0], epos[0])
        assert abs(r - er) <= 1e-12, "%s: radius of vehicle %d" % (what, k)


def records_equal(a, b, skip=("tick",)):
    """Two records of ``sim_record_read`` bit for bit (``skip``: head keys left out)."""
    for k in ("tick", "planner", "error", "sel", "t_now", "pos_est", "vel_est", "heading"):
        if k not in skip and not np.array_equal(np.asarray(a[k], dtype=object), np.asarray(b[k], dtype=object)):
            return "head %s: %s vs %s" % (k, a[k], b[k])
    if len(a["vehicles"]) != len(b["vehicles"]):
        return "vehicle count"
    for (r, v, pos), (r2, v2, pos2) in zip(a["vehicles"], b["vehicles"]):
        if r != r2 or v != v2 or not np.array_equal(pos, pos2):
            return "vehicles"
    pa, pb = a["paths"], b["paths"]
    for k in ("keys", "nodes", "n_rows", "red_len", "const_rows", "closest_obj_index"):
        if pa[k] != pb[k]:
            return "paths %s" % k
    if list(pa["start_node"]) != list(pb["start_node"]):
        return "start node"
    if (pa["const_path_seg"] is None) != (pb["const_path_seg"] is None):
        return "constant segment"
    if pa["const_path_seg"] is not None and not np.array_equal(pa["const_path_seg"], pb["const_path_seg"]):
        return "constant segment"
    (ta, ia, ra), (tb, ib, rb) = a["traj"], b["traj"]
    if list(ta.keys()) != list(tb.keys()) or ia != ib:
        return "trajectory keys / ids"
    for k in ta:
        if not np.array_equal(ta[k][0], tb[k][0]):
            return "trajectory %s" % k
    for k in ("cut_index_pos", "cut_layer", "vel_plan", "acc_plan"):
        if ra[k] != rb[k]:
            return "ref %s" % k
    return None
