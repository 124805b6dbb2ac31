"""Plain reference of the shortest-path sweep (csrc/paths_team.hpp `team_layer`, `team_serial_node` / `team_relax_layer`, `team_resweep`,
`team_goal`): a layered dynamic programme in NumPy that states the contract the device result is compared with bit for bit --

    frontier   d[n] = min over the usable in-edges (src -> n) of  dprev[src] + cost  (ONE fp64 addition; a discounted edge costs
               cost * factor, rounded, before that addition)
    parent     among the edges at that exact minimum: the smaller dprev[src], then the smaller source node
    goal       the node of the goal layer with the lexicographic minimum of (d + goal cost, d, node)
    n_ties     the nodes of the returned path with two or more in-edges at the exact minimum, plus the goal choice
    horizon    follow / straight step the goal layer back to the last layer they reach; the slots behind them inherit that layer

and the four filters: `planning_range` uses every edge, `default` the unblocked ones, left / right are `default` without the nodes
n >= cn / n < cn on the closest object's layer; zone nodes are missing in all four. WHAT is blocked, which object is the closest one and
the end layer are inputs (the oracle's, pinned by tests/test_gpu_mask_boundary.py and the recordings): this file is about the search only.

Besides the result it keeps a census per path node -- how many edges tied, which level of the rule decided, where the tied edges lie in
SWEEP ORDER (the order of a transition's edges in the kernel's register image and tail: by in-edge rank, then by destination, restated
here from the lattice) -- from which tests/sweep_cases.py computes what a scenario set exercises.
"""
import collections

import numpy as np

from graphbasedlocaltrajectoryplanner_amd import _capi

F_PR, F_DEF, F_LEFT, F_RIGHT = 0, 1, 2, 3
FILTER_NAMES = ("planning_range", "default", "left", "right")
LEVEL_UNIQUE, LEVEL_PRED_DIST, LEVEL_SOURCE = 0, 1, 2

# one tie on a path: the node (j layers behind the start layer), the edges at the minimum and the one the rule elects
Census = collections.namedtuple("Census", "j layer node level n_winners in_degree edges positions elected n_edges")
Path = collections.namedtuple("Path", "action_id valid reduced goal_layer n_nodes n_ties nodes filt goal_level census")


def sweep_positions(lat):
    """Position of every edge inside its transition in sweep order: the transition's edges sorted by (in-edge rank, destination node), the
    rank being the edge's index among the in-edges of its destination (sources ascending)."""
    in_ptr, off = lat.in_ptr.astype(np.int64), lat.layer_off.astype(np.int64)
    deg = np.diff(in_ptr)
    dst = np.repeat(np.arange(lat.num_nodes), deg)
    rank = np.arange(lat.num_edges) - in_ptr[dst]
    pos = np.empty(lat.num_edges, np.int64)
    for l in range(lat.num_layers):
        e0, e1 = in_ptr[off[l]], in_ptr[off[l + 1]]
        order = np.lexsort((dst[e0:e1], rank[e0:e1]))                 # (last key first)
        pos[e0 + order] = np.arange(e1 - e0)
    return pos


def discounted_costs(lat, scen, w_last, in_range):
    """The tick's copy of the edge costs: the i-th edge of the previous solution times w_last[i], where both its nodes are in the range."""
    cost = lat.edge_cost.copy()
    last = [n for n in (scen.get("last_nodes") or [])][:_capi.MAX_LAST_NODES]
    hit = []
    for i in range(min(len(last) - 1, len(w_last))):
        e = lat.find_edge(int(last[i][0]), int(last[i][1]), int(last[i + 1][0]), int(last[i + 1][1]))
        if e < 0:
            continue
        dst = int(lat.layer_off[last[i + 1][0]]) + int(last[i + 1][1])
        src = int(lat.layer_off[last[i][0]]) + int(last[i][1])
        if in_range[src] and in_range[dst]:
            cost[e] = cost[e] * float(w_last[i])
            hit.append(e)
    return cost, hit


class Sweep(object):
    """The frontiers of one filter over the whole planning range of one scenario."""

    def __init__(self, lat, start_layer, start_node, n_trans, active, cost, blocked):
        L, off, in_ptr = lat.num_layers, lat.layer_off.astype(np.int64), lat.in_ptr.astype(np.int64)
        self.lat, self.start_layer = lat, start_layer
        self.dist, self.parent, self.cand, self.e0 = [], [], [None], [0]
        k0 = int(lat.nodes_in_layer[start_layer])
        d = np.full(k0, np.inf)
        if 0 <= start_node < k0 and active[off[start_layer] + start_node]:
            d[start_node] = 0.0
        self.dist.append(d)
        self.parent.append(np.full(k0, -1))
        for j in range(1, n_trans + 1):
            l, pl = (start_layer + j) % L, (start_layer + j - 1) % L
            v0, v1 = off[l], off[l + 1]
            e0, e1 = in_ptr[v0], in_ptr[v1]
            deg = np.diff(in_ptr[v0:v1 + 1])
            dst = np.repeat(np.arange(v1 - v0), deg)
            src = lat.edge_src[e0:e1].astype(np.int64)
            dprev = self.dist[-1]
            with np.errstate(invalid="ignore"):
                cand = dprev[src] + cost[e0:e1]                       # the one addition
            usable = active[off[pl] + src] & active[v0 + dst] & np.isfinite(dprev[src])
            if blocked is not None:
                usable &= blocked[e0:e1] == 0
            cand = np.where(usable, cand, np.inf)
            d = np.full(v1 - v0, np.inf)
            np.minimum.at(d, dst, cand)
            par = np.full(v1 - v0, -1)
            win = usable & (cand == d[dst]) & np.isfinite(cand)
            # among the winners: smaller dprev, then smaller source (edges of one destination are sorted by source)
            idx = np.nonzero(win)[0]
            idx = idx[np.lexsort((src[idx], dprev[src[idx]], dst[idx]))]
            first = np.ones(len(idx), bool)
            first[1:] = dst[idx[1:]] != dst[idx[:-1]]
            par[dst[idx[first]]] = src[idx[first]]
            self.dist.append(d)
            self.parent.append(par)
            self.cand.append((cand, win, dst, src))
            self.e0.append(int(e0))

    def reachable(self, j):
        return bool(np.isfinite(self.dist[j]).any())

    def goal(self, j, goal_cost):
        """(node, level 0 / 1 / 2 that decided, number of nodes at the least total) on layer j."""
        d = self.dist[j]
        fin = np.isfinite(d)
        total = np.where(fin, d + goal_cost, np.inf)
        best = total.min()
        at = np.nonzero(fin & (total == best))[0]
        dm = d[at].min()
        at_d = at[d[at] == dm]
        level = LEVEL_UNIQUE if len(at) == 1 else (LEVEL_PRED_DIST if len(at_d) == 1 else LEVEL_SOURCE)
        return int(at_d[0]), level, len(at)

    def census(self, j, n, pos):
        """The tie (or None) at node n of layer j."""
        cand, win, dst, src = self.cand[j]
        idx = np.nonzero(win & (dst == n))[0]
        if len(idx) < 2:
            return None
        dprev = self.dist[j - 1]
        dp = dprev[src[idx]]
        level = LEVEL_PRED_DIST if int((dp == dp.min()).sum()) == 1 else LEVEL_SOURCE
        elected = idx[dp == dp.min()][0]
        assert src[elected] == self.parent[j][n]
        e0 = self.e0[j]
        return Census(j, (self.start_layer + j) % self.lat.num_layers, int(n), level, len(idx), int((dst == n).sum()),
                      tuple(int(e0 + e) for e in idx), tuple(int(pos[e0 + e]) for e in idx), int(e0 + elected), len(cand))


def plan_scenario(lat, scen, w_last, blocked, closest, pos=None):
    """The three action slots of one scenario: a list of `Path` (None for an unused slot). ``blocked``: uint8 [E], the edges `default`
    lacks; ``closest``: (layer, node) of the closest object or None. Scenarios with a constant-segment result are not covered."""
    assert not scen.get("obj_in_const") and not scen.get("obj_besides") and scen.get("const_closest") is None
    L, off = lat.num_layers, lat.layer_off.astype(np.int64)
    pos = sweep_positions(lat) if pos is None else pos
    sl, sn = int(scen["start_node"][0]), int(scen["start_node"][1])
    end_layer = lat.horizon_end_layer(sl)
    n_trans = (end_layer - sl) % L
    layer_of = np.repeat(np.arange(L), lat.nodes_in_layer)
    ahead = (layer_of - sl) % L
    in_range = ahead <= n_trans
    for g in scen.get("zone_gids", ()):
        in_range[int(g)] = False
    cost, _ = discounted_costs(lat, scen, w_last, in_range)
    if scen.get("action_sets", True) and closest is not None:
        slots = [(F_PR, _capi.ACT_FOLLOW), (F_LEFT, _capi.ACT_LEFT), (F_RIGHT, _capi.ACT_RIGHT)]
    else:
        slots = [(F_DEF, _capi.ACT_STRAIGHT)]
    out, sweeps, mod = [], {}, n_trans                                # ``mod``: the goal layer, in layers behind the start layer
    for filt, name in slots:
        active = in_range.copy()
        if filt in (F_LEFT, F_RIGHT):
            cl, cn = closest
            n = np.arange(int(lat.nodes_in_layer[cl]))
            active[off[cl]:off[cl + 1]] &= (n < cn) if filt == F_LEFT else (n >= cn)
        sw = Sweep(lat, sl, sn, n_trans, active, cost, None if filt == F_PR else blocked)
        found = False
        while mod > 0:
            found = sw.reachable(mod)
            if found or name not in (_capi.ACT_FOLLOW, _capi.ACT_STRAIGHT):
                break
            mod -= 1
        reduced = mod != n_trans or (not lat.closed and end_layer == L - 1)
        if reduced and closest is not None and (closest[0] - sl) % L > mod:
            if name in (_capi.ACT_FOLLOW, _capi.ACT_STRAIGHT):
                name = _capi.ACT_STRAIGHT
            else:
                found = False
        goal_layer = (sl + mod) % L
        if not found:
            out.append(Path(name, 0, int(reduced), goal_layer, 0, 0, (), filt, None, ()))
            continue
        node, goal_level, n_goal = sw.goal(mod, lat.vgoal_cost[off[goal_layer]:off[goal_layer + 1]])
        nodes, cen = [node], []
        for j in range(mod, 0, -1):
            c = sw.census(j, nodes[-1], pos)
            if c is not None:
                cen.append(c)
            nodes.append(int(sw.parent[j][nodes[-1]]))
        nodes.reverse()
        assert nodes[0] == sn
        out.append(Path(name, 1, int(reduced), goal_layer, len(nodes), len(cen) + (n_goal > 1), tuple(nodes), filt, goal_level, tuple(cen)))
    return out + [None] * (_capi.MAX_ACTIONS - len(out))


INT_FIELDS = ("action_id", "valid", "reduced", "goal_layer", "n_nodes", "n_ties")


def differences(paths, res, s):
    """Names of the fields in which slot results ``paths`` (of `plan_scenario`) differ from scenario s of a PathsResult."""
    bad = []
    if int(res.n_actions[s]) != sum(p is not None for p in paths):
        bad.append("n_actions")
    for a, p in enumerate(paths):
        if p is None:
            continue
        for f in INT_FIELDS:
            if int(getattr(res, f)[s, a]) != getattr(p, f):
                bad.append("%s[%d]" % (f, a))
        if p.valid and res.nodes[s, a, :p.n_nodes].tolist() != list(p.nodes):
            bad.append("nodes[%d]" % a)
    return bad
