"""Lattices, cost families and scenario sets of the sweep tests (tests/test_sweep_cases_host.py on the CPU, tests/test_gpu_sweep.py on the GPU):
small ovals, one per LDS plan class, whose transitions are pruned to CHOSEN edge counts around every size at which the layer step of
csrc/paths_team.hpp changes its form, and whose edge costs are overwritten so that exact ties lie on the returned paths by the hundred.

  lattice  plan class          layers x nodes   edges of a full transition   register image of the one-wave kernel
  A        PlanFx<32,32,1>     32 x 24          576 (fully connected)        192 edges (3 chunks of 64)
  B        PlanFx<32,40,1>     40 x 24          576 (fully connected)        192, the first 64 tail edges prefetched
  C        PlanFx<48,32,1>     32 x 40          608 (lat_steps 8)            192
  R        PlanRt              20 x 64          4096 (fully connected)       256 (4 chunks)
  V        PlanRt              16 x 70 / 40 alternating, one layer of 1 node (serial and edge-parallel layer steps in turns)

The geometry is the generator's (the assembly runs on it unchanged); `prune` rebuilds the CSC, sample and coefficient arrays for a keep
mask. Transition l keeps COUNTS[l % len(COUNTS)] edges: 64, 128, 192, 256, 320, 512 each -1 / 0 / +1 and the full transition, at least
one in-edge per node, and on some transitions a source node without any out-edge (a start there has no valid path).

A SET is (lattice, cost family, scenario family); `case(name).sets` lists them (15; V has one more: `goal_pair`). Both references -- the oracle (Dijkstra) and the layered
DP of tests/sweep_ref.py -- are computed once per process, shared by the tests and left unchanged.
"""
import functools

import numpy as np

import assembly_cases as ac
import sweep_ref as sr
from graphbasedlocaltrajectoryplanner_amd import _capi
from graphbasedlocaltrajectoryplanner_amd.lattice import Lattice
from graphbasedlocaltrajectoryplanner_amd.synthetic_lattice import make_oval_lattice

W_LAST = [1.0, 0.5, 0.5]

LATTICE_ARGS = {
    "A": dict(num_layers=32, nodes_per_layer=24, layer_spacing=6.0, lat_resolution=0.3, lat_steps=24, stepsize=2.5, radius=25.0,
              horizon=60.0, v_straight=40.0),
    "B": dict(num_layers=40, nodes_per_layer=24, layer_spacing=6.0, lat_resolution=0.3, lat_steps=24, stepsize=2.5, radius=30.0,
              horizon=186.0, v_straight=40.0),
    "C": dict(num_layers=32, nodes_per_layer=40, layer_spacing=6.0, lat_resolution=0.2, lat_steps=8, stepsize=2.5, radius=25.0,
              horizon=60.0, v_straight=40.0),
    "R": dict(num_layers=20, nodes_per_layer=64, layer_spacing=6.0, lat_resolution=0.1, lat_steps=64, stepsize=2.5, radius=15.0,
              horizon=36.0, v_straight=40.0),
    "V": dict(num_layers=16, nodes_per_layer=tuple(1 if l == 13 else (70 if l % 2 == 0 else 40) for l in range(16)), layer_spacing=6.0,
              lat_resolution=0.1, lat_steps=35, stepsize=2.5, radius=12.0, horizon=48.0, v_straight=40.0),
}
PLAN_CLASS = {"A": "PlanFx<32,32,1>", "B": "PlanFx<32,40,1>", "C": "PlanFx<48,32,1>", "R": "PlanRt", "V": "PlanRt"}
IMAGE = {"A": 192, "B": 192, "C": 192, "R": 256, "V": 256}      # edges of a transition in the registers of the one-wave kernel
FORM_EDGES = (64, 128, 192, 256, 320, 512)
NO_OUT_EVERY, NO_OUT_NODE = 5, 1                                 # transitions out of layers l % 5 == 2: source node 1 keeps no out-edge


def full_counts(lat):
    off, in_ptr = lat.layer_off, lat.in_ptr
    return [int(in_ptr[off[l + 1]] - in_ptr[off[l]]) for l in range(lat.num_layers)]


def chosen_counts(full, n_nodes=1):
    """The edge counts a lattice cycles through whose full transition has ``full`` edges (every node keeps an in-edge: at least ``n_nodes``)."""
    return sorted({c + d for c in FORM_EDGES for d in (-1, 0, 1) if n_nodes <= c + d < full}) + [full]


def prune(lat, keep):
    """``lat`` with the edges ``keep`` (bool [E]) only: CSC pointers, sources, costs, lengths, coefficients and samples rebuilt."""
    keep = np.asarray(keep, bool)
    deg = np.diff(lat.in_ptr)
    dst = np.repeat(np.arange(lat.num_nodes), deg)
    in_ptr = np.zeros(lat.num_nodes + 1, np.int64)
    np.add.at(in_ptr, dst[keep] + 1, 1)
    n_samp = np.diff(lat.samp_ptr)
    samp_keep = np.repeat(keep, n_samp)
    d = lat.to_dict()
    d.update(in_ptr=np.cumsum(in_ptr), edge_src=lat.edge_src[keep], edge_cost=lat.edge_cost[keep], edge_len=lat.edge_len[keep],
             edge_coeff=lat.edge_coeff[keep], samp_ptr=np.concatenate(([0], np.cumsum(n_samp[keep]))), samples=lat.samples[samp_keep])
    return Lattice(**d)


def keep_mask(lat, counts_of_layer, rng):
    """A keep mask with counts_of_layer[l] edges into layer l (clipped to what the transition has): one in-edge per node first, then
    random others; where l - 1 is a NO_OUT layer and the transition is not kept whole, none from NO_OUT_NODE."""
    off, in_ptr, L = lat.layer_off, lat.in_ptr, lat.num_layers
    keep = np.zeros(lat.num_edges, bool)
    for l in range(L):
        e0, e1 = int(in_ptr[off[l]]), int(in_ptr[off[l + 1]])
        pool = np.ones(e1 - e0, bool)
        if ((l - 1) % L) % NO_OUT_EVERY == 2 and counts_of_layer[l] < e1 - e0:
            pool &= lat.edge_src[e0:e1] != NO_OUT_NODE
        want = max(min(int(counts_of_layer[l]), int(pool.sum())), int(off[l + 1] - off[l]))
        sel = np.zeros(e1 - e0, bool)
        for v in range(int(off[l]), int(off[l + 1])):
            c = np.nonzero(pool[in_ptr[v] - e0:in_ptr[v + 1] - e0])[0] + (in_ptr[v] - e0)
            sel[rng.choice(c)] = True
        rest = np.nonzero(pool & ~sel)[0]
        sel[rng.choice(rest, want - int(sel.sum()), replace=False)] = True
        keep[e0:e1] = sel
    return keep


@functools.lru_cache(maxsize=None)
def lattice(name):
    """The pruned lattice ``name`` (generator's costs) and the edge count of every transition."""
    full = make_oval_lattice(**LATTICE_ARGS[name])
    fc = full_counts(full)
    if name == "V":                                               # widths alternate: every transition gets a count of its own size class
        width = full.nodes_in_layer
        counts = [chosen_counts(fc[l], width[l])[(l // 2) % len(chosen_counts(fc[l], width[l]))] for l in range(full.num_layers)]
    else:
        cc = chosen_counts(fc[0], int(full.nodes_in_layer[0]))
        assert len(set(fc)) == 1 and len(cc) <= full.num_layers
        counts = [cc[l % len(cc)] for l in range(full.num_layers)]
    lat = prune(full, keep_mask(full, counts, np.random.default_rng(sum(map(ord, name)))))
    assert np.all(np.diff(lat.in_ptr) >= 1)
    assert ac.plan_class_of(lat) == PLAN_CLASS[name], (name, ac.plan_class_of(lat))
    return lat


# ---- cost families ---------------------------------------------------------------------------------------------------------------
def _magnitudes(lat, rng):
    """Costs over the whole exponent range, 1e-320 (subnormal) into layer 0 up to 1e300 into the last layer, mantissas all different: every
    addition in front of the seam is dominated by the new edge (the frontier's bit patterns span the range), behind the seam it is
    absorbed (frontiers equal to the bit)."""
    dl = lat.layer_of(lat.edge_dst_gid()).astype(np.float64)
    return rng.uniform(1.0, 10.0, lat.num_edges) * np.power(10.0, -320.0 + 620.0 * dl / (lat.num_layers - 1))


def _chunk_edges(lat):
    pos = sr.sweep_positions(lat)
    n_edges = np.repeat(np.asarray(full_counts(lat)), np.asarray(full_counts(lat)))          # (edges are stored transition by transition)
    ends = np.isin(pos % 64, (0, 63)) | (pos == n_edges - 1)
    return np.where(ends, 1.0, 3.0)


COST_FAMILIES = {
    # name: (edge costs, goal costs or None = the generator's |offset from the race line| x 10000: unique at the goal)
    "ones": (lambda lat, rng: np.ones(lat.num_edges), None),
    "int13": (lambda lat, rng: rng.integers(1, 4, lat.num_edges).astype(np.float64), None),
    "tenths": (lambda lat, rng: 0.1 * rng.integers(1, 10, lat.num_edges), None),
    "magnitudes": (_magnitudes, None),
    "goal_zero": (lambda lat, rng: rng.integers(1, 4, lat.num_edges).astype(np.float64), lambda lat, rng: np.zeros(lat.num_nodes)),
    # every edge into node n costs 1 + n % 3 and the goal cost takes that back (3 - it, plus 0 or 1): totals tie among nodes of different distance
    "goal_ties": (lambda lat, rng: 1.0 + ((lat.edge_dst_gid() - lat.layer_off[lat.layer_of(lat.edge_dst_gid())]) % 3),
                  lambda lat, rng: 2.0 - ((np.arange(lat.num_nodes) - lat.layer_off[lat.layer_of(np.arange(lat.num_nodes))]) % 3)
                  + (rng.uniform(size=lat.num_nodes) > 0.3)),
    # all totals equal on exactly two nodes of a layer, 64 apart where the layer is that wide (one lane of the goal search holds both)
    "goal_pair": (lambda lat, rng: np.ones(lat.num_edges),
                  lambda lat, rng: 5.0 * (((np.arange(lat.num_nodes) - lat.layer_off[lat.layer_of(np.arange(lat.num_nodes))]) % 64) != 2)),
    # cost 1 on the edges at the ends of the 64-edge chunks and of the transition (in sweep order), 3 elsewhere: the paths run over them
    "chunk_edges": (lambda lat, rng: _chunk_edges(lat), None),
    "zero_mixed": (lambda lat, rng: rng.integers(0, 4, lat.num_edges).astype(np.float64), lambda lat, rng: np.zeros(lat.num_nodes)),
    "zero": (lambda lat, rng: np.zeros(lat.num_edges), lambda lat, rng: np.zeros(lat.num_nodes)),
}
ZERO_FAMILIES = ("zero_mixed", "zero")                            # where the layered rule and a settle order by vertex id may part


@functools.lru_cache(maxsize=None)
def costed(name, family):
    lat = lattice(name)
    rng = np.random.default_rng(sum(map(ord, name + family)))
    cost, goal = COST_FAMILIES[family]
    d = lat.to_dict()
    d["edge_cost"] = cost(lat, rng)
    if goal is not None:
        d["vgoal_cost"] = goal(lat, rng)
    assert np.all(np.isfinite(d["edge_cost"]))
    return Lattice(**d)


# ---- scenario families -----------------------------------------------------------------------------------------------------------
def scenario(lat, sl, sn, vehicles=(), zone=(), last_nodes=None):
    return {"start_node": (int(sl), int(sn)), "action_sets": True, "vehicles": list(vehicles), "zone_gids": [int(g) for g in zone],
            "last_nodes": last_nodes, "obj_in_const": False, "obj_besides": False, "last_action": None, "const_closest": None, "psi_s": None}


def start_layers(lat, at_least):
    L = lat.num_layers
    return list(range(0, L, 2 if L // 2 >= at_least else 1))


def free_scenarios(lat):
    """Free track from every (second) layer -- ranges that cross the seam included -- from both edge nodes, the race-line node and node 1,
    which on some layers has no out-edge."""
    out = []
    for l in start_layers(lat, 16):
        k = int(lat.nodes_in_layer[l])
        for n in sorted({0, min(1, k - 1), int(lat.raceline_index[l]), k - 1}):
            out.append(scenario(lat, l, n))
    for l in range(2, lat.num_layers, NO_OUT_EVERY):
        if int(lat.nodes_in_layer[l]) > NO_OUT_NODE:
            out.append(scenario(lat, l, NO_OUT_NODE))
    return out


def wall_scenarios(lat):
    """A zone wall d = 1 .. layers ahead (the whole layer, or all of it but its two outermost nodes on one side): follow / straight fall
    back to the last layer they reach."""
    out, L = [], lat.num_layers
    n_trans = (lat.horizon_end_layer(0) - 0) % L
    k = 0
    while len(out) < 64:
        for l in start_layers(lat, 16):
            d = 2 + (k + l) % (n_trans - 1)
            wl = (l + d) % L
            kw = int(lat.nodes_in_layer[wl])
            gids = [int(lat.layer_off[wl]) + n for n in range(kw if (k + l // 2) % 3 else max(kw - 2, 1))]
            kn = int(lat.nodes_in_layer[l])
            out.append(scenario(lat, l, (0, int(lat.raceline_index[l]), kn - 1)[(l // 2 + k) % 3], zone=gids))
        k += 1
    return out


def obstacle_scenarios(lat):
    """One to three static obstacles on the track: at the first transition, in the middle of the range and near its end."""
    rng = np.random.default_rng(lat.num_nodes)
    L = lat.num_layers
    n_trans = (lat.horizon_end_layer(0) - 0) % L
    out, k = [], 0
    while len(out) < 64:
        for l in start_layers(lat, 16):
            veh = []
            for i in range(1 + (k + l // 2) % 3):
                ahead = (rng.uniform(0.3, 1.2), rng.uniform(1.5, n_trans - 1.5), rng.uniform(n_trans - 2.0, n_trans - 0.5))[(i + k + l) % 3]
                l0 = (l + int(ahead)) % L
                f = ahead - int(ahead)
                half = (int(lat.nodes_in_layer[l0]) - 1) * lat.lat_resolution / 2.0
                pos = lat.refline[l0] * (1.0 - f) + lat.refline[(l0 + 1) % L] * f + lat.normvec[l0] * rng.uniform(-half, half)
                veh.append((rng.uniform(0.1, 0.8), np.vstack((pos[None, :], pos[None, :]))))
            kn = int(lat.nodes_in_layer[l])
            out.append(scenario(lat, l, (int(lat.raceline_index[l]), 0, kn - 1)[(l // 2 + k) % 3], vehicles=veh))
        k += 1
    # a small obstacle beside the outermost node of the start layer, start there: every edge it blocks leaves one of the last source nodes, so
    # in a transition of many edges they all have a high in-edge rank -- beyond the register image; `default` has no path, `planning_range` has
    counts = full_counts(lat)
    for l in range(L):
        kn = int(lat.nodes_in_layer[l])
        if counts[(l + 1) % L] > 256 and kn > 1:
            p = lat.node_pos[int(lat.layer_off[l]) + kn - 1] + lat.normvec[l] * 1.7
            out.append(scenario(lat, l, kn - 1, vehicles=[(0.1, np.vstack((p[None, :], p[None, :])))]))
            # ... and the same with the obstacle's last predicted position three layers ahead: the closest object's layer is then that one,
            # left / right share `default`'s sweep up to it and `planning_range` rides on it -- over a transition whose blocked edges all lie
            # beyond the register image, which the riding test cannot see: it has to part there
            l3 = (l + 3) % L
            q = lat.node_pos[int(lat.layer_off[l3 + 1]) - 1] + lat.normvec[l3] * 1.7
            out.append(scenario(lat, l, kn - 1, vehicles=[(0.1, np.vstack((p[None, :], q[None, :])))]))
    return out


def discount_scenarios(lat, pos, image):
    """Previous solutions whose discount (W_LAST = 1, 0.5, 0.5) CREATES a tie at P2, the second node of the free path: an edge n1 -> P2 that
    misses the minimum d[P2] without the discount and meets it exactly with it -- 1 + 2 x 0.5 beside 1 + 1 with the node list aligned at
    the start node, (start, n1, P2); 2 x 0.5 + 2 x 0.5 (elected or not by the source node) or 1 x 0.5 + 3 x 0.5 (elected by its smaller
    predecessor distance wherever it lies) with the list shifted by one layer, (before, start, n1, P2), where the edge start -> n1 is
    discounted as well -- and one that BREAKS a tie (an edge at the minimum halved). Per kind n1 is taken with the discounted edge in the
    register image and, where the transition has one, in the tail; as smallest and as largest such source."""
    out, L = [], lat.num_layers
    for l in range(L):
        k = int(lat.nodes_in_layer[l])
        mid = int(lat.raceline_index[l])
        for sn in sorted({0, max(mid - 1, 0), mid, min(mid + 1, k - 1), k - 1}):
            free = sr.plan_scenario(lat, scenario(lat, l, sn), W_LAST, None, None, pos)[0]
            if not free.valid or free.n_nodes < 4:
                continue
            l1, l2 = (l + 1) % L, (l + 2) % L
            p2 = int(free.nodes[2])
            v = int(lat.layer_off[l2]) + p2
            into = []                                             # (n1, edge, cost start -> n1, cost n1 -> P2)
            for e in range(int(lat.in_ptr[v]), int(lat.in_ptr[v + 1])):
                e1 = lat.find_edge(l, sn, l1, int(lat.edge_src[e]))
                if e1 >= 0:
                    into.append((int(lat.edge_src[e]), e, float(lat.edge_cost[e1]), float(lat.edge_cost[e])))
            dmin = min(c1 + c2 for _, _, c1, c2 in into)
            picks = {}
            for n1, e, c1, c2 in into:
                where = "reg" if pos[e] < image else "tail"
                kinds = []
                if c1 + c2 > dmin and c1 * W_LAST[0] + c2 * W_LAST[1] == dmin:
                    kinds.append("aligned")
                if c1 + c2 > dmin and c1 * W_LAST[1] + c2 * W_LAST[2] == dmin:
                    kinds.append("shifted, predecessor %s" % ("closer" if c1 * W_LAST[1] < 1.0 else "level"))
                if c1 + c2 == dmin:
                    kinds.append("breaks")
                for kind in kinds:
                    picks.setdefault((kind, where, "lo"), n1)
                    picks[(kind, where, "hi")] = n1
            for (kind, where, _), n1 in sorted(picks.items()):
                if kind.startswith("shifted"):
                    last = [[(l - 1) % L, 0], [l, sn], [l1, n1], [l2, p2]]
                else:
                    last = [[l, sn], [l1, n1], [l2, p2]]
                out.append(scenario(lat, l, sn, last_nodes=last))
    # (a random subset: the set stays a few hundred scenarios at the most)
    take = np.random.default_rng(len(out)).choice(len(out), min(len(out), 320), replace=False)
    return [out[i] for i in sorted(take)]


SETS = (("ones", "free"), ("int13", "free"), ("tenths", "free"), ("magnitudes", "free"), ("goal_zero", "free"), ("goal_ties", "free"),
        ("zero_mixed", "free"), ("zero", "free"), ("chunk_edges", "free"), ("int13", "discount"), ("ones", "wall"), ("tenths", "wall"), ("ones", "obstacles"),
        ("int13", "obstacles"), ("zero_mixed", "obstacles"))


def batch_of(scen):
    return _capi.PathsBatch(scen, w_last_edges=W_LAST)


class ScenarioSet(object):
    """One (cost family, scenario family) on a lattice with both references: ``ref`` the oracle's PathsResult, ``dp`` the slots of
    sweep_ref.plan_scenario per scenario, ``agree`` [n] whether the two give the same paths."""

    def __init__(self, name, family, kind, lat, scen, oracle, pos):
        self.name, self.family, self.kind, self.lat, self.scen = name, family, kind, lat, scen
        assert len(scen) >= 64, (name, family, kind, len(scen))
        self.ref, blocked = oracle.plan_paths_mask(batch_of(scen))
        self.blocked = blocked if kind == "obstacles" else None
        self.dp, self.diff = [], []
        for s, sc in enumerate(scen):
            cl = tuple(int(x) for x in self.ref.closest_obj_node[s])
            self.dp.append(sr.plan_scenario(lat, sc, W_LAST, blocked[s], None if cl[0] < 0 else cl, pos))
            assert int(self.ref.end_layer[s]) == lat.horizon_end_layer(sc["start_node"][0])
            self.diff.append(sr.differences(self.dp[-1], self.ref, s))
        self.agree = np.array([not d for d in self.diff])
        L = lat.num_layers
        self.crosses_seam = np.array([sc["start_node"][0] + (int(self.ref.end_layer[s]) - sc["start_node"][0]) % L >= L
                                      for s, sc in enumerate(scen)])

    @property
    def label(self):
        return "%s/%s/%s" % (self.name, self.family, self.kind)


class Case(object):
    def __init__(self, name):
        from oracle.oracle_lib import OracleBackend
        self.name, self.base = name, lattice(name)
        self.pos = sr.sweep_positions(self.base)
        self.image = IMAGE[name]
        self.counts = full_counts(self.base)
        self.sets = []
        families = {}
        for family, kind in SETS + ((("goal_pair", "free"),) if name == "V" else ()):
            lat = costed(name, family)
            if kind not in families:
                families[kind] = {"free": free_scenarios, "wall": wall_scenarios,
                                  "obstacles": obstacle_scenarios,
                                  "discount": lambda l: discount_scenarios(l, self.pos, self.image)}[kind](lat)
            self.sets.append(ScenarioSet(name, family, kind, lat, families[kind], OracleBackend(lat), self.pos))


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ---- what a lattice's sets exercise ----------------------------------------------------------------------------------------------------
COVERAGE_ITEMS = ("tie decided by the predecessor distance", "tie decided by the source node", "tied edges in different register chunks",
                  "tied edges in the register image and in the tail", "tied edges all in the tail beyond its first 64",
                  "as many tied edges as the node has in-edges", "goal unique", "goal decided by the distance", "goal decided by the node",
                  "tie on a reduced path", "tie in planning_range", "tie in default", "tie in left", "tie in right",
                  "discounted edge wins a tie in the register image", "discounted edge wins a tie in the tail",
                  "discounted edge loses a tie in the register image", "discounted edge loses a tie in the tail",
                  "scenario without a valid path", "planning_range and default elect differently",
                  "first blocked edges all in the tail, planning_range alone has a path",
                  "blocked edges all in the tail in front of the closest object's layer, planning_range leaves over one")


def coverage(c):
    """{item: number of occurrences} and {edge count: transitions on paths} over the oracle-agreeing paths of case ``c``."""
    n = dict.fromkeys(COVERAGE_ITEMS, 0)
    counts = dict.fromkeys(sorted(set(c.counts)), 0)
    img = c.image
    for st in c.sets:
        for s in np.nonzero(st.agree)[0]:
            paths = [p for p in st.dp[s] if p is not None]
            n["scenario without a valid path"] += not any(p.valid for p in paths)
            sl = st.scen[s]["start_node"][0]
            if st.blocked is not None and paths[0].filt == sr.F_PR and paths[0].valid and not any(p.valid for p in paths[1:]):
                l1 = (sl + 1) % st.lat.num_layers
                e0, e1 = (int(st.lat.in_ptr[st.lat.layer_off[l1]]), int(st.lat.in_ptr[st.lat.layer_off[l1 + 1]]))
                b = np.nonzero(st.blocked[s, e0:e1])[0]
                n["first blocked edges all in the tail, planning_range alone has a path"] += bool(len(b) and (c.pos[e0 + b] >= img).all())
            if st.blocked is not None and paths[0].filt == sr.F_PR and paths[0].valid:
                L_ = st.lat.num_layers
                l1 = (sl + 1) % L_
                e0, e1 = (int(st.lat.in_ptr[st.lat.layer_off[l1]]), int(st.lat.in_ptr[st.lat.layer_off[l1 + 1]]))
                b = np.nonzero(st.blocked[s, e0:e1])[0]
                first = st.lat.find_edge(sl, paths[0].nodes[0], l1, paths[0].nodes[1])
                ahead = (int(st.ref.closest_obj_node[s, 0]) - sl) % L_
                n["blocked edges all in the tail in front of the closest object's layer, planning_range leaves over one"] += bool(
                    ahead >= 2 and len(b) and (c.pos[e0 + b] >= img).all() and st.blocked[s, first])
            _, hit = sr.discounted_costs(st.lat, st.scen[s], W_LAST, np.ones(st.lat.num_nodes, bool))
            elected = {}
            for p in paths:
                if not p.valid:
                    continue
                for j in range(1, p.n_nodes):
                    counts[c.counts[(sl + j) % st.lat.num_layers]] += 1
                n[("goal unique", "goal decided by the distance", "goal decided by the node")[p.goal_level]] += 1
                for t in p.census:
                    pos = np.array(t.positions)
                    n["tie decided by the predecessor distance"] += t.level == sr.LEVEL_PRED_DIST
                    n["tie decided by the source node"] += t.level == sr.LEVEL_SOURCE
                    n["tied edges in different register chunks"] += len(set((pos[pos < img] // 64).tolist())) > 1
                    n["tied edges in the register image and in the tail"] += bool((pos < img).any() and (pos >= img).any())
                    n["tied edges all in the tail beyond its first 64"] += bool((pos >= img + 64).all())
                    n["as many tied edges as the node has in-edges"] += t.n_winners == t.in_degree
                    n["tie on a reduced path"] += bool(p.reduced)
                    n["tie in " + sr.FILTER_NAMES[p.filt]] += 1
                    for e in hit:
                        if e in t.edges:
                            where = "the register image" if c.pos[e] < img else "the tail"
                            n["discounted edge %s a tie in %s" % ("wins" if e == t.elected else "loses", where)] += 1
                    elected.setdefault((t.j, t.node), {})[p.filt] = t.elected
            n["planning_range and default elect differently"] += any(
                sr.F_PR in f and len(set(f.values())) > 1 for f in elected.values())
    return n, counts
