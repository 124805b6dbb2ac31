"""GPU: the sweep driver of csrc/paths_team.hpp drops an overtaking filter whose frontier has died out (phase 4):
between two runs of layers it reads the reachability entry of the last layer every advancing filter went through, takes a filter whose
entry says "no node reached" out of the rest of the sweep and fills the rows it skips. Behind the closest object's layer the driver
therefore runs `planning_range | left | right`, `planning_range` plus ONE side (one layer body, the side a run-time value),
`planning_range` alone, or nothing at all -- and every one of those routes has to return what the full sweep returned.

Each test first takes a CENSUS OF ROUTES on the reference alone (tests/sweep_ref.py `Sweep`, per filter: the first layer without a
reachable node), asserts that its scenario set walks every route, and only then compares the device, bit for bit, with the layered DP
(`sweep_ref.plan_scenario`) and the oracle:

  headline   512 C2 scenarios on Monteblanco (`c2_scenarios(lat, 512, seed=1)`, W_LAST = 0, 0.5, 0.8 -- the benchmark's first 512), one-wave
             and four-wave teams, and once with the parent tables in global memory (LTPL_FORCE_LONG_HORIZON, kernel PlanRtG)
  lattices   the `obstacles` sets of tests/sweep_cases.py on A, B, C, R, V (every plan class, transitions at every chunk count, tails, the
             serial layer form), one-wave and four-wave teams

Routes (three-slot scenarios: follow on `planning_range`, left, right; "dead" = the filter does not reach the last layer):
  left dead / right alive, left alive / right dead, both dead, both alive;
  a side that dies ON its first own layer (the object layer), ONE layer later (the second single-layer run catches it), later than that (it
  keeps sweeping: the driver prunes behind the third run only), or in front of it (the shared `default` prefix died);
  the object on the start layer (the filter never starts); `planning_range` short of the last layer (the later slots inherit the reduced
  layer and read reachability rows of layers their own filter skipped).

Found by the census (deaths counted per filter at the first layer without a reachable node; an object on the start layer counts as a death
on the first own layer):
  headline  487 three-slot scenarios: 260 / 90 / 131 / 6; deaths 497 on the first own layer, 92 one layer later, 3 later, 20 in the prefix;
            object on the start layer 32, planning_range short of the last layer 6
  A          84: 19 / 28 / 35 / 2;  74, 21, 0, 22;  24, 1          B   112: 27 / 28 / 49 / 8;  95, 24, 0, 34;  34, 1
  C          84: 17 / 21 / 42 / 4;  85, 15, 0, 22;  23, 5          R    96: 25 / 20 / 49 / 2;  96, 25, 4, 18;  17, 7
  V          64: 12 / 13 / 36 / 3;  77, 10, 6,  4;  12, 13
Wall time on the MI355X: 15 s for the eight cases (R 4.2 s, B 3.7 s with the lattice's references, which tests/test_gpu_sweep.py shares;
the headline's references 1.4 s; every other case below 2 s).
"""
import collections
import os
import warnings

import numpy as np
import pytest

import sweep_cases as sc
import sweep_ref as sr
from helpers import GOLDEN
from test_gpu_assembly import environment
from test_gpu_paths import compare_results
from test_gpu_sweep import rows, same_paths
from graphbasedlocaltrajectoryplanner_amd import _capi
from graphbasedlocaltrajectoryplanner_amd.lattice import Lattice
from graphbasedlocaltrajectoryplanner_amd.scenario_gen import c2_scenarios

pytestmark = pytest.mark.gpu

W_LAST = [0.0, 0.5, 0.8]
N_HEADLINE = 512
ROUTES = ("left dead, right alive", "left alive, right dead", "both dead", "both alive")

Routes = collections.namedtuple("Routes", "three_slot route first_own one_later later prefix start_layer pr_short")


def death_layer(sw, n_trans):
    """First layer (counted from the start layer) on which the sweep ``sw`` reaches no node; None if it reaches the last one. (An empty
    frontier stays empty: a single first layer describes the filter.)"""
    for j in range(n_trans + 1):
        if not sw.reachable(j):
            return j
    return None


def census(lat, scen, blocked, closest_nodes, w_last):
    """The routes the sweep driver takes on a scenario set, from the reference alone: `Routes` of counters (``route``: {name: scenarios})."""
    L, off = lat.num_layers, lat.layer_off.astype(np.int64)
    layer_of = np.repeat(np.arange(L), lat.nodes_in_layer)
    route = dict.fromkeys(ROUTES, 0)
    n3 = first_own = one_later = later = prefix = start_layer = pr_short = 0
    for s, scn in enumerate(scen):
        cl = tuple(int(x) for x in closest_nodes[s])
        if cl[0] < 0 or not scn.get("action_sets", True):
            continue
        n3 += 1
        sl, sn = int(scn["start_node"][0]), int(scn["start_node"][1])
        n_trans = (lat.horizon_end_layer(sl) - sl) % L
        in_range = (layer_of - sl) % L <= n_trans
        for g in scn.get("zone_gids", ()):
            in_range[int(g)] = False
        cost, _ = sr.discounted_costs(lat, scn, w_last, in_range)
        jcl = (cl[0] - sl) % L
        start_layer += jcl == 0
        pr_short += death_layer(sr.Sweep(lat, sl, sn, n_trans, in_range, cost, None), n_trans) is not None
        dead = {}
        for filt in (sr.F_LEFT, sr.F_RIGHT):
            active = in_range.copy()
            n = np.arange(int(lat.nodes_in_layer[cl[0]]))
            active[off[cl[0]]:off[cl[0] + 1]] &= (n < cl[1]) if filt == sr.F_LEFT else (n >= cl[1])
            d = death_layer(sr.Sweep(lat, sl, sn, n_trans, active, cost, blocked[s]), n_trans)
            dead[filt] = d is not None
            if d is None:
                continue
            first_own += d == jcl
            one_later += d == jcl + 1
            later += d > jcl + 1
            prefix += d < jcl
        route[{(True, False): ROUTES[0], (False, True): ROUTES[1], (True, True): ROUTES[2], (False, False): ROUTES[3]}[
            (dead[sr.F_LEFT], dead[sr.F_RIGHT])]] += 1
    return Routes(n3, route, first_own, one_later, later, prefix, start_layer, pr_short)


def describe(c):
    return "%d three-slot scenarios: %s; deaths on the first own layer %d, one layer later %d, later %d, in the prefix %d; object on the " \
           "start layer %d, planning_range short of the last layer %d" % (
               c.three_slot, ", ".join("%s %d" % (r, c.route[r]) for r in ROUTES), c.first_own, c.one_later, c.later, c.prefix,
               c.start_layer, c.pr_short)


# ---- headline shapes -------------------------------------------------------------------------------------------------------------------
_headline = {}


def headline():
    """Lattice, scenarios, the oracle's result and mask, the DP's slots and the census: computed once, shared, left unchanged."""
    if not _headline:
        from oracle.oracle_lib import OracleBackend
        lat = Lattice.load(os.path.join(GOLDEN, "monteblanco_lattice.npz"))
        scen, _ = c2_scenarios(lat, N_HEADLINE, seed=1)
        ref, blocked = OracleBackend(lat).plan_paths_mask(_capi.PathsBatch(scen, w_last_edges=W_LAST))
        pos = sr.sweep_positions(lat)
        dp = []
        for s, scn in enumerate(scen):
            cl = tuple(int(x) for x in ref.closest_obj_node[s])
            dp.append(sr.plan_scenario(lat, scn, W_LAST, blocked[s], None if cl[0] < 0 else cl, pos))
        _headline.update(lat=lat, scen=scen, ref=ref, blocked=blocked, dp=dp,
                         census=census(lat, scen, blocked, ref.closest_obj_node, W_LAST))
    return _headline


@pytest.fixture(scope="module", autouse=True)
def drop_references():
    yield
    _headline.clear()
    _base.clear()


def assert_headline_routes(c):
    """What the issue found on this set (in brackets) with room below it: the set walks every route."""
    print("headline: " + describe(c))
    assert c.route[ROUTES[0]] >= 50 and c.route[ROUTES[1]] >= 50 and c.route[ROUTES[2]] >= 50, describe(c)      # (260, 90, 131)
    assert c.route[ROUTES[3]] >= 5, describe(c)                                                                # (6)
    assert c.one_later >= 20, describe(c)                                                                      # (72)
    assert c.later >= 1, describe(c)                                                                           # (3)
    assert c.start_layer >= 10, describe(c)                                                                    # (32)
    assert c.pr_short >= 3, describe(c)                                                                        # (6)


def check_headline(res, what):
    h = headline()
    bad = [(s, sr.differences(h["dp"][s], res, s)) for s in range(N_HEADLINE)]
    bad = [(s, d) for s, d in bad if d]
    assert not bad, "%s against the layered DP: %d of %d scenarios differ, first %s" % (what, len(bad), N_HEADLINE, bad[:5])
    ref = h["ref"]
    for f in ("end_layer", "closest_obj_node", "n_actions") + sr.INT_FIELDS:
        assert np.array_equal(getattr(res, f), getattr(ref, f)), "%s against the oracle: %s" % (what, f)
    for s, a in zip(*np.nonzero(ref.valid)):
        nn = int(ref.n_nodes[s, a])
        assert np.array_equal(res.nodes[s, a, :nn], ref.nodes[s, a, :nn]), "%s against the oracle: nodes of scenario %d slot %d" % (what, s, a)


def run_headline(env, symbol=None):
    h = headline()
    with environment(**env):
        hip = _capi.HipBackend(h["lat"])
    try:
        if symbol is not None:
            assert symbol in hip.paths_kernel_symbol(1), hip.paths_kernel_symbol(1)
        return hip.plan_paths(_capi.PathsBatch(h["scen"], w_last_edges=W_LAST))
    finally:
        hip.close()


_base = {}


@pytest.mark.parametrize("form", ["batch", "batch_nw4"])
def test_headline_routes_match_dp_and_oracle(form):
    assert_headline_routes(headline()["census"])
    res = run_headline({} if form == "batch" else {"LTPL_BATCH_NW": "4"}, "PlanFxILi32ELi32ELi1E" if form == "batch" else None)
    check_headline(res, "headline, form %s" % form)
    _base.setdefault("batch", res if form == "batch" else run_headline({}))
    same_paths(res, _base["batch"], "headline, form %s against the batch kernel" % form)


def test_headline_routes_with_parents_in_global_memory():
    assert_headline_routes(headline()["census"])
    res = run_headline({"LTPL_FORCE_LONG_HORIZON": "1"}, "PlanRtG")
    check_headline(res, "headline, form long_horizon")


# ---- every plan class and layer form ---------------------------------------------------------------------------------------------------
def lattice_census(name):
    """The routes of the `obstacles` sets of lattice ``name`` together (they share their scenarios; costs, and with them nothing of the
    reachability, differ), and the sets."""
    sets = [st for st in sc.case(name).sets if st.kind == "obstacles"]
    assert sets, name
    st = sets[0]
    return sets, census(st.lat, st.scen, st.blocked, st.ref.closest_obj_node, sc.W_LAST)


@pytest.mark.parametrize("name", ["A", "B", "C", "R", "V"])
def test_lattice_routes_match_dp_and_oracle(name):
    sets, c = lattice_census(name)
    print("lattice %s: %s" % (name, describe(c)))
    # the four routes on which the driver drops something: the three outcomes with a dead side, and a death ONE layer behind the first own
    # layer (what the second single-layer run is for). At most one may lack a scenario, and then the test says which; "both alive" may not.
    assert c.route[ROUTES[3]] > 0, "lattice %s: no scenario with both sides alive -- %s" % (name, describe(c))
    found = dict((r, c.route[r]) for r in ROUTES[:3])
    found["a side dies one layer behind its first own layer"] = c.one_later
    missing = [r for r, n in found.items() if n == 0]
    assert len(missing) <= 1, "lattice %s: routes without a scenario: %s -- %s" % (name, missing, describe(c))
    if missing:
        warnings.warn("lattice %s: ROUTE WITHOUT A SCENARIO: %s -- %s" % (name, missing[0], describe(c)))
    failures = []
    for st in sets:
        results = {}
        for form, env in (("batch", {}), ("batch_nw4", {"LTPL_BATCH_NW": "4"})):
            what = "%s, form %s" % (st.label, form)
            try:
                with environment(**env):
                    hip = _capi.HipBackend(st.lat)
                try:
                    res = results[form] = hip.plan_paths(sc.batch_of(st.scen))
                finally:
                    hip.close()
                bad = [(s, sr.differences(st.dp[s], res, s)) for s in range(len(st.scen))]
                bad = [(s, d) for s, d in bad if d]
                assert not bad, "%s against the layered DP: %d of %d scenarios differ, first %s" % (what, len(bad), len(st.scen), bad[:5])
                idx = np.nonzero(st.agree)[0]
                for f in sr.INT_FIELDS:
                    assert np.array_equal(getattr(res, f)[idx], getattr(st.ref, f)[idx]), "%s against the oracle: %s" % (what, f)
                compare_results(rows(res, idx), rows(st.ref, idx), st.lat)
                if form != "batch" and "batch" in results:
                    same_paths(res, results["batch"], what + " against the batch kernel")
            except (AssertionError, _capi.BackendError) as e:
                failures.append("%s: %s" % (what, str(e)[:600]))
    assert not failures, "%d comparisons fail:\n%s" % (len(failures), "\n".join(failures))
