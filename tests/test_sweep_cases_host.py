"""CPU: the two references of the sweep tests side by side -- the oracle's Dijkstra and the layered DP of tests/sweep_ref.py agree on every
scenario of every set of tests/sweep_cases.py (nodes, n_ties, goal layer, action ids), with ONE named exception: zero-cost edges on a
planning range that crosses the seam; and the sets exercise what they were generated for, measured on the DP's
census of the agreeing paths, so that a generator that silently stops producing a class fails here and not on the device."""
import numpy as np
import pytest

import sweep_cases as sc
import sweep_ref as sr
from graphbasedlocaltrajectoryplanner_amd.synthetic_lattice import make_oval_lattice

COVERED = ("A", "B", "C", "R")


@pytest.mark.parametrize("name", COVERED + ("V",))
def test_layered_dp_equals_the_oracle(name):
    case = sc.case(name)
    n_total = n_diff = n_seam_zero = 0
    for st in case.sets:
        bad = np.nonzero(~st.agree)[0]
        n_total += len(st.scen)
        n_diff += len(bad)
        print("%-28s %4d scenarios, %3d cross the seam, %4d valid paths, %5d ties on them, references differ on %d" % (
            st.label, len(st.scen), int(st.crosses_seam.sum()), int(st.ref.valid.sum()), int(st.ref.n_ties.sum()), len(bad)))
        if st.family in sc.ZERO_FAMILIES:
            assert st.crosses_seam[bad].all(), "%s: the references differ on a range that does not cross the seam: scenarios %s (%s)" % (
                st.label, bad[~st.crosses_seam[bad]][:10].tolist(), st.diff[int(bad[~st.crosses_seam[bad]][0])])
            n_seam_zero += len(bad)
            for s in bad:                                            # both paths cost the same: the difference is the choice among ties
                for a, p in enumerate(st.dp[s]):
                    if p is not None and p.valid and st.ref.valid[s, a]:
                        assert path_cost(st, s, p.nodes) == path_cost(st, s, st.ref.nodes[s, a, :int(st.ref.n_nodes[s, a])].tolist()), (st.label, s, a)
        else:
            assert len(bad) == 0, "%s: the references differ on scenarios %s: %s" % (st.label, bad[:10].tolist(), st.diff[int(bad[0])])
    print("lattice %s: the layered DP and the oracle differ on %d of %d scenarios, all %d with zero-cost edges on a range across the seam" % (
        name, n_diff, n_total, n_seam_zero))
    assert n_diff == n_seam_zero
    if name != "V":                                                  # (on V the seam lies between two serial layers)
        assert n_seam_zero > 0, "the zero-cost families no longer show the settle-order difference at the seam"


def path_cost(st, s, nodes):
    """Cost of a path as the sweep adds it up (discounted edge costs, in order), plus the goal cost."""
    lat, (sl, _) = st.lat, st.scen[s]["start_node"]
    cost, _ = sr.discounted_costs(lat, st.scen[s], sc.W_LAST, np.ones(lat.num_nodes, bool))
    d = 0.0
    for j in range(1, len(nodes)):
        d = d + cost[lat.find_edge((sl + j - 1) % lat.num_layers, nodes[j - 1], (sl + j) % lat.num_layers, nodes[j])]
    return d + lat.vgoal_cost[lat.layer_off[(sl + len(nodes) - 1) % lat.num_layers] + nodes[-1]]


@pytest.mark.parametrize("name", COVERED)
def test_sets_cover_what_they_were_generated_for(name):
    case = sc.case(name)
    items, counts = sc.coverage(case)
    print("lattice %s (%s, register image %d edges)" % (name, sc.PLAN_CLASS[name], case.image))
    for k in sc.COVERAGE_ITEMS:
        print("    %-56s %6d" % (k, items[k]))
    print("    transitions on paths by edge count: %s" % ", ".join("%d: %d" % kv for kv in sorted(counts.items())))
    want = set(sc.chosen_counts(max(case.counts), int(case.base.nodes_in_layer[0])))
    assert set(counts) == want, sorted(set(counts) ^ want)
    missing = [k for k in sc.COVERAGE_ITEMS if not items[k]] + ["%d edges" % k for k, v in counts.items() if not v]
    assert not missing, "lattice %s: not on any oracle-agreeing path: %s" % (name, missing)


def test_alternating_widths_cover_their_hand_overs():
    """Lattice V: paths through the one-node layer, ties whose tied sources include ids above 63 into an edge-parallel (40-node) layer,
    ties into serial (70-node) layers, and serial and edge-parallel layers in turns on every path."""
    case = sc.case("V")
    lat = case.base
    assert sorted(set(lat.nodes_in_layer.tolist())) == [1, 40, 70]
    n = dict.fromkeys(("through the one-node layer", "tie into a 40-node layer with a source above 63", "tie into a 70-node layer",
                       "tie into the one-node layer", "tie behind the one-node layer", "goal tied between two nodes 64 apart"), 0)
    one = int(np.nonzero(lat.nodes_in_layer == 1)[0][0])
    for st in case.sets:
        for s in np.nonzero(st.agree)[0]:
            sl = st.scen[s]["start_node"][0]
            for p in st.dp[s]:
                if p is None or not p.valid:
                    continue
                on_path = [(sl + j) % lat.num_layers for j in range(p.n_nodes)]
                n["through the one-node layer"] += one in on_path[1:-1]
                for t in p.census:
                    k = int(lat.nodes_in_layer[t.layer])
                    src = [int(st.lat.edge_src[e]) for e in t.edges]
                    n["tie into a 40-node layer with a source above 63"] += k == 40 and max(src) > 63
                    n["tie into a 70-node layer"] += k == 70
                    n["tie into the one-node layer"] += k == 1
                    n["tie behind the one-node layer"] += one in on_path[1:t.j]
    pair = [st for st in case.sets if st.family == "goal_pair"][0]
    for s in np.nonzero(pair.agree)[0]:                          # the goal tie between nodes 2 and 66 alone, the path otherwise unique or not
        p = pair.dp[s][0]
        if p.valid and int(lat.nodes_in_layer[p.goal_layer]) == 70 and p.goal_level == sr.LEVEL_SOURCE:
            assert p.nodes[-1] == 2
            n["goal tied between two nodes 64 apart"] += 1
    print("\n".join("    %-56s %6d" % kv for kv in n.items()))
    assert all(n.values()), n


def test_pruning_keeps_the_chosen_counts_and_the_geometry():
    full = make_oval_lattice(**sc.LATTICE_ARGS["A"])
    lat = sc.lattice("A")
    cc = sc.chosen_counts(sc.full_counts(full)[0], 24)
    assert sc.full_counts(lat) == [cc[l % len(cc)] for l in range(lat.num_layers)]
    assert {63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320, 321, 511, 512, 513, 576} == set(cc)
    assert np.array_equal(lat.node_pos, full.node_pos) and np.all(np.diff(lat.in_ptr) >= 1)
    # every kept edge is the generator's edge between the same two nodes, samples and coefficients included
    for e in range(0, lat.num_edges, 97):
        v = int(np.searchsorted(lat.in_ptr, e, side="right") - 1)
        l = int(lat.layer_of(v))
        f = full.find_edge((l - 1) % lat.num_layers, int(lat.edge_src[e]), l, v - int(lat.layer_off[l]))
        assert f >= 0 and lat.edge_len[e] == full.edge_len[f] and np.array_equal(lat.edge_coeff[e], full.edge_coeff[f])
        assert np.array_equal(lat.samples[lat.samp_ptr[e]:lat.samp_ptr[e + 1]], full.samples[full.samp_ptr[f]:full.samp_ptr[f + 1]])
    # a source node without an out-edge
    sl, sn, _, _ = lat.edge_endpoints()
    assert not np.any((sl == 2) & (sn == sc.NO_OUT_NODE)) and np.any((sl == 3) & (sn == sc.NO_OUT_NODE))


def test_sweep_positions_follow_rank_then_destination():
    lat = sc.lattice("A")
    pos = sr.sweep_positions(lat)
    off, in_ptr = lat.layer_off, lat.in_ptr
    for l in (0, 5, lat.num_layers - 1):
        e0, e1 = int(in_ptr[off[l]]), int(in_ptr[off[l + 1]])
        assert sorted(pos[e0:e1].tolist()) == list(range(e1 - e0))
        by_pos = sorted(range(e0, e1), key=lambda e: pos[e])
        keys = []
        for e in by_pos:
            v = int(np.searchsorted(in_ptr, e, side="right") - 1)
            keys.append((e - int(in_ptr[v]), v))
        assert keys == sorted(keys)
