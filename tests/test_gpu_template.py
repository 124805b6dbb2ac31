"""GPU: the integer decisions of the path kernel (csrc/paths_team.hpp phase 1: closest reference-line layer and planning-range gate; phase 3:
closest object, closest node, action template; phase 5: horizon back-off, `reduced`, the in_mod renaming, the invalidation of left / right)
AT THEIR DECISION BOUNDARIES, on the probe sets of tests/template_cases.py: positions on the bisector of two layers and of two nodes down to
adjacent doubles and exact fp64 ties (the seam pair and layers more than 10 apart included), each alone and beside a position exactly on a
border of the closest-layer grid, ties inside a forced full scan at every position count and segment count, the gate at sl - 2 .. el + 2,
layer distances H - 1 .. H + 1 and L - 1, index ties among 96 vehicles, first / last positions in different layers, the whole template
table, and zone walls with an object around the backed-off goal layer.

Every set runs through `plan_paths_mask` in the one-wave and the four-wave kernel on eight handles (default Monteblanco, runtime plan, long
horizon, no closest-layer grid, open, C, V, and c3 for the closest-layer sets). Held exactly: closest_obj_index, closest_obj_node, n_actions,
action_id, valid, reduced, goal_layer against the fp64 restatement of tests/template_ref.py (which tests/test_template_cases_host.py shows
equal to the oracle on every scenario); the mask over the active edges and the node lists against the oracle; then the paths through
`compare_results`. The two kernel forms of a handle agree bit for bit, and the handle without the grid agrees bit for bit with the default
one. A failure names the probes of every differing scenario: family, kind, offset, layers or nodes, vehicle, position, handle and form.

Measured on the MI355X: 53 tests (eight handles, 52 handle x set cases; the sets of the five lattices hold 16 010 scenarios, each run in both kernel forms) in 36 s; the
slowest case 4.7 s (C, layer set: 2 060 scenarios), c3 layer 3.4 s, Monteblanco layer 3.3 s, every other case below 2 s; creating the eight
handles 6.8 s. The device agreed everywhere. Six deliberate one-comparison edits of csrc/paths_team.hpp (not kept; table in DESIGN.md
section 2) each fail: `<=` for `<` in the candidate scan (16 cases) and in the full scan (15), `ld < H` (28), `n > cn` in the left filter
(1; 2 with the left-empty family of the object set that was added for it, both on lattice V), `cl < goal` in in_mod (11), the last instead of the first position
for vehicles >= 64 (7).
"""
import numpy as np
import pytest

import template_cases as tc
import template_ref as tr
from test_edge_mask import active_edges
from test_gpu_assembly import environment
from test_gpu_paths import compare_results
from test_gpu_sweep import same_paths
from test_template_cases_host import reference, _refs
from graphbasedlocaltrajectoryplanner_amd import _capi

pytestmark = pytest.mark.gpu

# handle -> (lattice of tests/template_cases.py, switches of ltpl_create, kernel symbol of the one-wave form)
HANDLES = {
    "monteblanco": ("monteblanco", {}, "PlanFxILi32ELi32ELi1E"),
    "monteblanco-runtime-plan": ("monteblanco", {"LTPL_NO_FIXED_PLAN": "1"}, "6PlanRtE"),
    "monteblanco-long-horizon": ("monteblanco", {"LTPL_FORCE_LONG_HORIZON": "1"}, "PlanRtG"),
    "monteblanco-no-grid": ("monteblanco", {"LTPL_NO_LAYER_GRID": "1"}, "PlanFxILi32ELi32ELi1E"),
    "open": ("open", {}, "PlanFxILi32ELi32ELi1E"),
    "C": ("C", {}, "PlanFxILi48ELi32ELi1E"),
    "V": ("V", {}, "6PlanRtE"),
    "c3": ("c3", {}, "PlanFxILi32ELi40ELi1E"),
}
CASES = [(h, which) for h, spec in HANDLES.items() for which in tc.set_names(spec[0])]

_handles, _default = {}, {}


def handle(name):
    if name not in _handles:
        with environment(**HANDLES[name][1]):
            _handles[name] = _capi.HipBackend(tc.lattice(HANDLES[name][0]))
    return _handles[name]


@pytest.fixture(scope="module", autouse=True)
def close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()
    _default.clear()
    _refs.clear()


def test_handles_run_the_kernels_they_stand_for():
    for name, (_, _, symbol) in HANDLES.items():
        assert symbol in handle(name).paths_kernel_symbol(1), (name, handle(name).paths_kernel_symbol(1))
    assert "PlanFxILi32ELi32ELi4E" in handle("monteblanco").paths_kernel_symbol(4)
    assert "PlanFxILi32ELi32ELi4E" in handle("monteblanco-no-grid").paths_kernel_symbol(4)


def run(hip, ref, nw):
    """The set's calls through one kernel form: [(result, mask)]."""
    return [hip.plan_paths_mask(batch, team_waves=nw) for _, batch, _, _ in ref.calls]


def check(name, which, nw, ref, out):
    cs, lat = ref.cs, ref.cs.lat
    bad = {}                                                     # scenario -> what differs
    for (lo, batch, ores, omask), (res, mask) in zip(ref.calls, out):
        for i in range(batch.n_scen):
            d = tr.differences(ref.rows[lo + i], res, i)
            if d:
                bad.setdefault(lo + i, []).extend(d)
        diff = (mask != omask) & active_edges(lat, batch)
        for i in np.nonzero(diff.any(axis=1))[0]:
            e = int(np.nonzero(diff[i])[0][0])
            bad.setdefault(lo + int(i), []).append("mask: %d edges differ (first: edge %d, hip %d oracle %d)" % (int(diff[i].sum()), e, mask[i, e], omask[i, e]))
        same = (res.n_nodes == ores.n_nodes) & (res.valid == ores.valid)
        for i, a in zip(*np.nonzero(ores.valid)):
            if not same[i, a] or not np.array_equal(res.nodes[i, a, :ores.n_nodes[i, a]], ores.nodes[i, a, :ores.n_nodes[i, a]]):
                bad.setdefault(lo + int(i), []).append("node list of slot %d" % a)
    report = []
    for s in sorted(bad)[:30]:
        probes = [tc.describe(cs, p) for p in cs.probes if p["scen"] == s] or ["(padding scenario %d)" % s]
        report.append("%s\n    %s" % ("; ".join(probes), "; ".join(bad[s][:4])))
    assert not bad, "handle %s, team of %d waves: %d of %d scenarios differ\n%s" % (name, nw, len(bad), len(cs.scen), "\n".join(report))
    for (_, _, ores, _), (res, _) in zip(ref.calls, out):          # (after the integers: a wrong decision is reported probe by probe,
        compare_results(res, ores, lat)                            # not through the paths it bends)


@pytest.mark.parametrize("name,which", CASES, ids=["%s-%s" % c for c in CASES])
def test_integer_decisions_equal_the_reference_at_their_boundaries(name, which):
    lattice_name = HANDLES[name][0]
    ref = reference(lattice_name, which)
    hip = handle(name)
    outs = {}
    for nw in (1, 4):
        outs[nw] = run(hip, ref, nw)
        check(name, which, nw, ref, outs[nw])
    for (a, _), (b, _) in zip(outs[1], outs[4]):
        same_paths(b, a, "%s %s: the four-wave against the one-wave kernel" % (name, which))
    if name == "monteblanco":
        _default[which] = outs
    if name == "monteblanco-no-grid":
        if which not in _default:                                # (this test alone: the default handle first)
            _default[which] = {nw: run(handle("monteblanco"), ref, nw) for nw in (1, 4)}
        for nw in (1, 4):
            for (a, ma), (b, mb) in zip(_default[which][nw], outs[nw]):
                same_paths(b, a, "%s, team of %d waves: without the closest-layer grid against the default handle" % (which, nw))
                assert np.array_equal(ma, mb), "%s, team of %d waves: the masks with and without the grid differ" % (which, nw)
        del _default[which]
    n_tie = sum(p["kind"] == "tie" for p in ref.cs.probes)
    print("%s %s: %d scenarios, %d probes (%d exact ties), both kernel forms" % (name, which, len(ref.cs.scen), len(ref.cs.probes), n_tie))
