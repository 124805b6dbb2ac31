"""GPU: the obstacle x edge mask of the path kernel (csrc/paths_team.hpp phase 2, table of csrc/capsule.hpp) AT ITS DECISION BOUNDARIES, bit for
bit against the oracle's mask (pinned to the reference's own edge sets by tests/test_edge_mask.py) on the probe sets of tests/mask_cases.py:
queries on the boundary of the exact fp64 sample test (down to adjacent doubles and exact ties), on both boundaries of the fp32 capsule cull
and in the cusps between two samples, every vehicle with a radius of its own, alone and among up to 191 filler positions that fill the shell
list -- in the one-wave and the four-wave kernel, on every plan class (32x32, 32x40, 48x32, the runtime plan with its shell list of 128
entries, parent tables in global memory), on a planning range of 67 layers (every transition walked) and across the seam.
tests/test_mask_cases_host.py shows on the CPU that the oracle alone satisfies what is asserted here and that the sets populate the cull's
three classes; the same is asserted here for what is actually sent to the device.

A failure names every differing probe: edge, offset, ray family, radius, cull class, position index.

Measured on the MI355X: 29 tests in 32 s, the slowest case 2.3 s (C, gap rays: 3 526 scenarios in both kernel forms), creating the eight
handles 5.5 s. Builds with one deliberate error each (not kept) fail as they should: `<` for `<=` in flush_shell fails the tie probes and
o = 0 probes of 24 cases; qlm without the slack fails o <= 0 probes of the apex rays on Monteblanco and the open lattice (15 of 3 170); hg2 = 0
fails 700 of 3 175 gap-ray probes on Monteblanco (129 of the sample family); lane 0's threshold for every shell entry fails the probe + filler
cases only (103 of 300 on Monteblanco), on every handle.
"""
import numpy as np
import pytest

import mask_cases as mc
from test_capsule_cull import capsules, kernel_decisions
from test_edge_mask import active_edges
from test_gpu_assembly import environment
from test_gpu_paths import compare_results
from graphbasedlocaltrajectoryplanner_amd import _capi

pytestmark = pytest.mark.gpu

W_LAST = [0.0, 0.5, 0.8]
MAX_CALL = 512                                               # scenarios per call where the mask array is large (C3: 98 000 edges)
# handle -> (lattice of tests/mask_cases.py, switches of ltpl_create, kernel symbol of the one-wave form, sets)
HANDLES = {
    "monteblanco": ("monteblanco", {}, "PlanFxILi32ELi32ELi1E", ("sample", "gap", "seam", "fillers")),
    "monteblanco-runtime-plan": ("monteblanco", {"LTPL_NO_FIXED_PLAN": "1"}, "6PlanRtE", ("sample", "gap", "fillers")),
    "monteblanco-long-horizon": ("monteblanco", {"LTPL_FORCE_LONG_HORIZON": "1"}, "PlanRtG", ("sample", "gap", "fillers")),
    "open": ("open", {}, "PlanFxILi32ELi32ELi1E", ("sample", "gap", "seam")),
    "S": ("S", {}, "6PlanRtE", ("sample", "gap", "seam", "fillers")),
    "B": ("B", {}, "PlanFxILi32ELi40ELi1E", ("sample", "gap", "seam", "fillers")),
    "C": ("C", {}, "PlanFxILi48ELi32ELi1E", ("sample", "gap", "seam", "fillers")),
    "c3": ("c3", {}, "PlanFxILi32ELi40ELi1E", ("sample", "gap", "fillers")),
}
CASES = [(h, which) for h, spec in HANDLES.items() for which in spec[3]]
N_VARIANT_FILLERS = 100                                      # probe + filler scenarios on the two further Monteblanco handles

_handles, _oracles, _refs, _caps = {}, {}, {}, {}


def handle(name):
    if name not in _handles:
        with environment(**HANDLES[name][1]):
            _handles[name] = _capi.HipBackend(mc.lattice(HANDLES[name][0]))
    return _handles[name]


@pytest.fixture(scope="module", autouse=True)
def close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()
    _refs.clear()


def reference(lattice_name, which, limit):
    """[(first scenario, batch, oracle result, oracle mask)] of a set in calls of at most MAX_CALL scenarios; computed once and left unchanged."""
    key = (lattice_name, which, limit)
    if key not in _refs:
        from oracle.oracle_lib import OracleBackend
        if lattice_name not in _oracles:
            _oracles[lattice_name] = OracleBackend(mc.lattice(lattice_name))
        scen = mc.case_set(lattice_name, which).scen[:limit]
        n_calls = -(-len(scen) // MAX_CALL) if lattice_name == "c3" else 1
        size = -(-len(scen) // n_calls)
        assert size >= 64                                    # (the one-wave form needs 64 scenarios)
        _refs[key] = []
        for lo in range(0, len(scen), size):
            batch = _capi.PathsBatch(scen[lo:lo + size], w_last_edges=W_LAST)
            _refs[key].append((lo, batch) + _oracles[lattice_name].plan_paths_mask(batch))
    return _refs[key]


def cull_class(lattice_name, p):
    """'MISS' / 'HIT' / 'shell' per probe, by the restatement of the cull in tests/test_capsule_cull.py."""
    if lattice_name not in _caps:
        _caps[lattice_name] = capsules(mc.lattice(lattice_name))[:2]
    cap, slack = _caps[lattice_name]
    miss, hit = kernel_decisions(cap[p.edge], slack, p.qx, p.qy, np.sqrt(p.thr2))
    return np.where(miss, "MISS", np.where(hit, "HIT", "shell"))


def test_handles_run_the_kernels_they_stand_for():
    for name, (_, _, symbol, _) in HANDLES.items():
        assert symbol in handle(name).paths_kernel_symbol(1), (name, handle(name).paths_kernel_symbol(1))
    assert "PlanFxILi32ELi32ELi4E" in handle("monteblanco").paths_kernel_symbol(4)
    assert mc.lattice("S").max_horizon()[0] - 1 > 63                                   # every transition walked, no sparse bit set


@pytest.mark.parametrize("name,which", CASES, ids=["%s-%s" % c for c in CASES])
def test_mask_equals_the_oracle_at_the_decision_boundaries(name, which):
    lattice_name = HANDLES[name][0]
    lat, hip = mc.lattice(lattice_name), handle(name)
    cs = mc.case_set(lattice_name, which)
    limit = N_VARIANT_FILLERS if (which == "fillers" and HANDLES[name][1]) else len(cs.scen)
    p = cs.probes.take(np.arange(limit))
    pos_index = cs.pos_index[:limit]
    # what goes to the device holds the three classes of the cull and the ties (a later edit to the generators must not empty one quietly)
    cls = cull_class(lattice_name, p)
    shares = {c: float(np.mean(cls == c)) for c in ("MISS", "HIT", "shell")}
    assert min(shares.values()) >= 0.03, (name, which, shares)
    n_tie = int((p.family == mc.FAMILIES.index("tie")).sum())
    if which in ("sample", "gap"):
        assert n_tie + int((mc.case_set(lattice_name, "gap" if which == "sample" else "sample").probes.family == 2).sum()) >= 1, "no tie probes"
        assert int((p.offset == 0.0).sum()) >= 30 and len(set(p.offset.tolist())) == len(mc.OFFSETS)
    if which == "fillers":
        assert int((pos_index >= 64).sum()) >= 5 and int((pos_index >= 128).sum()) >= 2
    calls = reference(lattice_name, which, limit)
    expected = np.concatenate([om[np.arange(b.n_scen), p.edge[lo:lo + b.n_scen]] for lo, b, _, om in calls]).astype(bool)
    assert not np.any(expected & ~p.exact) and expected[p.exact].mean() >= 0.75             # (tests/test_mask_cases_host.py)
    for nw in (1, 4):
        got = np.zeros(p.n, bool)
        problems, planned = [], []
        for lo, batch, ores, omask in calls:
            res, mask = hip.plan_paths_mask(batch, team_waves=nw)
            got[lo:lo + batch.n_scen] = mask[np.arange(batch.n_scen), p.edge[lo:lo + batch.n_scen]]
            diff = (mask != omask) & active_edges(lat, batch)
            if diff.any():
                s, e = [int(x[0]) for x in np.nonzero(diff)]
                problems.append("%d edges differ (first: scenario %d edge %d, hip %d oracle %d)" % (int(diff.sum()), lo + s, e, mask[s, e], omask[s, e]))
            planned.append((res, ores))
        bad = np.nonzero(got != expected)[0]
        report = ["scenario %d: edge %d offset %+.0e %s ray radius %.6f class %s position %d: hip %d oracle %d (exact test: %d)" % (
            i, p.edge[i], p.offset[i], mc.FAMILIES[p.family[i]], p.radius[i], cls[i], pos_index[i], got[i], expected[i], p.exact[i]) for i in bad[:40]]
        assert not len(bad) and not problems, "%s %s, team of %d waves: %d of %d probes differ\n%s\n%s" % (
            name, which, nw, len(bad), p.n, "\n".join(report), "\n".join(problems))
        for res, ores in planned:                            # the diagnostic call plans like ltpl_plan_paths (after the masks: a wrong
            compare_results(res, ores, lat)                  # mask is reported probe by probe, not through the paths it bends)
    print("%s %s: %d probes (%d ties), certain MISS %.3f, certain HIT %.3f, shell %.3f; %d blocked" % (
        name, which, p.n, n_tie, shares["MISS"], shares["HIT"], shares["shell"], int(expected.sum())))
