"""GPU: the layered shortest-path sweep (csrc/paths_team.hpp `team_layer`, `team_serial_node` / `team_relax_layer`, `team_resweep`, `team_goal`
and the run driver around them) against the layered DP of tests/sweep_ref.py, bit for bit, on the lattices and sets of
tests/sweep_cases.py: transitions of 63 .. 513 edges and whole ones around every size at which the layer step changes its form, exact ties
decided at every level of the rule, tied edges across register chunks, across the register image / tail boundary and deep in the tail,
the discounted edge in either place, reduced horizons, all four filters -- on every form of the path kernel: the one-wave batch kernel of
the lattice's plan class, the runtime plan (LTPL_NO_FIXED_PLAN), parent tables in global memory (LTPL_FORCE_LONG_HORIZON), four-wave teams
for batches (LTPL_BATCH_NW=4), the four-wave kernel in calls of fewer than 64 scenarios and the path stage of `tick_batch`.

`valid`, `action_id`, `reduced`, `goal_layer`, `n_nodes`, `n_ties` and `nodes` equal the DP on EVERY scenario; they equal the oracle wherever
the oracle equals the DP (everywhere but zero-cost edges on a range across the seam: tests/test_sweep_cases_host.py),
and there the rest of the result goes through `compare_results`; all forms of one lattice agree bit for bit.

Found by this test and fixed with it: `team_goal` flagged a goal tie only when two LANES attained the least total; in a layer of more
than 64 nodes (runtime plans) a lane holds two nodes, and a tie between exactly those two (nodes n and n + 64; family `goal_pair` on
lattice V) returned the right node with `n_ties` one too small -- 17 of 64 scenarios, batch and four-wave kernel alike.

Wall time on the MI355X (26 cases, 19 s in all): the first case of a lattice builds its lattice, both references and runs 15 sets --
R-batch 4.2 s, B-batch 3.4 s, V-batch 2.1 s, A-batch 1.9 s, C-batch 1.6 s; every other case 0.16 .. 0.28 s (15 handles, 1 100 .. 1 600
scenarios, results compared path by path).

Deliberate errors, ONE each in a scratch copy of csrc/paths_team.hpp (values only, never an address or a loop bound; none is kept), and what
fails -- "all forms" = batch, no_fixed_plan, long_horizon, batch_nw4, chunks, tick against the DP; a form that does not run the changed code
fails by its comparison with the batch kernel, or `ltpl_create` refuses the lattice because its self-test sees the one-wave and the
four-wave kernel disagree:
  election takes the LARGEST key (edge-parallel form)        every family with ties, all forms, all five lattices (316 of 320 `discount`
                                                             scenarios on A, 61 of 70 `ones/free`, 16 of 70 `magnitudes/free`)
  predecessor-distance round skipped for tail edges only     `int13/discount` on A, B, C, R in all forms (12 .. 15 of 320 scenarios on A / C);
                                                             `tenths/wall` C, R, `goal_zero/free` R, `int13/obstacles` R; `tenths/*` on A, B
                                                             refused at create
  NCHK instance chosen with `ne <= 65` (the 65th edge lost)  A and C, batch and tick: `tenths/free`, `zero_mixed/*`, `ones` / `int13/obstacles`;
                                                             `chunk_edges/free` refused at create; the other forms by comparison. Not seen
                                                             on B: no path there runs over the 65th edge of its two 65-edge transitions
  NCHK instance chosen with `<` for `<=`                      nothing fails, and nothing can: at 64 / 128 edges the larger instance processes one
                                                             more chunk whose lanes all lie beyond the transition and carry +inf -- the same
                                                             values, one chunk slower
  riding test ignores tail transitions                       `ones` / `int13` / `zero_mixed/obstacles` on A, B, C, R in the forms that ride (batch,
                                                             no_fixed_plan, tick), the other forms by comparison: the scenarios whose obstacle
                                                             beside the start node blocks edges beyond the register image only, with the
                                                             closest object's layer three layers on (without them: nothing failed)
  `team_goal` without its distance level                     `goal_ties/free` on all five lattices, all forms (31 of 70 scenarios on A, 50 of 88
                                                             on B); `magnitudes/free` on R
  discount not applied in the tail loop                      `int13/discount` on A, B, C, R, all forms (90 of 320 scenarios on A)
"""
import types

import numpy as np
import pytest

import sweep_cases as sc
import sweep_ref as sr
from test_gpu_assembly import environment, vel_inputs
from test_gpu_paths import compare_results
from graphbasedlocaltrajectoryplanner_amd import _capi

pytestmark = pytest.mark.gpu

ENV = {"batch": {}, "chunks": {}, "tick": {}, "no_fixed_plan": {"LTPL_NO_FIXED_PLAN": "1"}, "long_horizon": {"LTPL_FORCE_LONG_HORIZON": "1"},
       "batch_nw4": {"LTPL_BATCH_NW": "4"}}
CHUNK = 40                                                   # scenarios per call of the four-wave form (fewer than 64)
KERNEL_OF_CLASS = {"PlanRt": "6PlanRtE", "PlanFx<32,32,1>": "PlanFxILi32ELi32ELi1E", "PlanFx<32,40,1>": "PlanFxILi32ELi40ELi1E",
                   "PlanFx<48,32,1>": "PlanFxILi48ELi32ELi1E"}
RESULT_FIELDS = ("end_layer", "closest_obj_index", "closest_obj_node", "n_actions", "action_id", "valid", "reduced", "goal_layer", "n_nodes",
                 "n_pts", "n_ties", "nodes", "node_idx", "coeff", "path_param")

CASES = [(name, form) for name in ("A", "B", "C", "R") for form in ("batch", "no_fixed_plan", "long_horizon", "batch_nw4", "chunks", "tick")]
CASES += [("V", "batch"), ("V", "chunks")]

_base = {}                                                   # (lattice, set index) -> result of the batch form; one lattice at a time


@pytest.fixture(scope="module", autouse=True)
def drop_results():
    yield
    _base.clear()


def rows(res, idx):
    """A result restricted to the scenarios ``idx``, with the attributes `compare_results` reads."""
    out = types.SimpleNamespace(n_scen=len(idx))
    for f in RESULT_FIELDS:
        setattr(out, f, getattr(res, f)[idx])
    return out


def run_set(hip, st, form):
    """The whole set through one form: a result of len(st.scen) scenarios."""
    scen, n = st.scen, len(st.scen)
    if form == "tick":
        batch = sc.batch_of(scen)
        res, _ = hip.tick_batch(batch, vel_inputs(st.lat, scen))
        return res
    if form != "chunks":
        return hip.plan_paths(sc.batch_of(scen))
    parts = [hip.plan_paths(sc.batch_of(scen[lo:lo + CHUNK])) for lo in range(0, n, CHUNK)]
    out = hip.new_paths_result(n)
    for f in RESULT_FIELDS:
        getattr(out, f)[...] = np.concatenate([getattr(p, f) for p in parts])
    return out


def same_paths(res, base, what):
    """Two device results agree bit for bit: the integers whole, the path arrays as far as they are defined."""
    for f in RESULT_FIELDS[:11]:
        assert np.array_equal(getattr(res, f), getattr(base, f)), "%s: %s" % (what, f)
    for s, a in zip(*np.nonzero(base.valid)):
        nn, npts = int(base.n_nodes[s, a]), int(base.n_pts[s, a])
        for f, k in (("nodes", nn), ("node_idx", nn), ("coeff", nn - 1), ("path_param", npts)):
            assert np.array_equal(getattr(res, f)[s, a, :k], getattr(base, f)[s, a, :k]), "%s: %s of scenario %d slot %d" % (what, f, s, a)


def check_set(st, res, what):
    bad = [(s, sr.differences(st.dp[s], res, s)) for s in range(len(st.scen))]
    bad = [(s, d) for s, d in bad if d]
    assert not bad, "%s against the layered DP: %d of %d scenarios differ, first %s" % (what, len(bad), len(st.scen), bad[:5])
    idx = np.nonzero(st.agree)[0]
    for f in ("valid", "action_id", "reduced", "goal_layer", "n_nodes", "n_ties"):
        assert np.array_equal(getattr(res, f)[idx], getattr(st.ref, f)[idx]), "%s against the oracle: %s" % (what, f)
    compare_results(rows(res, idx), rows(st.ref, idx), st.lat)


def run_and_check(name, i, st, form, first):
    with environment(**ENV[form]):
        hip = _capi.HipBackend(st.lat)
    try:
        if first:
            sym = hip.paths_kernel_symbol(1)
            want = {"batch": KERNEL_OF_CLASS[sc.PLAN_CLASS[name]], "no_fixed_plan": KERNEL_OF_CLASS["PlanRt"], "long_horizon": "PlanRtG"}
            assert want.get(form, "") in sym, (name, form, sym)
        res = run_set(hip, st, form)
    finally:
        hip.close()
    what = "%s, form %s" % (st.label, form)
    if form == "batch":
        _base[(name, i)] = res
    check_set(st, res, what)
    if form != "batch":
        if (name, i) not in _base:                               # (this test alone: the batch form first)
            with environment():
                hip = _capi.HipBackend(st.lat)
            try:
                _base[(name, i)] = run_set(hip, st, "batch")
            finally:
                hip.close()
        same_paths(res, _base[(name, i)], what + " against the batch kernel")
    return res


@pytest.mark.parametrize("name,form", CASES, ids=["%s-%s" % c for c in CASES])
def test_sweep_matches_the_layered_dp(name, form):
    case = sc.case(name)
    for key in [k for k in _base if k[0] != name]:
        del _base[key]
    n_scen = n_paths = n_ties = 0
    failures = []                                                # every set is run: the message names all that fail, not the first
    for i, st in enumerate(case.sets):
        try:
            res = run_and_check(name, i, st, form, i == 0)
        except (AssertionError, _capi.BackendError) as e:
            failures.append("%s, form %s: %s" % (st.label, form, str(e)[:600]))
            continue
        n_scen, n_paths, n_ties = n_scen + len(st.scen), n_paths + int(res.valid.sum()), n_ties + int(res.n_ties.sum())
    print("lattice %s, form %s: %d of %d sets, %d scenarios, %d paths with %d ties on them equal the layered DP" % (
        name, form, len(case.sets) - len(failures), len(case.sets), n_scen, n_paths, n_ties))
    assert not failures, "%d of %d sets fail:\n%s" % (len(failures), len(case.sets), "\n".join(failures))
