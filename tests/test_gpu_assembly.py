"""GPU: the path assembly (csrc/paths_team.hpp `team_assemble_rest`: edge look-up, gather, slope solve, coefficients, re-sampling, heading,
curvature) against the long-double reference of tests/spline_ref.py at ASSEMBLY_TOL = 1e-10, at EVERY segment count N the lattices of
tests/assembly_cases.py allow (1 .. 67: both sides of the switch from cyclic reduction to the serial elimination at 63 / 64, and the small N
at which a missing reduction round is not damped away), on every form of the path kernel: one-wave batch kernel, four-wave kernel, the
path stage of `tick_batch`, parent tables in global memory, in-edges by rank instead of by node record. Integers and the element-length
column are bit-exact against the oracle; all forms of one lattice agree bit for bit.

Measured on the MI355X, worst deviation from the reference (the forms of one lattice agree bit for bit, so there is one value per lattice;
the oracle's own, on the CPU: coefficients 1.1e-12, kappa 1.2e-12, xy 4.3e-15, psi 1.1e-15):
    S  coefficients 4.4e-13  kappa 1.4e-14  xy 3.6e-15  psi 2.5e-15        A  5.3e-12  7.7e-15  4.2e-15  2.6e-15
    B  coefficients 1.4e-13  kappa 7.9e-15  xy 4.2e-15  psi 2.7e-15        C  1.1e-13  6.3e-15  3.8e-15  2.3e-15"""
import contextlib
import os

import numpy as np
import pytest

import assembly_cases as ac
import spline_ref as sr
from spline_ref import ASSEMBLY_TOL
from graphbasedlocaltrajectoryplanner_amd import _capi

pytestmark = pytest.mark.gpu

INT_FIELDS = ("end_layer", "closest_obj_index", "closest_obj_node", "n_actions", "action_id", "valid", "reduced", "goal_layer", "n_nodes",
              "n_pts", "n_ties")
KERNEL_OF_CLASS = {"PlanRt": "6PlanRtE", "PlanFx<32,32,1>": "PlanFxILi32ELi32ELi1E", "PlanFx<32,40,1>": "PlanFxILi32ELi40ELi1E",
                   "PlanFx<48,32,1>": "PlanFxILi48ELi32ELi1E"}
CHUNK = 40                                                   # scenarios per call of the four-wave form (fewer than 64)

CASES = [(name, form) for name in ("S", "A", "B", "C") for form in ("batch", "chunks", "tick")]
CASES += [("S", "long_horizon"), ("A", "no_fixed_plan")]

_handles, _results = {}, {}


@contextlib.contextmanager
def environment(**env):
    """The switches `ltpl_create` reads, for the creation of one handle."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def handle(name, variant="default"):
    if (name, variant) not in _handles:
        env = {"default": {}, "long_horizon": {"LTPL_FORCE_LONG_HORIZON": "1"}, "no_fixed_plan": {"LTPL_NO_FIXED_PLAN": "1"}}[variant]
        with environment(**env):
            _handles[(name, variant)] = _capi.HipBackend(ac.lattice(name))
    return _handles[(name, variant)]


@pytest.fixture(scope="module", autouse=True)
def close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()
    _results.clear()


def whole_set(scen):
    """The set in one call of the one-wave batch kernel (at least 64 scenarios: a short set is repeated)."""
    out = list(scen) * (1 if len(scen) >= 64 else 2)
    assert 64 <= len(out) <= 140
    return out


def vel_inputs(lat, scen):
    n = len(scen)
    params = _capi.VelParamSet(len_veh=lat.veh_length)
    pos = np.array([lat.node_pos[lat.layer_off[s["start_node"][0]] + s["start_node"][1]] for s in scen])
    n_veh = sum(len(s["vehicles"]) for s in scen)
    return _capi.TickVelBatch(params, n, np.full(n, 20.0), np.full(n, 20.0), pos, np.zeros(n_veh))


def paths_of(res, offset, paths):
    """{(s, a): the arrays of one path} of scenarios ``offset`` .. of a set, from a result that starts at scenario ``offset``."""
    out = {}
    for s, a, nn, npts in paths:
        k = s - offset
        if 0 <= k < res.n_scen:
            out[(s, a)] = (res.nodes[k, a, :nn].copy(), res.node_idx[k, a, :nn].copy(), res.coeff[k, a, :nn - 1].copy(),
                           res.path_param[k, a, :npts].copy())
    return out


def run_form(name, form):
    """(integer outputs of the set, {(s, a): path arrays}) of one kernel form on lattice ``name``; computed once."""
    if (name, form) in _results:
        return _results[(name, form)]
    case = ac.case(name)
    scen, n = case.scen, len(case.scen)
    hip = handle(name, form if form in ("long_horizon", "no_fixed_plan") else "default")
    calls = []                                               # (first scenario, result)
    if form in ("batch", "long_horizon", "no_fixed_plan"):
        calls.append((0, hip.plan_paths(ac.batch_of(whole_set(scen)))))
    elif form == "chunks":
        for lo in range(0, n, CHUNK):
            calls.append((lo, hip.plan_paths(ac.batch_of(scen[lo:lo + CHUNK]))))
    elif form == "tick":
        # the pipeline's path kernel on the whole set (and the fused tick kernel on its first scenarios): the path outputs are those of
        # plan_paths on the same call, bit for bit
        for group in (scen[:CHUNK], whole_set(scen)):
            batch = ac.batch_of(group)
            res, _ = hip.tick_batch(batch, vel_inputs(case.lat, group))
            alone = hip.plan_paths(batch)
            for f in INT_FIELDS:
                assert np.array_equal(getattr(res, f), getattr(alone, f)), "tick_batch against plan_paths, %d scenarios: %s" % (len(group), f)
            got, exp = paths_of(res, 0, case.paths), paths_of(alone, 0, case.paths)
            assert got.keys() == exp.keys() and all(np.array_equal(x, y) for k in got for x, y in zip(got[k], exp[k])), \
                "tick_batch against plan_paths, %d scenarios: path outputs" % len(group)
            if len(group) >= n:
                calls.append((0, res))
            else:
                small = got
    ints = {f: np.concatenate([getattr(r, f)[:n - lo] for lo, r in calls]) for f in INT_FIELDS}
    paths = {}
    for lo, r in calls:
        paths.update(paths_of(r, lo, case.paths))
    if form == "tick":                                       # the fused tick kernel's paths are the pipeline's
        for key, arrays in small.items():
            assert all(np.array_equal(x, y) for x, y in zip(arrays, paths[key])), "fused tick against the pipeline, path %s" % (key,)
    if form in ("long_horizon", "no_fixed_plan"):            # ... and its four-wave kernel
        for lo in range(0, n, CHUNK):
            for key, arrays in paths_of(hip.plan_paths(ac.batch_of(scen[lo:lo + CHUNK])), lo, case.paths).items():
                assert all(np.array_equal(x, y) for x, y in zip(arrays, paths[key])), "%s: four-wave against one-wave kernel, path %s" % (form, key)
    _results[(name, form)] = (ints, paths)
    return _results[(name, form)]


def test_lattices_land_in_their_plan_classes():
    for name in ("S", "A", "B", "C"):
        lat, hip = ac.lattice(name), handle(name)
        assert hip.caps.max_path_nodes == lat.max_horizon()[0]
        assert ac.plan_class_of(lat) == ac.PLAN_CLASS[name]
        assert KERNEL_OF_CLASS[ac.PLAN_CLASS[name]] in hip.paths_kernel_symbol(1), (name, hip.paths_kernel_symbol(1))
    assert KERNEL_OF_CLASS["PlanRt"] in handle("A", "no_fixed_plan").paths_kernel_symbol(1)
    assert "PlanRtG" in handle("S", "long_horizon").paths_kernel_symbol(1)            # (parent tables in global memory)


@pytest.mark.parametrize("name,form", CASES, ids=["%s-%s" % c for c in CASES])
def test_assembly_matches_the_long_double_reference(name, form):
    case = ac.case(name)
    ac.assert_coverage(name, case.lat, case.scen, case.ref)
    ints, paths = run_form(name, form)
    for f in INT_FIELDS:                                    # as everywhere in the suite: integers bit-exact against the oracle
        assert np.array_equal(ints[f], getattr(case.ref, f)), "%s %s: %s" % (name, form, f)
    assert set(paths) == set(case.assembly)
    worst, failures = {}, []
    for s, a, nn, npts in case.paths:
        nodes, idx, coeff, pp = paths[(s, a)]
        assert np.array_equal(nodes, case.ref.nodes[s, a, :nn]) and np.array_equal(idx, case.ref.node_idx[s, a, :nn]), (name, form, s, a)
        assert np.array_equal(pp[:, 4], case.ref.path_param[s, a, :npts, 4]), "%s %s s%d a%d: element lengths" % (name, form, s, a)
        dev = sr.assembly_deviation(coeff, pp, case.assembly[(s, a)])
        sr.merge_worst(worst, dev)
        if not all(v <= ASSEMBLY_TOL for v in dev.values()):
            failures.append("s%d a%d N %d rows %d: %s" % (s, a, nn - 1, npts, ", ".join("%s %.2e" % kv for kv in sorted(dev.items()))))
    msg = "lattice %s, form %s, kernel against the long-double reference, worst deviation: %s" % (
        name, form, ", ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    print(msg)
    assert not failures, msg + "\n" + "\n".join(failures[:20])
    for s, a, _, _ in case.paths[::7]:                      # (and through the checker itself)
        sr.assert_assembly_close(paths[(s, a)][2:], case.assembly[(s, a)], ASSEMBLY_TOL, "%s %s s%d a%d" % (name, form, s, a))
    # all forms of one lattice agree bit for bit on every output
    base_ints, base_paths = run_form(name, "batch")
    for f in INT_FIELDS:
        assert np.array_equal(ints[f], base_ints[f]), "%s: form %s against the batch kernel: %s" % (name, form, f)
    for key, arrays in paths.items():
        for x, y, what in zip(arrays, base_paths[key], ("nodes", "node_idx", "coeff", "path_param")):
            assert np.array_equal(x, y), "%s: form %s against the batch kernel, path %s: %s" % (name, form, key, what)
