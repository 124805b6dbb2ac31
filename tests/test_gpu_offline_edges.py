"""GPU: `k_offline_edges` through `offline_build.edges_on_device(hip_backend.lib)` AT ITS DECISION BOUNDARIES, against the long-double
reference of tests/offline_ref.py on the case families of tests/offline_cases.py (what each family holds and why its margins suffice is
asserted without a GPU by tests/test_offline_cases_host.py):

  * n_samples and valid EXACT on every edge of every call -- chords one part in 1e9 on either side of k x step, curvature limits one part in
    1e9 on either side of an edge's peak (the peak being the first or the last sample), edges that fill the staging capacity to the last row
    and edges one row too long, an edge of zero length, launches of 1, 63, 64, 65 and 129 edges;
  * every float -- coefficients, x, y, psi, kappa, element lengths, length, kappa_avg, kappa_range -- within `offline_cases.bounds()` over
    rows [0, n) of an edge: 100 x what an fp64 evaluation of the reference function deviates from long double (2e-9 of the scale for kappa,
    2e-11 for lengths, 7e-14 for psi and the coefficients on edges of 0.3 m and more), NOT the 1e-5 of the lattice tests; the element
    length of the last row 0. Rows at and beyond n_samples are unspecified: nothing is pre-filled and nothing asserted there;
  * given coefficients of race-line edges bit for bit; rows and scalars of an edge independent of cap_samples and of the edges around it,
    bit for bit;
  * the argument refusals of `ltpl_offline_edges`, a message for each, and a correct call afterwards.
Nothing here reads the reference checkout or oracle/_ref. The worst deviation so far is printed by every family (pytest -s); DESIGN.md
section 2 has the table and the list of deliberate errors each family catches.
"""
import ctypes as C

import numpy as np
import pytest

import offline_cases as oc
import offline_ref as oref
from graphbasedlocaltrajectoryplanner_amd import offline_build as ob

pytestmark = pytest.mark.gpu

LTPL_OK, LTPL_ERR_INVALID_ARG, LTPL_ERR_NO_DEVICE = 0, 1, 2
WORST = {}


@pytest.fixture
def on_device(hip_backend):
    return ob.edges_on_device(hip_backend.lib)           # (binds the argument types of the shared library object: once per test)


def run(on_device, call):
    """The call on the device, checked against the reference; returns the device's outputs."""
    got = on_device(*call.args)
    ref = oc.reference(call)
    dev = oref.check_call(got, ref, oc.bounds(), oc.STEP, call.name, call.labels)
    oref.merge_worst(WORST, dev, oref.edge_class(ref, oc.STEP))
    return got


def report():
    print(oc.format_table([("kernel on the device, worst so far", {cls: WORST.get(cls, dict.fromkeys(oref.QUANTITIES, 0.0)) for cls in ("regular", "micro")}),
                           ("  bound", oc.bounds())]))


def rows_equal(a, b, ea, eb, n):
    """Edge ``ea`` of the outputs ``a`` and edge ``eb`` of ``b`` agree bit for bit in everything the ABI specifies."""
    return (a["n_samples"][ea] == b["n_samples"][eb] == n and a["valid"][ea] == b["valid"][eb]
            and np.array_equal(a["coeff"][ea], b["coeff"][eb]) and np.array_equal(a["samples"][ea, :n], b["samples"][eb, :n])
            and all(a[k][ea] == b[k][eb] for k in ("length", "kappa_avg", "kappa_range")))


@pytest.mark.parametrize("name", ["step", "curved", "limits", "degenerate"])
def test_family_matches_the_long_double_reference(on_device, name):
    for call in oc.family(name):
        run(on_device, call)
    report()


def test_raceline_edges_keep_their_coefficients_and_pass_the_filter(on_device):
    (call,) = oc.raceline_family()
    got = run(on_device, call)
    rl = call.raceline_edge.astype(bool)
    assert np.array_equal(got["coeff"][rl].view(np.uint64), call.given[rl].view(np.uint64))          # bit for bit
    assert np.all(got["valid"][rl] == 1) and np.any(got["valid"][~rl] == 0)
    report()


def test_capacity_decides_per_edge_and_the_stride_follows_the_argument(on_device):
    fits, tight, wide = (run(on_device, c) for c in oc.capacity_family())
    ref = oc.reference(oc.capacity_family()[0])
    ns = ref["n_samples"]
    big = ns == ns.max()
    assert np.array_equal(tight["n_samples"], ns) and np.all(tight["valid"][big] == 0)               # refused, their n reported
    for e in range(ns.shape[0]):
        n = int(ns[e])
        assert rows_equal(fits, wide, e, e, n), "edge %d: cap %d against cap %d" % (e, ns.max(), ns.max() + 37)
        if not big[e]:
            assert rows_equal(fits, tight, e, e, n), "edge %d: unchanged next to a refused edge" % e
    report()


def test_every_launch_shape_gives_each_edge_what_the_full_launch_gives_it(on_device):
    base = run(on_device, oc.curved_call())
    ns = oc.reference(oc.curved_call())["n_samples"]
    for call in oc.shapes_family():
        got = run(on_device, call)
        for e in range(call.n_edges):
            assert rows_equal(got, base, e, 250 + e, int(ns[250 + e])), "%s / edge %d (%s)" % (call.name, e, call.labels[e])
    report()


# ---- argument refusals: decided on the host before any device work ------------------------------------------------------------------------

_pf64, _pi32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)


class EdgesIn(C.Structure):                                   # ltpl_offline_edges_in of include/ltpl_hip.h
    _fields_ = [("n_edges", C.c_int32), ("cap_samples", C.c_int32), ("stepsize_approx", C.c_double), ("kappa_max_turn", C.c_double),
                ("start_x", _pf64), ("start_y", _pf64), ("start_psi", _pf64), ("end_x", _pf64), ("end_y", _pf64), ("end_psi", _pf64),
                ("kappa_max_vel", _pf64), ("raceline_edge", _pi32), ("given_coeff", _pf64)]


class EdgesOut(C.Structure):                                  # ltpl_offline_edges_out
    _fields_ = [("n_samples", _pi32), ("valid", _pi32), ("coeff", _pf64), ("length", _pf64), ("kappa_avg", _pf64), ("kappa_range", _pf64),
                ("samples", _pf64)]


def test_argument_refusals(hip_backend, on_device):
    import torch
    lib = C.CDLL(hip_backend.lib_path)                 # the same library through function objects of its own: argument types set freely
    fn = lib.ltpl_offline_edges
    fn.argtypes, fn.restype = [C.c_int, C.c_void_p, C.c_void_p], C.c_int
    lib.ltpl_last_error.argtypes, lib.ltpl_last_error.restype = [C.c_void_p], C.c_char_p
    (call,) = oc.degenerate_family()
    n, cap = call.n_edges, call.cap
    cols = [np.ascontiguousarray(a) for a in (call.start[:, 0], call.start[:, 1], call.start[:, 2], call.end[:, 0], call.end[:, 1], call.end[:, 2],
                                              call.kappa_max_vel)]
    rl, given = np.ascontiguousarray(call.raceline_edge), np.ascontiguousarray(call.given)
    o = {"n_samples": np.zeros(n, np.int32), "valid": np.zeros(n, np.int32), "coeff": np.zeros((n, 8)), "length": np.zeros(n),
         "kappa_avg": np.zeros(n), "kappa_range": np.zeros(n), "samples": np.zeros((n, cap, 5))}

    def structs(**kw):
        i, out = EdgesIn(), EdgesOut()
        i.n_edges, i.cap_samples, i.stepsize_approx, i.kappa_max_turn = n, cap, oc.STEP, call.kappa_max_turn
        for (field, _), a in zip(EdgesIn._fields_[4:11], cols):
            setattr(i, field, a.ctypes.data_as(_pf64))
        i.raceline_edge, i.given_coeff = rl.ctypes.data_as(_pi32), given.ctypes.data_as(_pf64)
        for field, typ in EdgesOut._fields_:
            setattr(out, field, o[field].ctypes.data_as(typ))
        for k, v in kw.items():
            setattr(i, k, v)
        return i, out

    def call_abi(device, i, out):
        return fn(device, None if i is None else C.addressof(i), None if out is None else C.addressof(out))

    def refused(rc_want, device, i, out, what):
        rc = call_abi(device, i, out)
        assert rc == rc_want, "%s: status %d, expected %d" % (what, rc, rc_want)
        assert (lib.ltpl_last_error(None) or b"") != b"", "%s: no message" % what

    for what, kw in (("n_edges = 0", dict(n_edges=0)), ("cap_samples = 1", dict(cap_samples=1)), ("stepsize_approx = 0", dict(stepsize_approx=0.0)),
                     ("stepsize_approx < 0", dict(stepsize_approx=-2.5)), ("stepsize_approx = NaN", dict(stepsize_approx=float("nan")))):
        refused(LTPL_ERR_INVALID_ARG, -1, *structs(**kw), what)
    i, out = structs()
    refused(LTPL_ERR_INVALID_ARG, -1, None, out, "in = NULL")
    refused(LTPL_ERR_INVALID_ARG, -1, i, None, "out = NULL")
    refused(LTPL_ERR_NO_DEVICE, torch.cuda.device_count(), i, out, "device index = device count")
    assert not np.any(o["n_samples"]) and not np.any(o["samples"])          # no refusal wrote anything
    assert call_abi(-1, i, out) == LTPL_OK                                   # a correct call afterwards succeeds
    oref.check_call(o, oc.reference(call), oc.bounds(), oc.STEP, "after the refusals", call.labels)
    run(on_device, call)
