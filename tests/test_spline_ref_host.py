"""CPU: the long-double reference of the path assembly (tests/spline_ref.py) and its checker, without a GPU -- the oracle stays within
ASSEMBLY_TOL of the reference on every scenario set of tests/assembly_cases.py, the reference agrees with scipy's clamped CubicSpline, the
scenario sets cover what they claim, and the checker rejects the small errors the 1e-5 bound of the parity suite lets through."""
import numpy as np
import pytest

import assembly_cases as ac
import spline_ref as sr
from spline_ref import ASSEMBLY_TOL, LD

LATTICES = ("S", "A", "B", "C")


@pytest.fixture(scope="module", params=LATTICES)
def case(request):
    return ac.case(request.param)


def oracle_path(case, s, a):
    nn, npts = int(case.ref.n_nodes[s, a]), int(case.ref.n_pts[s, a])
    return case.ref.coeff[s, a, :nn - 1].copy(), case.ref.path_param[s, a, :npts].copy()


def curved_path(case, n_seg=None, min_rows=0):
    """(s, a) of a path whose curvature is well above KAPPA_FLOOR (a straight one has a2 = a3 = kappa = 0: nothing to perturb)."""
    for s, a, nn, npts in case.paths:
        if (n_seg is None or nn - 1 == n_seg) and npts >= min_rows and float(np.max(np.abs(case.ref.path_param[s, a, :npts, 3]))) > 1e-2:
            return s, a
    raise AssertionError("no curved path with N = %s on lattice %s" % (n_seg, case.name))


def test_lattices_take_their_plan_class_and_the_sets_cover_their_classes(case):
    assert ac.plan_class_of(case.lat) == ac.PLAN_CLASS[case.name]
    assert case.lat.num_edges <= 10000 and len(case.scen) <= 140
    ac.assert_coverage(case.name, case.lat, case.scen, case.ref)


def test_oracle_stays_within_the_bound_of_the_long_double_reference(case):
    worst = {}
    for s, a, nn, npts in case.paths:
        ref = case.assembly[(s, a)]
        assert np.array_equal(ref.node_idx, case.ref.node_idx[s, a, :nn]) and ref.n_pts == npts, (s, a)
        sr.merge_worst(worst, sr.assembly_deviation(*oracle_path(case, s, a), ref))
    msg = "lattice %s, oracle against the long-double reference, worst deviation: %s" % (
        case.name, ", ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    print(msg)
    assert all(v <= ASSEMBLY_TOL for v in worst.values()), msg
    for s, a, nn, npts in case.paths:                      # ... and through the checker itself (element-length column included)
        sr.assert_assembly_close(oracle_path(case, s, a), case.assembly[(s, a)], ASSEMBLY_TOL, "%s s%d a%d" % (case.name, s, a))


def test_reference_agrees_with_scipys_clamped_cubic_spline(case):
    """An independent statement of the same spline: scipy.interpolate.CubicSpline over the cumulated segment parameter with first-derivative
    end conditions, its polynomial pieces rescaled to t in [0, 1] and evaluated on the reference's rows."""
    from scipy.interpolate import CubicSpline
    s, a = curved_path(case, min_rows=30)
    nn = int(case.ref.n_nodes[s, a])
    lat, sl, nodes, psi_s = case.lat, case.scen[s]["start_node"][0], case.ref.nodes[s, a, :nn], case.scen[s]["psi_s"]
    ref = case.assembly[(s, a)]
    edges = sr.path_edges(lat, sl, nodes)
    h = lat.edge_len[edges]
    u = np.concatenate(([0.0], np.cumsum(h)))
    knots = np.vstack([lat.samples[lat.samp_ptr[e], 0:2] for e in edges] + [lat.samples[lat.samp_ptr[edges[-1] + 1] - 1, 0:2]])
    psi0 = lat.samples[lat.samp_ptr[edges[0]], 2] if psi_s is None else psi_s
    psiN = lat.samples[lat.samp_ptr[edges[-1] + 1] - 1, 2]
    tan = lambda p: np.array([np.cos(p + np.pi / 2), np.sin(p + np.pi / 2)])
    cs = CubicSpline(u, knots, bc_type=((1, tan(psi0)), (1, tan(psiN))))
    coeff = np.zeros((nn - 1, 8))
    for ax in range(2):
        for k in range(4):
            coeff[:, 4 * ax + k] = cs.c[3 - k, :, ax] * h ** k
    pp = np.zeros((ref.n_pts, 5))
    pp[:, 0:4] = sr.evaluate_rows(coeff.astype(LD), ref.node_idx).astype(np.float64)
    pp[:, 4] = ref.path_param[:, 4]
    sr.assert_assembly_close((coeff, pp), ref, ASSEMBLY_TOL, "scipy, lattice %s s%d a%d" % (case.name, s, a))
    # ... and scipy's own evaluation at the knots' parameters: the rows of the nodes lie on the spline
    assert float(np.max(np.abs(cs(u) - ref.path_param[ref.node_idx, 0:2].astype(np.float64)))) <= 1e-12


def rejected(actual, ref):
    with pytest.raises(AssertionError, match="beyond"):
        sr.assert_assembly_close(actual, ref, ASSEMBLY_TOL, "perturbed")


def test_checker_rejects_small_errors_of_every_quantity():
    """Each of these passes the parity suite's 1e-5; a checker that accepts one of them is the bug."""
    case = ac.case("S")
    s, a = curved_path(case, min_rows=30)
    ref = case.assembly[(s, a)]
    sr.assert_assembly_close(oracle_path(case, s, a), ref)                      # (the unperturbed copy passes)
    coeff, pp = oracle_path(case, s, a)                                          # one segment's a2
    i = int(np.argmax(np.abs(coeff[:, 2])))
    coeff[i, 2] *= 1.0 + 1e-8
    rejected((coeff, pp), ref)
    coeff, pp = oracle_path(case, s, a)                                          # psi of one row
    pp[pp.shape[0] // 2, 2] += 1e-9
    rejected((coeff, pp), ref)
    coeff, pp = oracle_path(case, s, a)                                          # kappa of one row
    r = int(np.argmax(np.abs(pp[:, 3])))
    pp[r, 3] *= 1.0 + 1e-8
    rejected((coeff, pp), ref)
    coeff, pp = oracle_path(case, s, a)                                          # one segment sampled at t = k / n_i
    i = coeff.shape[0] // 2
    wrong = sr.evaluate_rows(coeff.astype(LD), ref.node_idx, t_of=lambda k, n_i: LD(k) / LD(n_i)).astype(np.float64)
    r0, r1 = int(ref.node_idx[i]), int(ref.node_idx[i + 1])
    assert r1 - r0 >= 2
    pp[r0:r1, 0:4] = wrong[r0:r1]
    rejected((coeff, pp), ref)
    coeff, pp = oracle_path(case, s, a)                                          # element-length column: a copy, bit for bit
    pp[3, 4] = np.nextafter(pp[3, 4], 1.0)
    with pytest.raises(AssertionError, match="copy"):
        sr.assert_assembly_close((coeff, pp), ref)


def cyclic_reduction_slopes(knots, h, s0, sN, rounds):
    """Inner knot slopes by parallel cyclic reduction of the clamped spline's system (rows 1 .. N-1; rows 0 and N are identity rows),
    ``rounds`` rounds at distances 1, 2, 4, ...; the full solve needs ceil(log2(N - 1)) of them."""
    N = h.shape[0]
    a, b, c, d = np.zeros(N + 1), np.ones(N + 1), np.zeros(N + 1), np.zeros((N + 1, 2))
    for i in range(1, N):
        ai, ci = 1.0 / h[i - 1], 1.0 / h[i]
        b[i] = 2.0 * (ai + ci)
        d[i] = 3.0 * ((knots[i] - knots[i - 1]) * ai * ai + (knots[i + 1] - knots[i]) * ci * ci)
        a[i], c[i] = (0.0 if i == 1 else ai), (0.0 if i == N - 1 else ci)
        if i == 1:
            d[i] -= ai * s0
        if i == N - 1:
            d[i] -= ci * sN
    st = 1
    for _ in range(rounds):
        lo, hi = np.maximum(np.arange(N + 1) - st, 0), np.minimum(np.arange(N + 1) + st, N)
        al, ga = -a / b[lo], -c / b[hi]
        a, b, c, d = al * a[lo], b + al * c[lo] + ga * a[hi], ga * c[hi], d + al[:, None] * d[lo] + ga[:, None] * d[hi]
        st *= 2
    m = d / b[:, None]
    m[0], m[N] = s0, sN
    return m


def test_checker_rejects_a_cyclic_reduction_that_stops_one_round_early_at_four_segments():
    case = ac.case("S")
    s, a = curved_path(case, n_seg=4)
    ref = case.assembly[(s, a)]
    lat, sl, nodes = case.lat, case.scen[s]["start_node"][0], case.ref.nodes[s, a, :5]
    edges = sr.path_edges(lat, sl, nodes)
    h = lat.edge_len[edges]
    knots = np.vstack([lat.samples[lat.samp_ptr[e], 0:2] for e in edges] + [lat.samples[lat.samp_ptr[edges[-1] + 1] - 1, 0:2]])
    # end slopes as the reference has them: a1 = m h on the first segment, the derivative at t = 1 on the last
    s0 = (ref.coeff[0, [1, 5]] / LD(h[0])).astype(np.float64)
    sN = ((ref.coeff[-1, [1, 5]] + 2 * ref.coeff[-1, [2, 6]] + 3 * ref.coeff[-1, [3, 7]]) / LD(h[-1])).astype(np.float64)

    def assembled(rounds):
        coeff = sr.segment_coefficients(knots, h, cyclic_reduction_slopes(knots, h, s0, sN, rounds))
        pp = np.zeros((ref.n_pts, 5))
        pp[:, 0:4] = sr.evaluate_rows(coeff, ref.node_idx).astype(np.float64)
        pp[:, 4] = ref.path_param[:, 4]
        return coeff.astype(np.float64), pp

    sr.assert_assembly_close(assembled(2), ref, ASSEMBLY_TOL, "two rounds at N = 4")        # three unknowns: distances 1 and 2
    coeff, pp = assembled(1)
    rejected((coeff, pp), ref)
    # (the error of the missing round is what the parity suite's bound cannot see at larger N: it shrinks with every further row)
    dev = sr.assembly_deviation(coeff, pp, ref)
    print("one round early at N = 4: %s" % dev)
