"""CPU: the case families of tests/offline_cases.py do what their names say (asserted on the long-double reference of tests/offline_ref.py),
their margins are wide enough for an fp64 evaluation to take every decision as the reference does, the bounds of the kernel's comparison
follow from the fp64 evaluation of the reference function alone, and oracle/offline_edges_ref.py -- the restatement the lattice tests build
on -- agrees with the reference on every case. Prints the margins and the table of deviations (pytest -s)."""
import numpy as np
import pytest

import offline_cases as oc
import offline_ref as oref
from offline_ref import LD


def restatement(call):
    from oracle import offline_edges_ref
    return offline_edges_ref.evaluate(*call.args)


def test_long_double_is_wider_than_fp64():
    assert np.finfo(LD).eps <= 2.0 ** -63


@pytest.mark.parametrize("name", oc.FAMILIES)
def test_every_call_is_small_and_finite(name):
    for c in oc.family(name):
        assert 1 <= c.n_edges <= 400 and len(set(c.labels)) == c.n_edges, c.name
        ref = oc.reference(c)
        for k in ("coeff", "length", "kappa_avg", "kappa_range", "samples"):
            assert np.all(np.isfinite(ref[k])), (c.name, k)


def test_step_family_sits_on_both_sides_of_every_multiple_of_the_step():
    (c,) = oc.step_family()
    ref = oc.reference(c)
    n = {lab: int(v) for lab, v in zip(c.labels, ref["n_samples"])}
    q = {lab: v for lab, v in zip(c.labels, ref["quotient"])}
    for k in range(1, 7):
        for j in range(8):
            below, above = "k=%d dir=%d below" % (k, j), "k=%d dir=%d above" % (k, j)
            assert n[below] == k + 1 and n[above] == k + 2, (k, j)
            assert 0 < k - q[below] <= 1.01e-9 * k and 0 < q[above] - k <= 1.01e-9 * k, (k, j)
    short = [lab for lab in c.labels if lab.startswith("chord=")]
    assert len(short) == 32 and all(n[lab] == 2 for lab in short)            # one element: the shortest valid edge
    assert np.all(ref["valid"] == 1)
    micro = oref.edge_class(ref, oc.STEP) == "micro"
    assert [lab for lab, m in zip(c.labels, micro) if m] == [lab for lab in c.labels if lab.startswith("chord=1e-6")]
    assert np.all(np.abs(ref["len15"][micro] - LD(1e-6)) <= 1e-12)


def test_curved_family_covers_what_it_claims():
    (c,) = oc.curved_family()
    ref = oc.reference(c)
    ns = ref["n_samples"]
    assert ns.min() == 2 and ns.max() >= 14
    assert np.mean(ns[1:] != ns[:-1]) >= 0.75                                  # neighbouring lanes differ in n
    chord = np.hypot(c.end[:, 0] - c.start[:, 0], c.end[:, 1] - c.start[:, 1])
    assert chord.min() >= 0.5 and chord.max() <= 33.0 and chord[:oc.N_RANDOM].min() < 1.0 and chord.max() > 30.0
    assert np.all(ref["valid"] == 1)                                           # limits far away
    theta = np.arctan2(c.end[:, 1] - c.start[:, 1], c.end[:, 0] - c.start[:, 0])[:oc.N_RANDOM]
    assert np.all(np.histogram(theta, bins=8, range=(-np.pi, np.pi))[0] >= 20)  # directions all around
    # where the peaks lie: at the first sample or at the last, about evenly
    at, last = ref["peak_at"], ns - 1
    first_n, last_n, inner_n = int(np.sum(at == 0)), int(np.sum((at == last) & (at != 0))), int(np.sum((at > 0) & (at < last)))
    print("curved: peak at the first sample %d, at the last %d, inside %d of %d edges" % (first_n, last_n, inner_n, ns.size))
    assert first_n >= 100 and last_n >= 100 and first_n + last_n + inner_n == ns.size
    # the wrap: node headings and sample headings on both sides of +-pi, in both directions
    south = np.arange(c.n_edges)[oc.SOUTH]
    node = np.concatenate((c.start[south, 2], c.end[south, 2]))
    assert np.any(node > np.pi - 1e-3) and np.any(node < -np.pi + 1e-3)
    psi = np.concatenate([ref["rows"][e][:, 2] for e in south])
    assert np.all((psi >= -LD(np.pi)) & (psi < LD(np.pi)))
    assert np.any(psi > np.pi - 1e-3) and np.any(psi < -np.pi + 1e-3)
    down = [e for e in south if ref["rows"][e][0, 2] > 2.8 and ref["rows"][e][-1, 2] < -2.8]
    up = [e for e in south if ref["rows"][e][0, 2] < -2.8 and ref["rows"][e][-1, 2] > 2.8]
    assert len(down) >= 20 and len(up) >= 20
    inside = [e for e in south if np.any(np.abs(np.diff(ref["rows"][e][:, 2].astype(float))) > 6.0) and ref["n_samples"][e] >= 4]
    assert len(inside) >= 20                                                    # the jump lies between two samples of the edge


def test_limits_family_puts_every_limit_one_part_in_1e9_from_a_peak():
    calls = oc.limits_family()
    assert [c.name.split(" pivot")[0] for c in calls[:6]] == ["limits vel above", "limits vel below"] + ["limits turn above", "limits turn below"] * 2
    base = oc.reference(oc.curved_call())
    assert [c.name for c in calls[6:]] == ["limits equal vel", "limits equal turn"]
    for c in calls[6:]:                                                          # the limit EQUALS the peak, and both are exactly 0
        for ref in (oc.reference(c), oc.reference(c, np.float64), restatement(c)):
            ns = np.asarray(ref["n_samples"])
            assert list(ns) == [3, 4, 6, 9] and np.all(np.asarray(ref["valid"]) == 1)
            assert all(np.all(ref["samples"][e][:ns[e], 3] == 0) for e in range(4)), c.name
        assert (c.kappa_max_vel.min() == 0.0) != (c.kappa_max_turn == 0.0)
    calls = calls[:6]
    for c in calls:
        ref = oc.reference(c)
        assert c.n_edges >= 200 and np.all(ref["peak"] >= 1e-3)
        at, last = ref["peak_at"], ref["n_samples"] - 1
        assert np.sum(at == 0) >= 100 and np.sum(at == last) >= 100        # a filter that skips the first or the last sample passes half of them
        if " vel " in c.name:
            rel = (c.kappa_max_vel.astype(LD) / ref["peak"] - LD(1)) * (1 if "above" in c.name else -1)
            assert np.all(np.abs(rel - LD(1e-9)) <= 1e-15), c.name          # exactly 1e-9 up to the rounding of the fp64 limit
            assert c.kappa_max_turn == oc.FAR
            assert np.all(ref["valid"] == (1 if "above" in c.name else 0)), c.name
        else:
            p = c.pivot
            rel = (LD(c.kappa_max_turn) / ref["peak"][p] - LD(1)) * (1 if "above" in c.name else -1)
            assert abs(rel - LD(1e-9)) <= 1e-15 and np.all(c.kappa_max_vel == oc.FAR), c.name
            assert ref["peak_at"][p] == (0 if "first" in c.name else last[p])
            others = np.delete(np.arange(c.n_edges), p)
            assert np.min(np.abs(LD(c.kappa_max_turn) / ref["peak"][others] - LD(1))) >= 1e-7      # no other edge near the limit
            want = (ref["peak"] <= LD(c.kappa_max_turn)).astype(np.int64)
            assert np.array_equal(ref["valid"], want) and 50 <= want.sum() <= c.n_edges - 50
            assert ref["valid"][p] == (1 if "above" in c.name else 0)
    assert base["peak"].min() < 1e-3                                             # (the cut at 1e-3 1/m leaves edges out of THIS family only)


def test_raceline_family_has_given_cubics_beyond_both_limits():
    (c,) = oc.raceline_family()
    ref = oc.reference(c)
    rl = c.raceline_edge.astype(bool)
    assert rl.sum() == (~rl).sum() == 10 and np.array_equal(rl[0::2], np.ones(10, bool))
    assert np.array_equal(ref["coeff"][rl].astype(np.float64), c.given[rl])      # passed through
    assert np.all(ref["valid"][rl] == 1)
    over = rl & (ref["peak"] > max(oc.KAPPA_TURN, oc.KAPPA_VEL) * 1.01)
    assert over.sum() >= 1                                                      # valid DESPITE the filter
    # the poses of the race-line edges have nothing to do with the samples: those start on the polygon
    for i, e in enumerate(np.flatnonzero(rl)):
        assert np.array_equal(ref["rows"][e][0, 0:2].astype(np.float64), oc.POLYGON[i])
        assert np.hypot(*(c.start[e, 0:2] - oc.POLYGON[i])) > 10.0
    # the ordinary edge along a corner segment is refused, with a margin far above 1e-9; elsewhere it passes
    ordinary_over = np.roll(over, 1) & ~rl
    assert ordinary_over.sum() >= 1 and np.all(ref["valid"][ordinary_over] == 0)
    assert np.all(ref["peak"][ordinary_over] > max(oc.KAPPA_TURN, oc.KAPPA_VEL) * 1.01)
    assert np.sum(ref["valid"][~rl] == 1) >= 4
    margin = np.abs(ref["peak"][~rl] / LD(oc.KAPPA_VEL) - 1)
    assert margin.min() >= 1e-3


def test_capacity_family_refuses_exactly_the_largest_edges():
    fits, tight, wide = oc.capacity_family()
    rf, rt, rw = oc.reference(fits), oc.reference(tight), oc.reference(wide)
    nmax = int(rf["n_samples"].max())
    assert (fits.cap, tight.cap, wide.cap) == (nmax, nmax - 1, nmax + 37) and tight.cap >= 2
    assert np.array_equal(rf["n_samples"], rt["n_samples"]) and np.array_equal(rf["n_samples"], rw["n_samples"])
    assert all(r is not None for r in rf["rows"]) and all(r is not None for r in rw["rows"])
    big = rf["n_samples"] == nmax
    assert 1 <= big.sum() <= 10 and np.sum(rf["n_samples"] == nmax - 1) >= 1     # the next smaller edge fills the tight staging to its last row
    assert [r is None for r in rt["rows"]] == list(big)
    for k in ("valid", "length", "kappa_avg", "kappa_range"):
        assert np.all(rt[k][big] == 0) and np.array_equal(rt[k][~big], rf[k][~big]) and np.array_equal(rw[k], rf[k]), k
    assert np.all(rf["valid"][big] == 1)


def test_degenerate_family_has_one_edge_of_a_single_sample():
    (c,) = oc.degenerate_family()
    ref = oc.reference(c)
    assert list(ref["n_samples"][[1]]) == [1] and ref["len15"][1] == 0 and ref["rows"][1] is None
    assert ref["valid"][1] == 0 and ref["length"][1] == 0 and ref["kappa_avg"][1] == 0 and ref["kappa_range"][1] == 0
    assert np.all(ref["coeff"][1, [1, 2, 3, 5, 6, 7]] == 0)
    assert np.all(ref["n_samples"][[0, 2]] >= 3) and np.all(ref["valid"][[0, 2]] == 1)


def test_shapes_family_ends_its_last_block_partial_full_and_absent():
    calls = oc.shapes_family()
    assert [c.n_edges for c in calls] == [1, 63, 64, 65, 129]
    assert sorted(c.n_edges % 64 for c in calls) == [0, 1, 1, 1, 63]
    base = oc.curved_call()
    assert all(np.array_equal(c.start, base.start[250:250 + c.n_edges]) for c in calls)
    kinds = {lab.split()[0] for lab in calls[-1].labels}
    assert kinds == {"random", "south"}


# ---- margins: conditions on the cases, not measurements of any code under test ---------------------------------------------------------------

def test_margins_let_an_fp64_evaluation_take_every_decision():
    """No case of any family is excluded from any comparison, so EVERY edge must be decidable in fp64: len15 / step at least 1e-10 from an
    integer, and the fp64 evaluation of the reference function and the restatement each reproduce every n and every valid."""
    smallest, n_zero = 1.0, 0
    for c in oc.all_calls():
        ref = oc.reference(c)
        q = ref["quotient"]
        margin = np.abs(q - np.rint(q))
        # the one edge that is exempt, explicitly: start = end, so len15 and the quotient are exactly 0 and n is 1 in EVERY number type
        # (asserted below for the fp64 evaluations and the restatement like every other n); it is still compared in every comparison
        zero = ref["len15"] == 0
        assert int(zero.sum()) == (1 if c.name == "degenerate" else 0) and np.all(ref["n_samples"][zero] == 1), c.name
        n_zero += int(zero.sum())
        margin = margin[~zero]
        assert margin.min() >= 1e-10, c.name
        smallest = min(smallest, float(margin.min()))
        for title, other in (("fp64 evaluation", oc.reference(c, np.float64)), ("fp64 evaluation, absolute form", oc.reference(c, np.float64, "absolute")),
                             ("restatement", restatement(c))):
            assert np.array_equal(np.asarray(other["n_samples"], np.int64), ref["n_samples"]), (c.name, title)
            assert np.array_equal(np.asarray(other["valid"], np.int64), ref["valid"]), (c.name, title)
    print("smallest |len15 / step - integer| over %d calls: %.2e" % (len(oc.all_calls()), smallest))
    assert smallest <= 1.01e-9                                                   # ... and the step family really sits that close
    assert n_zero == 1


def test_bounds_follow_from_the_fp64_evaluation_and_the_restatement_keeps_its_own():
    fp64 = oc.worst_of(lambda c: oc.reference(c, np.float64))
    absolute = oc.worst_of(lambda c: oc.reference(c, np.float64, "absolute"))
    rest = oc.worst_of(restatement)
    bounds, rbounds = oc.bounds(), oc.restatement_bounds()
    print(oc.format_table([("fp64 evaluation of the reference function", fp64), ("  bound of the kernel (100 x, rounded up)", bounds),
                           ("fp64 evaluation, absolute-coordinate form", absolute), ("  bound of the restatement", rbounds),
                           ("oracle/offline_edges_ref.evaluate", rest)]))
    for cls in ("regular", "micro"):
        for k in oref.QUANTITIES:
            b = bounds[cls][k]
            assert b >= oref.BOUND_FLOOR and b >= 100.0 * fp64[cls][k] and (b == oref.BOUND_FLOOR or b <= 200.0 * fp64[cls][k] * (1 + 1e-9)), (cls, k)
            assert float("%.0e" % b) == b or b == oref.BOUND_FLOOR, (cls, k)     # one digit
            assert rest[cls][k] <= rbounds[cls][k], "restatement, %s edges, %s: %.3e beyond %.1e" % (cls, k, rest[cls][k], rbounds[cls][k])
        # the bounds are sharp: nine orders below the 1e-5 contract on regular edges where the issue's table expects it
    assert bounds["regular"]["psi"] <= 1e-12 and bounds["regular"]["coeff"] <= 1e-12 and bounds["regular"]["kappa"] <= 1e-8
    for c in oc.all_calls():                                                    # ... and through the checker itself
        oref.check_call(oc.reference(c, np.float64), oc.reference(c), bounds, oc.STEP, "fp64 evaluation / " + c.name, c.labels)
        oref.check_call(restatement(c), oc.reference(c), rbounds, oc.STEP, "restatement / " + c.name, c.labels)


def test_rounding_up_to_one_digit():
    assert oref.round_up_one_digit(2.4e-10) == 3e-10 and oref.round_up_one_digit(3e-10) == 3e-10
    assert oref.round_up_one_digit(9.01e-13) == 1e-12 and oref.round_up_one_digit(1.0e-7) == 1e-7 and oref.round_up_one_digit(0.0) == 0.0


def test_checker_rejects_what_the_1e5_contract_lets_through():
    """Each of these passes a 1e-5 comparison; a checker that accepts one of them is the bug."""
    (c,) = oc.curved_family()
    ref, bounds = oc.reference(c), oc.bounds()

    def fresh():
        src = oc.reference(c, np.float64)
        return {k: np.array(src[k], dtype=(np.int64 if k in ("n_samples", "valid") else np.float64)) for k in
                ("n_samples", "valid", "coeff", "length", "kappa_avg", "kappa_range", "samples")}
    oref.check_call(fresh(), ref, bounds, oc.STEP, "unperturbed")
    e = int(np.argmax(ref["n_samples"]))
    n = int(ref["n_samples"][e])
    for what, edit in (("psi", lambda g: g["samples"].__setitem__((e, n // 2, 2), g["samples"][e, n // 2, 2] + 1e-9)),
                       ("kappa", lambda g: g["samples"].__setitem__((e, 0, 3), g["samples"][e, 0, 3] * (1 + 1e-7))),
                       ("el", lambda g: g["samples"].__setitem__((e, 1, 4), g["samples"][e, 1, 4] * (1 + 1e-8))),
                       ("xy", lambda g: g["samples"].__setitem__((e, n - 1, 0), g["samples"][e, n - 1, 0] + 1e-7)),
                       ("coeff", lambda g: g["coeff"].__setitem__((e, 6), g["coeff"][e, 6] * (1 + 1e-8))),
                       ("length", lambda g: g["length"].__setitem__(e, g["length"][e] * (1 + 1e-8))),
                       ("kappa_avg", lambda g: g["kappa_avg"].__setitem__(e, g["kappa_avg"][e] * n / (n - 1.0))),
                       ("kappa_range", lambda g: g["kappa_range"].__setitem__(e, g["kappa_range"][e] * (1 + 1e-7)))):
        g = fresh()
        edit(g)
        with pytest.raises(AssertionError, match=what + " off by"):
            oref.check_call(g, ref, bounds, oc.STEP, "perturbed " + what)
    g = fresh()
    g["samples"][e, n - 1, 4] = 1e-300
    with pytest.raises(AssertionError, match="last row"):
        oref.check_call(g, ref, bounds, oc.STEP, "last row")
    g = fresh()
    g["n_samples"][e] += 1
    with pytest.raises(AssertionError, match="n_samples"):
        oref.check_call(g, ref, bounds, oc.STEP, "n")
    g = fresh()
    g["valid"][e] = 0
    with pytest.raises(AssertionError, match="valid"):
        oref.check_call(g, ref, bounds, oc.STEP, "valid")
