"""Reference of the per-edge operation of the offline build (`k_offline_edges` / `ltpl_offline_edges`, include/ltpl_hip.h) and the comparison
against it. NumPy only, written from the inputs of `ltpl_offline_edges_in` alone, with the number type as a parameter: np.longdouble by
default (THE reference), np.float64 on request (what an fp64 evaluation of the same formulas can reach: the source of the bounds).

  cubic      ordinary edge, per axis, d = end - start, chord = |d|, slopes T0 = cos / sin(psi_start + pi/2) chord, T1 likewise at the end:
               a0 = start, a1 = T0, a2 = 3 d - 2 T0 - T1, a3 = -2 d + T0 + T1             (difference form: no absolute coordinate but a0)
             race-line edge (raceline_edge != 0): the GIVEN coefficients, untouched; the poses are not read
  len15      length of the polyline through t = 0, 1/14 .. 1
  n          ceil(len15 / step) + 1 samples at t_i = i / (n - 1); the last point is a0 + a1 + a2 + a3
  psi        atan2(y', x') - pi/2 wrapped into [-pi, pi);  kappa = (x' y'' - y' x'') / |r'|^3
  el         distance from sample i to sample i + 1, 0 in the last row;  length = sum of el
  kappa_avg  sum |kappa| / n;  kappa_range = |max kappa - min kappa|
  valid      1 if |kappa| <= kappa_max_turn and <= kappa_max_vel[e] at EVERY sample, or if the edge is a race-line edge
  n > cap_samples or n < 2: n is reported, valid = 0, length = kappa_avg = kappa_range = 0, no sample rows
pi is the fp64 constant of the product in every number type (the inputs are fp64 headings measured against that constant).
`form="absolute"` computes a2 and a3 of ordinary edges from the absolute coordinates (-3 x0 + 3 x1 - 2 T0 - T1, 2 x0 - 2 x1 + T0 + T1: the rows
of the inverse of the reference's 4 x 4 system) -- the formulation of oracle/offline_edges_ref.py, which loses an ulp of the COORDINATE
where the difference form loses an ulp of the chord.

THE BOUNDS (`derive_bounds`). Per quantity 100 x the worst deviation of the fp64 evaluation of THIS function from its long-double
evaluation over all cases of tests/offline_cases.py, rounded up to one digit, never below 100 eps(fp64). The factor 100 is the convention
of DESIGN.md section 2: two orders for another library's sin / cos / atan2 / sqrt and another summation order. Nothing the kernel computes
enters. Scales, on the reference:  x, y, a0 against the edge's largest |coordinate| (at least 1 m);  a1 .. a3 against the edge's extent
(len15);  psi in radians modulo 2 pi;  kappa, kappa_avg, kappa_range against max(peak, 1e-4 1/m), peak = max |kappa| of the edge;
element lengths against the longest of the edge;  length relative.
Two classes of edges, each with bounds derived over its own members, every edge compared in the class it belongs to:
  regular   len15 >= step / 10
  micro     shorter (the 1e-6 m chords of the step family). An fp64 evaluation cannot know a 1e-6 m element between samples at +-500 m
            better than ulp(500 m) / 1e-6 m = 6e-8, nor the curvature of such an edge better than eps / 1e-6 m = 2e-10 1/m, which is 2e-6 of
            the curvature floor. One bound over both classes would be the micro edges' bound (1e-5 .. 1e-4) for every edge of the suite; the
            split keeps the regular edges at what THEY allow (1e-10 and below). Either class's bound is at most the bound over all edges.
"""
import math

import numpy as np

LD = np.longdouble
KAPPA_FLOOR = 1e-4
QUANTITIES = ("xy", "coeff", "psi", "kappa", "el", "length", "kappa_avg", "kappa_range")
MARGIN = 100.0
BOUND_FLOOR = MARGIN * float(np.finfo(np.float64).eps)


def _poly(c, t):
    return c[0] + c[1] * t + c[2] * (t * t) + c[3] * (t * t * t)


def edge_coefficients(start, end, T, form="difference"):
    """(cx, cy) of the two-point cubic from pose ``start`` to pose ``end`` (x, y, psi each) in number type ``T``."""
    half_pi = T(math.pi) / T(2)
    d = [T(end[0]) - T(start[0]), T(end[1]) - T(start[1])]
    chord = np.sqrt(d[0] * d[0] + d[1] * d[1])
    out = []
    for ax, fn in ((0, np.cos), (1, np.sin)):
        p0, p1 = T(start[ax]), T(end[ax])
        t0, t1 = fn(T(start[2]) + half_pi) * chord, fn(T(end[2]) + half_pi) * chord
        if form == "difference":
            a2, a3 = T(3) * d[ax] - T(2) * t0 - t1, -T(2) * d[ax] + t0 + t1
        elif form == "absolute":
            a2, a3 = -T(3) * p0 + T(3) * p1 - T(2) * t0 - t1, T(2) * p0 - T(2) * p1 + t0 + t1
        else:
            raise ValueError(form)
        out.append(np.array([p0, t0, a2, a3], dtype=T))
    return out[0], out[1]


def evaluate(start, end, kappa_max_vel, raceline_edge, given_coeff, stepsize, kappa_max_turn, cap, dtype=LD, form="difference"):
    """The call of ``offline_build.edges_on_device(...)`` in number type ``dtype``. Besides the outputs of the ABI (samples zero where the
    ABI leaves them unspecified): ``rows`` (list of (n, 5) arrays, None where there are none), ``len15``, ``quotient`` = len15 / step,
    ``peak`` = max |kappa| over the samples and ``peak_at`` = its sample index (0 / -1 where there are no rows)."""
    T = dtype
    start, end = np.asarray(start, np.float64), np.asarray(end, np.float64)
    kmv, rl, given = np.asarray(kappa_max_vel, np.float64), np.asarray(raceline_edge), np.asarray(given_coeff, np.float64)
    n_edges, cap = start.shape[0], int(cap)
    pi, step, kturn = T(math.pi), T(stepsize), T(kappa_max_turn)
    out = {"n_samples": np.zeros(n_edges, np.int64), "valid": np.zeros(n_edges, np.int64), "coeff": np.zeros((n_edges, 8), T),
           "length": np.zeros(n_edges, T), "kappa_avg": np.zeros(n_edges, T), "kappa_range": np.zeros(n_edges, T),
           "samples": np.zeros((n_edges, cap, 5), T), "rows": [None] * n_edges, "len15": np.zeros(n_edges, T),
           "quotient": np.zeros(n_edges, T), "peak": np.zeros(n_edges, T), "peak_at": np.full(n_edges, -1, np.int64)}
    for e in range(n_edges):
        if rl[e]:
            cx, cy = given[e, 0:4].astype(T), given[e, 4:8].astype(T)
        else:
            cx, cy = edge_coefficients(start[e], end[e], T, form)
        out["coeff"][e, 0:4], out["coeff"][e, 4:8] = cx, cy
        t15 = np.arange(15).astype(T) / T(14)
        px, py = _poly(cx, t15), _poly(cy, t15)
        len15 = np.sum(np.sqrt(np.diff(px) ** 2 + np.diff(py) ** 2))
        n = int(np.ceil(len15 / step)) + 1
        out["len15"][e], out["quotient"][e], out["n_samples"][e] = len15, len15 / step, n
        if n < 2 or n > cap:
            continue
        t = np.arange(n).astype(T) / T(n - 1)
        x, y = _poly(cx, t), _poly(cy, t)
        x[-1], y[-1] = ((cx[0] + cx[1]) + cx[2]) + cx[3], ((cy[0] + cy[1]) + cy[2]) + cy[3]
        xd, yd = cx[1] + T(2) * cx[2] * t + T(3) * cx[3] * (t * t), cy[1] + T(2) * cy[2] * t + T(3) * cy[3] * (t * t)
        xdd, ydd = T(2) * cx[2] + T(6) * cx[3] * t, T(2) * cy[2] + T(6) * cy[3] * t
        psi = np.arctan2(yd, xd) - pi / T(2)
        psi = np.where(psi < -pi, psi + T(2) * pi, psi)            # atan2 - pi/2 lies in [-3 pi/2, pi/2]
        psi = np.where(psi >= pi, psi - T(2) * pi, psi)
        q = xd * xd + yd * yd
        kappa = (xd * ydd - yd * xdd) / (q * np.sqrt(q))
        el = np.zeros(n, T)
        el[:-1] = np.sqrt(np.diff(x) ** 2 + np.diff(y) ** 2)
        ka = np.abs(kappa)
        ok = bool(np.all(ka <= kturn) and np.all(ka <= T(kmv[e])))
        rows = np.stack((x, y, psi, kappa, el), axis=1)
        out["rows"][e] = rows
        out["samples"][e, :n] = rows
        out["valid"][e] = 1 if (ok or rl[e]) else 0
        out["length"][e] = np.sum(el)
        out["kappa_avg"][e] = np.sum(ka) / T(n)
        out["kappa_range"][e] = np.abs(np.max(kappa) - np.min(kappa))
        out["peak_at"][e] = int(np.argmax(ka))
        out["peak"][e] = ka[out["peak_at"][e]]
    return out


def edge_class(ref, stepsize):
    """"micro" / "regular" per edge (see the module's docstring), decided on the reference's len15."""
    return np.where(ref["len15"] < LD(stepsize) / LD(10), "micro", "regular")


def deviations(got, ref):
    """{quantity: per-edge array} of the deviation of ``got`` (outputs in the layout of ``edges_on_device``; any float type) from ``ref`` (a
    long-double `evaluate` of the same call), each against its scale, over rows [0, n) of an edge only. The coefficients of every edge are
    compared; the other quantities are 0 for an edge without rows."""
    n_edges = ref["n_samples"].shape[0]
    pi = LD(math.pi)
    dev = {k: np.zeros(n_edges) for k in QUANTITIES}
    coeff = np.asarray(got["coeff"], LD)
    for e in range(n_edges):
        rc = ref["coeff"][e]
        rows = ref["rows"][e]
        cmax = max(np.max(np.abs(rc[[0, 4]])), LD(1)) if rows is None else max(np.max(np.abs(rows[:, 0:2])), LD(1))
        extent = ref["len15"][e] if ref["len15"][e] > 0 else LD(1)
        dev["coeff"][e] = float(max(np.max(np.abs(coeff[e, [0, 4]] - rc[[0, 4]])) / cmax,
                                    np.max(np.abs(coeff[e, [1, 2, 3, 5, 6, 7]] - rc[[1, 2, 3, 5, 6, 7]])) / extent))
        if rows is None:
            continue
        n = rows.shape[0]
        g = np.asarray(got["samples"][e][:n], LD)
        kscale = max(ref["peak"][e], LD(KAPPA_FLOOR))
        dev["xy"][e] = float(np.max(np.abs(g[:, 0:2] - rows[:, 0:2])) / cmax)
        dev["psi"][e] = float(np.max(np.abs(np.mod(g[:, 2] - rows[:, 2] + pi, LD(2) * pi) - pi)))
        dev["kappa"][e] = float(np.max(np.abs(g[:, 3] - rows[:, 3])) / kscale)
        dev["el"][e] = float(np.max(np.abs(g[:-1, 4] - rows[:-1, 4])) / np.max(rows[:, 4]))
        dev["length"][e] = float(np.abs(LD(got["length"][e]) - ref["length"][e]) / ref["length"][e])
        dev["kappa_avg"][e] = float(np.abs(LD(got["kappa_avg"][e]) - ref["kappa_avg"][e]) / kscale)
        dev["kappa_range"][e] = float(np.abs(LD(got["kappa_range"][e]) - ref["kappa_range"][e]) / kscale)
    return dev


def merge_worst(worst, dev, classes):
    """Fold one call's per-edge deviations into ``worst`` = {class: {quantity: (value, label)}}; returns ``worst``."""
    for cls in ("regular", "micro"):
        sel = np.flatnonzero(classes == cls)
        if sel.size == 0:
            continue
        w = worst.setdefault(cls, {})
        for k in QUANTITIES:
            w[k] = max(w.get(k, 0.0), float(np.max(dev[k][sel])))
    return worst


def round_up_one_digit(v):
    """The smallest m x 10^k >= v with m in 1 .. 9."""
    if not v > 0.0:
        return 0.0
    k = math.floor(math.log10(v))
    m = math.ceil(v / 10.0 ** k * (1.0 - 1e-12))
    return float("%de%d" % (m, k)) if m < 10 else float("1e%d" % (k + 1))


def derive_bounds(worst):
    """{class: {quantity: bound}} from the worst deviations of an fp64 evaluation (`merge_worst`)."""
    return {cls: {k: max(round_up_one_digit(MARGIN * v), BOUND_FLOOR) for k, v in w.items()} for cls, w in worst.items()}


def check_call(got, ref, bounds, stepsize, what, labels=None):
    """``got`` against the long-double ``ref`` of the same call: n_samples and valid EXACT, every float within ``bounds`` over rows [0, n), the
    element length of the last row 0, and 0 in the three scalars of an edge without rows. Returns the deviations (`deviations`)."""
    lab = (lambda e: "%s / edge %d" % (what, e)) if labels is None else (lambda e: "%s / edge %d (%s)" % (what, e, labels[e]))
    ns, va = np.asarray(got["n_samples"], np.int64), np.asarray(got["valid"], np.int64)
    bad = np.flatnonzero(ns != ref["n_samples"])
    assert bad.size == 0, "%s: n_samples %d, reference %d (len15 / step = %.12f); %d edges differ" % (
        lab(bad[0]), ns[bad[0]], ref["n_samples"][bad[0]], float(ref["quotient"][bad[0]]), bad.size)
    bad = np.flatnonzero(va != ref["valid"])
    assert bad.size == 0, "%s: valid %d, reference %d (peak %.12e at sample %d of %d); %d edges differ" % (
        lab(bad[0]), va[bad[0]], ref["valid"][bad[0]], float(ref["peak"][bad[0]]), ref["peak_at"][bad[0]], ref["n_samples"][bad[0]], bad.size)
    for e in range(ns.shape[0]):
        if ref["rows"][e] is None:
            assert va[e] == 0 and got["length"][e] == 0.0 and got["kappa_avg"][e] == 0.0 and got["kappa_range"][e] == 0.0, \
                "%s: an edge without rows reports valid = 0 and 0 in length, kappa_avg, kappa_range" % lab(e)
        else:
            assert got["samples"][e][ns[e] - 1][4] == 0.0, "%s: the element length of the last row is 0" % lab(e)
    dev = deviations(got, ref)
    classes = edge_class(ref, stepsize)
    for cls in ("regular", "micro"):
        sel = np.flatnonzero(classes == cls)
        for k in QUANTITIES:
            if sel.size:
                e = sel[int(np.argmax(dev[k][sel]))]
                assert dev[k][e] <= bounds[cls][k], "%s: %s off by %.3e of its scale, bound %.1e (%s edges)" % (lab(e), k, dev[k][e], bounds[cls][k], cls)
    return dev
