"""Named case families for `ltpl_offline_edges` at its decision boundaries (no test functions): tests/test_offline_cases_host.py asserts
on the long-double reference of tests/offline_ref.py that every family does what its name says and derives the bounds from them,
tests/test_gpu_offline_edges.py runs them through the kernel. Every family is a list of `Call`s (one launch each) of at most a few hundred
edges at stepsize_approx = 2.5; coordinates have the magnitude of real tracks (+-500 m), so the cancellation between position and element
length is part of what is compared. Every edge carries a label that a failure prints.

  step       straight edges, headings along the chord, chord = k step (1 -+ 1e-9), k = 1 .. 6, eight compass directions: n = k + 1 / k + 2;
             chords below one step (n = 2: one element); chords of 1e-6 m
  curved     seeded Hermite edges: chords 0.5 .. 32 m, lateral shift up to a quarter of the chord, end headings up to +-0.3 rad off the chord,
             directions uniform; a subset that runs south, whose node and sample headings straddle +-pi in both directions. (The
             curvature of such a cubic peaks at its first or its last sample: 3 000 seeded edges of these ranges hold no interior peak.)
  limits     the curved edges with peak >= 1e-3 1/m: kappa_max_vel[e] = peak_e (1 + 1e-9) (all valid) and peak_e (1 - 1e-9) (none valid) with
             kappa_max_turn far away; one global kappa_max_turn = peak_m (1 +- 1e-9) of a pivot edge m with kappa_max_vel far away (the edges
             below the pivot valid, those above not, the pivot itself flips), once with a pivot whose peak is its first sample, once its last;
             straight edges due east between integer coordinates, whose curvature is exactly 0, at a limit of exactly 0 (`<=`, not `<`)
  raceline   raceline_edge = 1 with the coefficients of the closed spline through a small polygon with one tight corner, poses unrelated to
             them: coefficients passed through, samples of the GIVEN cubic, valid despite the filter; between them ordinary edges along
             the same segments, invalid at the corner
  capacity   one set of edges at cap_samples = largest n (fits exactly), one smaller (the largest edges are refused), well above (stride)
  degenerate an edge whose start and end coincide between two ordinary ones
  shapes     the curved family cut to 1, 63, 64, 65, 129 edges: the last block partial, full and absent
"""
import functools
import math

import numpy as np

import offline_ref as oref
from graphbasedlocaltrajectoryplanner_amd import offline_build as ob

STEP = 2.5
FAR = 1.0e3                      # a curvature limit no edge of any family comes near [1/m]
KAPPA_TURN, KAPPA_VEL = 1.0 / 7.0, 0.1          # the limits of the race-line family (veh_turn = 7 m as in OFFLINE_DEFAULTS)
REL = 1e-9                       # relative distance of chords from a multiple of the step and of limits from a peak
FAMILIES = ("step", "curved", "limits", "raceline", "capacity", "degenerate", "shapes")


class Call(object):
    """One launch: the arguments of ``edges_on_device(...)`` / ``offline_ref.evaluate`` and a label per edge."""

    def __init__(self, name, start, end, labels, kappa_max_vel=None, kappa_max_turn=FAR, raceline_edge=None, given=None, cap=None):
        n = len(labels)
        self.name, self.labels = name, list(labels)
        self.start, self.end = np.ascontiguousarray(start, np.float64).reshape(n, 3), np.ascontiguousarray(end, np.float64).reshape(n, 3)
        self.kappa_max_vel = np.full(n, FAR) if kappa_max_vel is None else np.ascontiguousarray(kappa_max_vel, np.float64)
        self.kappa_max_turn = float(kappa_max_turn)
        self.raceline_edge = np.zeros(n, np.int32) if raceline_edge is None else np.ascontiguousarray(raceline_edge, np.int32)
        self.given = np.zeros((n, 8)) if given is None else np.ascontiguousarray(given, np.float64)
        self.cap = cap
        assert np.all(np.isfinite(self.start)) and np.all(np.isfinite(self.end)) and np.all(np.isfinite(self.given))
        assert float(max(np.max(np.abs(self.start[:, 0:2])), np.max(np.abs(self.end[:, 0:2])))) <= 600.0
        if cap is None:                                                         # room for every edge: three rows above the largest n
            self.cap = int(np.max(oref.evaluate(*self._args(0), dtype=np.float64)["n_samples"])) + 3      # (cap 0: n alone, no rows)

    def _args(self, cap):
        return (self.start, self.end, self.kappa_max_vel, self.raceline_edge, self.given, STEP, self.kappa_max_turn, cap)

    @property
    def args(self):
        return self._args(self.cap)

    @property
    def n_edges(self):
        return len(self.labels)

    def cut(self, name, sel, **kw):
        """The edges ``sel`` of this call as a call of their own."""
        sel = np.arange(self.n_edges)[sel]
        args = dict(kappa_max_vel=self.kappa_max_vel[sel], kappa_max_turn=self.kappa_max_turn, raceline_edge=self.raceline_edge[sel],
                    given=self.given[sel])
        args.update(kw)
        return Call(name, self.start[sel], self.end[sel], [self.labels[i] for i in sel], **args)


def wrap(psi):
    """Into [-pi, pi), as node headings are."""
    return (psi + math.pi) % (2.0 * math.pi) - math.pi


def straight(p, theta, chord):
    """(start, end) of a straight edge from ``p`` in the direction ``theta`` (mathematical angle): both headings along the chord."""
    psi = wrap(theta - math.pi / 2)
    return (p[0], p[1], psi), (p[0] + chord * math.cos(theta), p[1] + chord * math.sin(theta), psi)


def _site(i):
    """Deterministic positions spread over a +-500 m track."""
    return (-480.0 + 37.3 * (i % 26) + 0.011 * i, 470.0 - 41.9 * ((i * 7) % 23) - 0.007 * i)


@functools.lru_cache(maxsize=None)
def step_family():
    start, end, labels = [], [], []

    def add(theta, chord, label):
        s, e = straight(_site(len(labels)), theta, chord)
        start.append(s), end.append(e), labels.append(label)
    for k in range(1, 7):
        for j in range(8):
            for sign in (-1, 1):
                add(j * math.pi / 4, k * STEP * (1.0 + sign * REL), "k=%d dir=%d %s" % (k, j, "below" if sign < 0 else "above"))
    for chord in (0.3, 1.0, 2.4):
        for j in range(8):
            add(j * math.pi / 4 + 0.1, chord, "chord=%.1f dir=%d" % (chord, j))
    for j in range(8):
        add(j * math.pi / 4 + 0.2, 1e-6, "chord=1e-6 dir=%d" % j)
    return (Call("step", start, end, labels),)


def hermite(p, theta, chord, lateral, off0, off1):
    """(start, end): the end lies ``chord`` along ``theta`` and ``lateral`` to its left; headings ``off0`` / ``off1`` off the actual chord."""
    ex, ey = p[0] + chord * math.cos(theta) - lateral * math.sin(theta), p[1] + chord * math.sin(theta) + lateral * math.cos(theta)
    along = math.atan2(ey - p[1], ex - p[0]) - math.pi / 2
    return (p[0], p[1], wrap(along + off0)), (ex, ey, wrap(along + off1))


N_RANDOM, N_SOUTH = 320, 64


@functools.lru_cache(maxsize=None)
def curved_call():
    rng = np.random.default_rng(20240611)
    start, end, labels = [], [], []
    for i in range(N_RANDOM):
        chord = rng.uniform(0.5, 32.0)
        s, e = hermite(rng.uniform(-500.0, 500.0, 2), rng.uniform(-math.pi, math.pi), chord, rng.uniform(-0.25, 0.25) * chord,
                       rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3))
        start.append(s), end.append(e), labels.append("random %d" % i)
    for i in range(N_SOUTH):                                 # running south (psi = +-pi): the heading crosses the wrap inside the edge
        d = (1 if i % 2 else -1) * (5e-4 if i < 8 else rng.uniform(0.01, 0.25))
        p = rng.uniform(-480.0, 480.0, 2)
        chord, theta = rng.uniform(2.0, 32.0), -math.pi / 2 + rng.uniform(-1e-4, 1e-4)
        s = (p[0], p[1], wrap(math.pi - d))                  # d > 0: from just below +pi to just above -pi, d < 0: the other way round
        e = (p[0] + chord * math.cos(theta), p[1] + chord * math.sin(theta), wrap(-math.pi + d))
        start.append(s), end.append(e), labels.append("south %d %s" % (i, "+pi -> -pi" if d > 0 else "-pi -> +pi"))
    return Call("curved", start, end, labels)


def curved_family():
    return (curved_call(),)


SOUTH = slice(N_RANDOM, N_RANDOM + N_SOUTH)


def _limit(peak, sign):
    return float(peak * (oref.LD(1) + sign * oref.LD(REL)))


@functools.lru_cache(maxsize=None)
def limits_family():
    base = curved_call()
    ref = reference(base)
    sel = np.flatnonzero(ref["peak"] >= 1e-3)
    peak, at, last = ref["peak"][sel], ref["peak_at"][sel], ref["n_samples"][sel] - 1
    calls = []
    for sign, tag in ((1, "above"), (-1, "below")):
        calls.append(base.cut("limits vel %s" % tag, sel, kappa_max_vel=[_limit(p, sign) for p in peak], kappa_max_turn=FAR))
    order = np.argsort(peak)
    for where, cond in (("first", at == 0), ("last", at == last)):
        mid = [i for i in order[order.size // 3: 2 * order.size // 3] if cond[i]]
        pivot = mid[len(mid) // 2]
        for sign, tag in ((1, "above"), (-1, "below")):
            c = base.cut("limits turn %s pivot peak at %s sample" % (tag, where), sel, kappa_max_vel=np.full(sel.size, FAR),
                         kappa_max_turn=_limit(peak[pivot], sign))
            c.pivot = int(pivot)
            calls.append(c)
    # a limit EQUAL to the peak needs a peak every evaluation knows exactly: straight edges due east between integer coordinates have
    # cos(psi + pi/2) = 1 and sin = 0 exactly, so a2 = a3 = 0 and kappa = 0 at every sample, in every number type; the limit is 0
    start = [(100.0 * j - 300.0, 40.0 * j - 100.0, -math.pi / 2) for j in range(4)]
    end = [(s[0] + d, s[1], s[2]) for s, d in zip(start, (3.0, 7.0, 11.0, 19.0))]
    labels = ["east %d m" % d for d in (3, 7, 11, 19)]
    calls.append(Call("limits equal vel", start, end, labels, kappa_max_vel=np.zeros(4), kappa_max_turn=FAR))
    calls.append(Call("limits equal turn", start, end, labels, kappa_max_vel=np.full(4, FAR), kappa_max_turn=0.0))
    return tuple(calls)


POLYGON = np.array([[300.0, -200.0], [330.0, -204.0], [356.0, -190.0], [362.0, -186.5], [361.0, -181.0], [340.0, -168.0], [312.0, -160.0],
                    [284.0, -166.0], [270.0, -184.0], [280.0, -196.0]])         # clockwise; the corner at (362, -186.5) turns within ~3 m


@functools.lru_cache(maxsize=None)
def raceline_family():
    coeff = ob._periodic_spline_coeffs(POLYGON)
    n = POLYGON.shape[0]
    rng = np.random.default_rng(7)
    start, end, labels, rl, given = [], [], [], [], []
    for i in range(n):
        cx, cy = coeff[i, 0:4], coeff[i, 4:8]
        # the race-line edge: poses that have nothing to do with its coefficients
        start.append(np.append(rng.uniform(-500.0, 500.0, 2), rng.uniform(-math.pi, math.pi)))
        end.append(np.append(rng.uniform(-500.0, 500.0, 2), rng.uniform(-math.pi, math.pi)))
        labels.append("race line segment %d" % i), rl.append(1), given.append(coeff[i])
        # the ordinary edge along the same segment: the spline's end points and end headings
        psi0 = wrap(math.atan2(cy[1], cx[1]) - math.pi / 2)
        psi1 = wrap(math.atan2(cy[1] + 2 * cy[2] + 3 * cy[3], cx[1] + 2 * cx[2] + 3 * cx[3]) - math.pi / 2)
        nxt = POLYGON[(i + 1) % n]
        start.append((POLYGON[i, 0], POLYGON[i, 1], psi0)), end.append((nxt[0], nxt[1], psi1))
        labels.append("ordinary edge along segment %d" % i), rl.append(0), given.append(np.zeros(8))
    return (Call("raceline", start, end, labels, kappa_max_vel=np.full(2 * n, KAPPA_VEL), kappa_max_turn=KAPPA_TURN, raceline_edge=rl,
                 given=given),)


N_CAPACITY = 96


@functools.lru_cache(maxsize=None)
def capacity_family():
    base = curved_call()
    nmax = int(np.max(reference(base)["n_samples"][:N_CAPACITY]))
    return tuple(base.cut("capacity cap=%s" % tag, slice(0, N_CAPACITY), cap=cap)
                 for tag, cap in (("nmax", nmax), ("nmax-1", nmax - 1), ("nmax+37", nmax + 37)))


@functools.lru_cache(maxsize=None)
def degenerate_family():
    a, b = hermite(_site(3), 0.7, 11.0, 1.5, 0.1, -0.2), hermite(_site(11), -2.1, 6.0, -1.0, -0.15, 0.05)
    p = _site(17)
    return (Call("degenerate", [a[0], (p[0], p[1], 0.3), b[0]], [a[1], (p[0], p[1], -1.2), b[1]],
                 ["ordinary before", "start = end", "ordinary after"]),)


SHAPES = (1, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def shapes_family():
    base = curved_call()
    # from edge 250 on: random edges and the first south-bound ones
    return tuple(base.cut("shapes n_edges=%d" % m, slice(250, 250 + m)) for m in SHAPES)


def family(name):
    return {"step": step_family, "curved": curved_family, "limits": limits_family, "raceline": raceline_family, "capacity": capacity_family,
            "degenerate": degenerate_family, "shapes": shapes_family}[name]()


def all_calls():
    return [c for f in FAMILIES for c in family(f)]


_REF = {}


def reference(call, dtype=oref.LD, form="difference"):
    """The evaluation of ``call`` by tests/offline_ref.py, computed once per (call, number type, formulation) and shared: do not modify."""
    key = (call.name, np.dtype(dtype).name, form)
    if key not in _REF:
        _REF[key] = oref.evaluate(*call.args, dtype=dtype, form=form)
    return _REF[key]


def worst_of(evaluator):
    """{class: {quantity: worst deviation}} of ``evaluator(call)`` from the long-double reference over ALL calls of all families."""
    worst = {}
    for c in all_calls():
        ref = reference(c)
        oref.merge_worst(worst, oref.deviations(evaluator(c), ref), oref.edge_class(ref, STEP))
    return worst


@functools.lru_cache(maxsize=None)
def bounds():
    """THE bounds of every comparison of the kernel with the reference (offline_ref.derive_bounds): from the fp64 evaluation of the
    reference function, over every call of every family."""
    return oref.derive_bounds(worst_of(lambda c: reference(c, np.float64)))


@functools.lru_cache(maxsize=None)
def restatement_bounds():
    """The bounds oracle/offline_edges_ref.py is held to: derived the same way from the fp64 evaluation of the reference function IN THE
    RESTATEMENT'S FORMULATION (a2, a3 from absolute coordinates), which is what dominates its deviation."""
    return oref.derive_bounds(worst_of(lambda c: reference(c, np.float64, "absolute")))


def format_table(rows):
    """Text table: one line per (title, {class: {quantity: value}})."""
    lines = []
    for cls in ("regular", "micro"):
        lines.append("%-44s " % ("against long double, %s edges" % cls) + " ".join("%11s" % k for k in oref.QUANTITIES))
        for title, w in rows:
            lines.append("%-44s " % title + " ".join("%11.1e" % w[cls][k] for k in oref.QUANTITIES))
    return "\n".join(lines)
