"""Probe generators of the object-ingestion boundary tests (tests/test_object_cases_host.py on the CPU, tests/test_gpu_objects_boundary.py on
the GPU): object positions placed ON PURPOSE at the decision boundaries of `check_inside_bounds` (check_inside_bounds.py:7-59) -- the on-track
test of ObjectListInterface.process_object_list that decides whether an opponent exists for a planner at all -- in its forms
process_object_dev (csrc/ltpl_hip.hip: k_process_objects, and inlined into the simulation's k_fleet_sim_step / k_fleet_sim_mates) and the
oracle's check_inside_bounds (oracle/ltpl_oracle.c). Pure NumPy, seeded; nothing here runs a kernel.

THE FOUR DECISIONS, in the order the function takes them:
  1. the closest centre-line point nb: the FIRST minimum of dx * dx + dy * dy (the project's contract, as in tests/projection_cases.py; the
     reference's np.argpartition is not that on every exact tie, so there the oracle, not the reference, is the measure);
  2. the bracketing neighbour: ang1 >= ang2 of the two |angle3pt| (four atan2; the centre line is always taken as CLOSED, on the open track
     too) -> the segment (nb - 1, nb) or (nb, nb + 1). The device calls ITS atan2 here, the oracle libm's: on the tie locus |ang1| == |ang2|
     the last bit decides, and where the track's width changes along it the two segments give different verdicts near the bound;
  3. the closest of the 50 np.linspace points of that segment's centre line (point 49 is `stop` itself, not 49 * step + start);
  4. d_b1_2 > d_track_2 || d_b2_2 > d_track_2 with the bound points interpolated at that index: strict, so an object exactly ON an
     interpolated bound point (where d_b2_2 and d_track_2 are the same expression) is on the track.

RESTATEMENT (`restate`): check_inside_bounds.py operation by operation in fp64 (the angles in a scalar loop with math.atan2) and, per probe:
nb and n_min (the number of centre points that attain the minimum), ang1 - ang2 and the MARGIN ||ang1| - |ang2|| evaluated in np.longdouble,
the chosen segment (first: 1 = (nb - 1, nb), 0 = (nb, nb + 1)), the linspace index bi, the verdict and the verdict with the segment choice
FORCED either way (v_forced[0]: (nb, nb + 1), v_forced[1]: (nb - 1, nb)).

A `segment` probe is DECIDED when its margin exceeds `MARGIN` = 1e-12 rad (projection_cases.MARGIN, with the same argument: the atan2 form's
own rounding is some 1e-16 rad, every correct implementation takes the same branch above it). On an undecided probe either forced verdict is
right. Every probe of another family whose two forced verdicts agree, or whose margin exceeds MARGIN, is decided as well.

PROBE FAMILIES (each probe labelled; `OFFSETS` of tests/mask_cases.py reused, measured as displacement from the locus):
  bound     rays from the centre line towards either bound at along-track fractions 0, j / 49, 0.5, 1e-9, 1 - 1e-9 and random, bisected on the ray
            parameter down to adjacent doubles: the last parameter that is on the track and the next double (a PAIR: `pair` holds the
            partner's index), then the first displaced along the ray by the offsets
  index     the switch of the closest linspace point i -> i + 1 of the chosen segment (i = 0 and 48 always), at a lateral position between
            the two bound crossings that the indices i and i + 1 give (where they differ): bisected along the track to adjacent doubles (a
            pair), displaced along the track. Where both indices cross the bound at the same place (a track of one width: the oval) up to
            `INDEX_PLAIN` switches 0 / 1 and 48 / 49 are kept AT the bound without a pair. The bisected double often has d2[i] == d2[i + 1]
            EXACTLY: a tie among the linspace points (`n_min50` > 1), first minimum again
  segment   the tie locus |ang1| == |ang2| of nb = k (closed tracks: also k = 0 and L - 1, across the seam), at the middle of the lateral
            band in which the two forced verdicts differ; the band's edges by bisection of the lateral position on each forced verdict, the
            locus recomputed at every step; displaced along the track. Up to `SEGMENT_THIN` loci per lattice (and those of the seam) are
            kept at the bound although no band wider than `MIN_BAND` separates the forced verdicts there (the oval has no other)
  centre    the switch of the closest centre point k -> k + 1 (k = L - 1 -> 0 too), bisected along the track to adjacent doubles, at
            laterals 0, +- half the width and at either bound; displaced along the track
  tie       exact ties of the squared distance on the oval: midpoints of consecutive centre points of a straight (on the centre line and
            beside it), the oval's centre, points of the axis between the straights
  on-point  the object exactly on a centre point (atan2(0, 0) enters), exactly on b1 / b2 of a layer, exactly on an interpolated bound
            point of linspace index 1, 25 and 48
  special   NaN, +-inf and +-1e300 in x and / or y: nb and bi keep their initial 0 (no d2 compares below infinity), every load stays in
            range; arithmetic only -- NaN is ON the track (no `>` holds), the others are off it
"""
import math
import os

import numpy as np

import mask_cases
from mask_cases import OFFSETS
from projection_cases import MARGIN, _angle3pt, _angle3pt_ld, _bisect, _unit

FAMILIES = ("bound", "index", "segment", "centre", "tie", "on-point", "special")
FIXTURE_FAMILIES = FAMILIES[:6]
LATTICES = ("monteblanco", "millbrook", "open", "c3")
N_RAYS = {"monteblanco": 400, "millbrook": 400, "open": 400, "c3": 200}
RAY_FRACTIONS = (0.0, 1.0 / 49, 24.0 / 49, 25.0 / 49, 48.0 / 49, 0.5, 1e-9, 1.0 - 1e-9, 48.75 / 49)     # (the last two: linspace point 49, `stop` itself)
INDEX_LAYERS, INDEX_IS = 12, (0, 48, 1, 24, 47)
INDEX_PLAIN = 8           # switches i = 0 / 1 and 48 / 49 kept although the verdict cannot show them (a track of one width)
SEGMENT_THIN = 8          # tie loci kept at the bound although no band separates the forced verdicts there
CENTRE_LAYERS = 10
ON_POINT_IS = (1, 25, 48)
SPECIALS = (float("nan"), float("inf"), float("-inf"), 1e300, -1e300)
SEGMENT_STRIDE = {"c3": 16}   # every layer's tie locus is tried, on the oval (400 layers of one width) every sixteenth
MIN_BAND = 1e-6          # a tie locus counts when the band between the two forced bound crossings is wider than this [m]
I50 = np.arange(50.0)


class Track(object):
    """The three polylines of check_inside_bounds as ObjectListInterface.set_track_data forms them (ObjectListInterface.py:71-72,
    check_inside_bounds.py:28): b1, b2, c = (b1 + b2) / 2, [L, 2] each, and the widths."""

    def __init__(self, name, lat):
        self.name, self.closed, self.L = name, bool(lat.closed), int(lat.num_layers)
        refline, normvec = np.asarray(lat.refline, np.float64), np.asarray(lat.normvec, np.float64)
        self.wr, self.wl = np.asarray(lat.track_width_right, np.float64), np.asarray(lat.track_width_left, np.float64)
        self.b1 = refline + normvec * np.expand_dims(self.wr, 1)
        self.b2 = refline - normvec * np.expand_dims(self.wl, 1)
        self.c = (self.b1 + self.b2) / 2
        self.cx, self.cy = np.ascontiguousarray(self.c[:, 0]), np.ascontiguousarray(self.c[:, 1])

    def nbrs(self, nb):
        """(idx1, idx2) of get_s_coord.py:38-42 with closed = True, Python's negative index wrapped."""
        return (nb - 1) % self.L, (0 if nb + 1 > self.L - 1 else nb + 1)


def _lin(a, b, i):
    """np.linspace(a, b, 50)[i]: i * ((b - a) / 49) + a, the last point b itself."""
    return np.where(i == 49, b, i * ((b - a) / 49.0) + a)


def tail(T, a, b, qx, qy, bi=None):
    """Decisions 3 and 4 for the segment (a, b), vectorised over probes: (bi, verdict, number of the 50 points that attain the minimum);
    ``bi`` given: forced."""
    a, b, qx, qy = np.atleast_1d(a), np.atleast_1d(b), np.atleast_1d(np.asarray(qx, np.float64)), np.atleast_1d(np.asarray(qy, np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        n50 = np.zeros(a.shape, np.int64)
        if bi is None:
            lx, ly = _lin(T.cx[a][:, None], T.cx[b][:, None], I50[None, :]), _lin(T.cy[a][:, None], T.cy[b][:, None], I50[None, :])
            dx, dy = lx - qx[:, None], ly - qy[:, None]
            d2 = dx * dx + dy * dy
            bi = np.where(np.isnan(d2).all(axis=1), 0, np.argmin(np.where(np.isnan(d2), np.inf, d2), axis=1))
            n50 = np.count_nonzero(d2 == d2[np.arange(a.size), bi][:, None], axis=1)
        bi = np.broadcast_to(np.asarray(bi, np.int64), a.shape)
        f = bi.astype(np.float64)
        l1x, l1y = _lin(T.b1[a, 0], T.b1[b, 0], f), _lin(T.b1[a, 1], T.b1[b, 1], f)
        l2x, l2y = _lin(T.b2[a, 0], T.b2[b, 0], f), _lin(T.b2[a, 1], T.b2[b, 1], f)
        d_track_2 = (l1x - l2x) * (l1x - l2x) + (l1y - l2y) * (l1y - l2y)
        d_b1_2 = (l1x - qx) * (l1x - qx) + (l1y - qy) * (l1y - qy)
        d_b2_2 = (l2x - qx) * (l2x - qx) + (l2y - qy) * (l2y - qy)
        return bi, ~((d_b1_2 > d_track_2) | (d_b2_2 > d_track_2)), n50


def _closest(T, qx, qy):
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = T.cx - qx, T.cy - qy
        d2 = dx * dx + dy * dy
    if np.isnan(d2).all() or not np.any(d2 < np.inf):
        return 0, d2                                          # (no d2 compares below the initial infinity: nb keeps its 0)
    return int(np.argmin(d2)), d2


def _diff(T, nb, qx, qy):
    i1, i2 = T.nbrs(nb)
    nx, ny = float(T.cx[nb]), float(T.cy[nb])
    return (abs(_angle3pt(nx, ny, qx, qy, float(T.cx[i1]), float(T.cy[i1]))) - abs(_angle3pt(nx, ny, qx, qy, float(T.cx[i2]), float(T.cy[i2]))))


def evaluate(T, qx, qy, force=None):
    """One query, the scalar form of `restate` for the bisections: (nb, ang1 - ang2, first, a, b, bi, verdict)."""
    qx, qy = float(qx), float(qy)
    nb, _ = _closest(T, qx, qy)
    i1, i2 = T.nbrs(nb)
    d = _diff(T, nb, qx, qy)
    first = bool(d >= 0.0) if force is None else bool(force)
    a, b = (i1, nb) if first else (nb, i2)
    bi, v, _ = tail(T, a, b, qx, qy)
    return nb, d, first, a, b, int(bi[0]), bool(v[0])


class Restated(object):
    """Columns per probe: nb, n_min, idx1, idx2, ang1, ang2, diff, first, a, b, bi, n_min50 (the number of linspace points that attain the
    minimum), tie (an exact tie in decision 1 or 3: the contract is the first minimum), verdict, v_forced [2, m], margin (long double),
    decided."""


def restate(T, qx, qy):
    qx, qy = np.asarray(qx, np.float64), np.asarray(qy, np.float64)
    m = qx.size
    r = Restated()
    r.nb, r.n_min = np.zeros(m, np.int64), np.zeros(m, np.int64)
    for i in range(m):
        r.nb[i], d2 = _closest(T, qx[i], qy[i])
        with np.errstate(invalid="ignore"):
            r.n_min[i] = int(np.count_nonzero(d2 == d2[r.nb[i]]))
    r.idx1, r.idx2 = (r.nb - 1) % T.L, np.where(r.nb + 1 > T.L - 1, 0, r.nb + 1)
    cols = [v.tolist() for v in (T.cx[r.nb], T.cy[r.nb], qx, qy, T.cx[r.idx1], T.cy[r.idx1], T.cx[r.idx2], T.cy[r.idx2])]
    r.ang1 = np.array([abs(_angle3pt(nx, ny, px, py, x1, y1)) for nx, ny, px, py, x1, y1, _, _ in zip(*cols)], np.float64).reshape(-1)
    r.ang2 = np.array([abs(_angle3pt(nx, ny, px, py, x2, y2)) for nx, ny, px, py, _, _, x2, y2 in zip(*cols)], np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        r.diff = r.ang1 - r.ang2
        r.first = r.ang1 >= r.ang2
    _, v_second, _ = tail(T, r.nb, r.idx2, qx, qy)
    _, v_first, _ = tail(T, r.idx1, r.nb, qx, qy)
    r.v_forced = np.stack((v_second, v_first))
    r.a, r.b = np.where(r.first, r.idx1, r.nb), np.where(r.first, r.nb, r.idx2)
    r.bi, r.verdict, r.n_min50 = tail(T, r.a, r.b, qx, qy)
    r.tie = (r.n_min > 1) | (r.n_min50 > 1)
    with np.errstate(invalid="ignore"):
        a1 = np.abs(_angle3pt_ld(T.cx[r.nb], T.cy[r.nb], qx, qy, T.cx[r.idx1], T.cy[r.idx1]))
        a2 = np.abs(_angle3pt_ld(T.cx[r.nb], T.cy[r.nb], qx, qy, T.cx[r.idx2], T.cy[r.idx2]))
        r.margin = np.abs(a1 - a2)
        r.decided = (r.margin > MARGIN) | (r.v_forced[0] == r.v_forced[1])
    return r


# ---- families ---------------------------------------------------------------------------------------------------------------------------------
class _Rows(object):
    """Probe rows under construction: (qx, qy, family, k, offset, param, pair)."""

    def __init__(self):
        self.rows = []

    def add(self, q, fam, k, offset, param, pair=-1):
        self.rows.append((float(q[0]), float(q[1]), FAMILIES.index(fam), int(k), float(offset), float(param), int(pair)))
        return len(self.rows) - 1

    def add_locus(self, at, t0, fam, k, param, paired):
        """The probes of one locus: at(t0) and, ``paired``, at(next double) as its partner; then at(t0 + o) for the other offsets."""
        i0 = self.add(at(t0), fam, k, 0.0, param)
        if paired:
            i1 = self.add(at(np.nextafter(t0, np.inf)), fam, k, 0.0, param, pair=i0)
            r = self.rows[i0]
            self.rows[i0] = r[:6] + (i1,)
        for o in OFFSETS[1:]:
            self.add(at(t0 + o), fam, k, o, param)


def _bound_t(T, ox, oy, ux, uy, reach, inside):
    """Last ray parameter in [0, reach] for which ``inside`` holds (None: the origin is outside, or the far end inside)."""
    at = lambda t: (ox + t * ux, oy + t * uy)
    if not inside(*at(0.0)) or inside(*at(reach)):
        return None
    return _bisect(lambda t: inside(*at(t)), 0.0, reach)


def bound_probes(T, rows, n_rays, rng):
    L, found = T.L, 0
    for r in range(n_rays):
        l = int(rng.integers(0, L)) if r >= 8 else (0, L - 1, L - 2, 1)[r % 4]          # (the first rays at the seam)
        l2 = (l + 1) % L
        f = RAY_FRACTIONS[(r // 2) % len(RAY_FRACTIONS)] if r % 4 < 2 else float(rng.uniform(0.0, 1.0))
        bs = T.b1 if r % 2 == 0 else T.b2
        ox, oy = T.cx[l] * (1 - f) + T.cx[l2] * f, T.cy[l] * (1 - f) + T.cy[l2] * f
        tx, ty = bs[l, 0] * (1 - f) + bs[l2, 0] * f - ox, bs[l, 1] * (1 - f) + bs[l2, 1] * f - oy
        ux, uy = _unit(tx, ty)
        t0 = _bound_t(T, ox, oy, ux, uy, 2.0 * math.hypot(tx, ty) + 5.0, lambda x, y: evaluate(T, x, y)[6])
        if t0 is None:
            continue
        found += 1
        rows.add_locus(lambda t: (ox + t * ux, oy + t * uy), t0, "bound", l, f if r % 2 == 0 else -f - 1.0, True)
    return found


def index_probes(T, rows, rng):
    """(loci found, set of the indices i they switch from)."""
    L = T.L
    layers = sorted(set(rng.choice(L - 1, min(INDEX_LAYERS, L - 1), replace=False).tolist()))
    found, seen, n_plain = 0, set(), 0
    for l in layers:
        l2 = l + 1
        sx, sy = T.cx[l2] - T.cx[l], T.cy[l2] - T.cy[l]
        seg = math.hypot(sx, sy)
        for side in (1.0, -1.0):
            bs = T.b1 if side > 0 else T.b2
            nx, ny = -sy / seg, sx / seg
            if nx * (bs[l, 0] - T.cx[l]) + ny * (bs[l, 1] - T.cy[l]) < 0:
                nx, ny = -nx, -ny
            reach = 2.0 * max(math.hypot(bs[l, 0] - T.cx[l], bs[l, 1] - T.cy[l]), math.hypot(bs[l2, 0] - T.cx[l2], bs[l2, 1] - T.cy[l2])) + 5.0
            for i in INDEX_IS:
                al = (i + 0.5) / 49.0
                ox, oy = T.cx[l] + al * sx, T.cy[l] + al * sy
                ts = [_bound_t(T, ox, oy, nx, ny, reach, lambda x, y, j=j: bool(tail(T, l, l2, x, y, bi=j)[1][0])) for j in (i, i + 1)]
                if None in ts:
                    continue
                # (the two indices cross the bound at the same place, as everywhere on a track of one width: nothing to observe in the
                #  verdict; the switch is probed AT the bound all the same, as a locus without a pair)
                observable = abs(ts[0] - ts[1]) >= 1e-9
                if not observable and (n_plain >= INDEX_PLAIN or i not in (0, 48)):
                    continue
                t = (ts[0] + ts[1]) / 2
                at = lambda a: (T.cx[l] + a * sx + t * nx, T.cy[l] + a * sy + t * ny)

                def still_i(a):
                    e = evaluate(T, *at(a))
                    return None if (e[3], e[4]) != (l, l2) or e[5] not in (i, i + 1) else e[5] == i
                lo, hi = al - 0.4 / 49.0, al + 0.4 / 49.0
                if still_i(lo) is not True or still_i(hi) is not False:
                    continue
                a0 = _bisect(still_i, lo, hi)
                if a0 is None:
                    continue
                if evaluate(T, *at(a0))[6] == evaluate(T, *at(np.nextafter(a0, np.inf)))[6]:
                    if observable:
                        continue
                    n_plain += 1
                    observable = False
                else:
                    observable = True
                    found += 1
                seen.add(i)
                i0 = rows.add(at(a0), "index", l, 0.0, i)
                i1 = rows.add(at(np.nextafter(a0, np.inf)), "index", l, 0.0, i, pair=i0 if observable else -1)
                if observable:
                    rows.rows[i0] = rows.rows[i0][:6] + (i1,)
                for o in OFFSETS[1:]:
                    rows.add(at(a0 + o / seg), "index", l, o, i)
    return found, seen


def _locus(T, k, bx, by, tx, ty, h):
    """Along-track parameter of the tie locus of nb = k on the line (bx, by) + a (tx, ty): the last a with ang1 >= ang2."""
    pred = lambda a: _diff(T, k, bx + a * tx, by + a * ty) >= 0.0
    if not pred(-h) or pred(h):
        return None
    return _bisect(pred, -h, h)


def segment_probes(T, rows):
    """Tie loci of every (layer, side): (loci found, band widths [m])."""
    L = T.L
    widths, n_thin = [], 0
    for k in (range(0, L, SEGMENT_STRIDE.get(T.name, 1)) if T.closed else range(1, L - 1)):
        i1, i2 = T.nbrs(k)
        tx, ty = _unit(T.cx[i2] - T.cx[i1], T.cy[i2] - T.cy[i1])
        h = 0.45 * min(math.hypot(T.cx[k] - T.cx[i1], T.cy[k] - T.cy[i1]), math.hypot(T.cx[i2] - T.cx[k], T.cy[i2] - T.cy[k]))
        for side in (1.0, -1.0):
            bs = T.b1 if side > 0 else T.b2
            nx, ny = -ty, tx
            if nx * (bs[k, 0] - T.cx[k]) + ny * (bs[k, 1] - T.cy[k]) < 0:
                nx, ny = -nx, -ny
            reach = 2.0 * math.hypot(bs[k, 0] - T.cx[k], bs[k, 1] - T.cy[k]) + 5.0

            def on_locus(lat):
                bx, by = T.cx[k] + lat * nx, T.cy[k] + lat * ny
                a0 = _locus(T, k, bx, by, tx, ty, h)
                return None if a0 is None else (bx + a0 * tx, by + a0 * ty)

            def crossing(which):
                """Last lateral position at which the verdict forced to segment ``which`` (1: first) is on the track."""
                def inside(lat):
                    q = on_locus(lat)
                    if q is None:
                        return None
                    a, b = (i1, k) if which else (k, i2)
                    return bool(tail(T, a, b, q[0], q[1])[1][0])
                lo = 0.0                                      # (walked outwards: far beside the track the locus leaves nb = k's cell)
                while lo < reach and inside(lo) is True:
                    lo += 0.5
                if lo == 0.0 or inside(lo) is not False:
                    return None
                return _bisect(inside, lo - 0.5, lo)
            c = [crossing(0), crossing(1)]
            if None in c:
                continue
            thin = abs(c[0] - c[1]) <= MIN_BAND
            if thin and n_thin >= SEGMENT_THIN and not (T.closed and k in (0, L - 1)):
                continue
            lat = (c[0] + c[1]) / 2
            bx, by = T.cx[k] + lat * nx, T.cy[k] + lat * ny
            a0 = _locus(T, k, bx, by, tx, ty, h)
            if a0 is None:
                continue
            e = (evaluate(T, bx + a0 * tx, by + a0 * ty, force=0), evaluate(T, bx + a0 * tx, by + a0 * ty, force=1))
            if e[0][0] != k or (not thin and e[0][6] == e[1][6]):
                continue                                      # (another point is closer, or the band is too thin to stand in)
            if thin:
                n_thin += 1
            else:
                widths.append(abs(c[0] - c[1]))
            rows.add_locus(lambda a: (bx + a * tx, by + a * ty), a0, "segment", k, side * lat, False)
    return len(widths), np.array(widths)


def centre_probes(T, rows, rng):
    L = T.L
    ks = sorted(set(rng.choice(L, min(CENTRE_LAYERS, L), replace=False).tolist()) | {0, L - 2, L - 1})
    found = 0
    for k in ks:
        k2 = (k + 1) % L
        sx, sy = T.cx[k2] - T.cx[k], T.cy[k2] - T.cy[k]
        seg = math.hypot(sx, sy)
        tx, ty = sx / seg, sy / seg
        nx, ny = -ty, tx
        if nx * (T.b1[k, 0] - T.cx[k]) + ny * (T.b1[k, 1] - T.cy[k]) < 0:
            nx, ny = -nx, -ny
        mx, my = (T.cx[k] + T.cx[k2]) / 2, (T.cy[k] + T.cy[k2]) / 2
        w1, w2 = math.hypot(T.b1[k, 0] - T.cx[k], T.b1[k, 1] - T.cy[k]), math.hypot(T.b2[k, 0] - T.cx[k], T.b2[k, 1] - T.cy[k])
        lats = [0.0, w1 / 2, -w2 / 2]
        for s, w in ((1.0, w1), (-1.0, w2)):                  # at the bound: the last lateral on the track beside the middle of the segment
            t = _bound_t(T, mx, my, s * nx, s * ny, 2.0 * w + 5.0, lambda x, y: evaluate(T, x, y)[6])
            if t is not None:
                lats.append(s * t)
        h = 0.45 * seg
        for lat in lats:
            bx, by = mx + lat * nx, my + lat * ny
            at = lambda a: (bx + a * tx, by + a * ty)

            def still_k(a):
                nb = evaluate(T, *at(a))[0]
                return True if nb == k else (False if nb == k2 else None)
            if still_k(-h) is not True or still_k(h) is not False:
                continue
            a0 = _bisect(still_k, -h, h)
            if a0 is None:
                continue
            found += 1
            rows.add_locus(at, a0, "centre", k, lat, True)
    return found


def on_point_probes(T, rows, rng):
    L = T.L
    ks = sorted(set(rng.choice(L, min(8, L), replace=False).tolist()) | {0, 1, L - 1})
    for k in ks:
        rows.add((T.cx[k], T.cy[k]), "on-point", k, 0.0, 0.0)
        rows.add(T.b1[k], "on-point", k, 0.0, 1.0)
        rows.add(T.b2[k], "on-point", k, 0.0, 2.0)
        k2 = (k + 1) % L
        for i in ON_POINT_IS:
            f = np.float64(i)
            rows.add((_lin(T.b1[k, 0], T.b1[k2, 0], f), _lin(T.b1[k, 1], T.b1[k2, 1], f)), "on-point", k, 0.0, 100.0 + i)
            rows.add((_lin(T.b2[k, 0], T.b2[k2, 0], f), _lin(T.b2[k, 1], T.b2[k2, 1], f)), "on-point", k, 0.0, 200.0 + i)


def tie_probes(T, rows):
    """Candidates on the oval; only those at which two or more centre points attain the minimum EXACTLY are kept."""
    L = T.L
    cand = [(0.0, 0.0, 0)]
    straight = [k for k in range(L) if T.cy[k] == T.cy[(k + 1) % L]]
    for k in straight:
        k2 = (k + 1) % L
        mx = (T.cx[k] + T.cx[k2]) / 2
        for dy in (0.0, 1.5, -3.0):
            cand.append((mx, T.cy[k] + dy, k))
        cand.append((T.cx[k], 0.0, k))                         # the axis between the straights
        cand.append((mx, 0.0, k))
    for x, y, k in cand:
        _, d2 = _closest(T, x, y)
        if np.count_nonzero(d2 == d2.min()) > 1:
            rows.add((x, y), "tie", k, 0.0, 0.0)


def special_probes(rows):
    for i, x in enumerate(SPECIALS):
        rows.add((x, 10.0), "special", 0, 0.0, i)
        rows.add((-20.0, x), "special", 0, 0.0, i)
        for y in SPECIALS:
            rows.add((x, y), "special", 0, 0.0, i)


# ---- the sets -------------------------------------------------------------------------------------------------------------------------------------
class Probes(object):
    """Columns of m probes: qx, qy, family (index into FAMILIES), k (the layer the probe is about), offset, param (the family's parameter:
    along-track fraction, linspace index, lateral position), pair (index of the probe one double away across the boundary, -1: none)."""
    FIELDS = ("qx", "qy", "family", "k", "offset", "param", "pair")

    def __init__(self, rows):
        cols = list(zip(*rows))
        self.qx, self.qy = np.array(cols[0], np.float64), np.array(cols[1], np.float64)
        self.family, self.k = np.array(cols[2], np.int64), np.array(cols[3], np.int64)
        self.offset, self.param, self.pair = np.array(cols[4], np.float64), np.array(cols[5], np.float64), np.array(cols[6], np.int64)
        self.m = int(self.qx.size)


class ProbeSet(object):
    """name, track (Track), lat (Lattice), probes (Probes), ref (Restated), counts: rays / loci found per family, band_widths."""


_lattices, _sets = {}, {}


def lattice(name):
    if name not in _lattices:
        from graphbasedlocaltrajectoryplanner_amd.lattice import Lattice
        if name in mask_cases.LATTICES:
            _lattices[name] = mask_cases.lattice(name)           # (one object per process: the oval takes seconds to build)
        else:
            golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
            _lattices[name] = Lattice.load(os.path.join(golden, name + "_lattice.npz"))
    return _lattices[name]


def probe_set(name):
    """The probes of lattice ``name``: built once per process, shared and left unchanged."""
    if name not in _sets:
        lat = lattice(name)
        T = Track(name, lat)
        rng = np.random.default_rng(7000 + LATTICES.index(name))
        rows = _Rows()
        ps = ProbeSet()
        ps.name, ps.track, ps.lat, ps.counts = name, T, lat, {}
        ps.counts["bound"] = bound_probes(T, rows, N_RAYS[name], rng)
        ps.counts["index"], ps.index_seen = index_probes(T, rows, rng)
        ps.counts["segment"], ps.band_widths = segment_probes(T, rows)
        ps.counts["centre"] = centre_probes(T, rows, rng)
        if name == "c3":
            tie_probes(T, rows)
        on_point_probes(T, rows, rng)
        special_probes(rows)
        ps.probes = Probes(rows.rows)
        ps.ref = restate(T, ps.probes.qx, ps.probes.qy)
        _sets[name] = ps
    return _sets[name]


FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "objects_boundary.npz")
_fixture, _fixture_sets = {}, {}


def fixture(name):
    """The stored probes of lattice ``name`` (families of FIXTURE_FAMILIES, in the order of its probe set) and the verdicts of the UNMODIFIED
    reference on them (oracle/gen_golden_objects.py boundary): (Probes, verdict)."""
    if not _fixture:
        with np.load(FIXTURE) as z:
            off = np.concatenate(([0], np.cumsum(z["counts"])))
            for i, nm in enumerate(z["names"].tolist()):
                sl = slice(int(off[i]), int(off[i + 1]))
                rows = zip(z["qx"][sl], z["qy"][sl], z["family"][sl], z["k"][sl], np.asarray(OFFSETS)[z["offset_index"][sl]], z["param"][sl],
                           z["pair"][sl])
                _fixture[nm] = (Probes(list(rows)), z["verdict"][sl].astype(bool))
            _fixture["numpy"] = str(z["numpy_version"])
    return _fixture[name]


def fixture_set(name):
    """The probe set of lattice ``name`` WITHOUT its bisections: the stored probes of tests/golden/objects_boundary.npz (which
    tests/test_object_cases_host.py shows to be the generators' output bit for bit) and the `special` family behind them, restated."""
    if name not in _fixture_sets:
        stored, _ = fixture(name)
        rows = _Rows()
        special_probes(rows)
        sp = Probes(rows.rows)
        ps = ProbeSet()
        ps.name, ps.lat = name, lattice(name)
        ps.track = Track(name, ps.lat)
        ps.probes = Probes(list(zip(*[np.concatenate((getattr(stored, f), getattr(sp, f))) for f in Probes.FIELDS])))
        ps.ref = restate(ps.track, ps.probes.qx, ps.probes.qy)
        _fixture_sets[name] = ps
    return _fixture_sets[name]


def in_fixture(ps):
    return ps.probes.family < len(FIXTURE_FAMILIES)


def describe(ps, i):
    p = ps.probes
    return "%s on %s, layer %d, offset %+.0e, param %g, q (%.17g, %.17g)" % (FAMILIES[p.family[i]], ps.name, p.k[i], p.offset[i], p.param[i],
                                                                          p.qx[i], p.qy[i])
