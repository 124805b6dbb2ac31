"""Probe generators of the template tests (tests/test_template_cases_host.py on the CPU, tests/test_gpu_template.py on the GPU): scenarios
placed ON the decision boundaries of the three integer phases of the path kernel (csrc/paths_team.hpp) -- phase 1 (closest reference-line
layer per position, planning-range gate), phase 3 (closest object, closest node, action template) and phase 5 (horizon back-off,
`reduced`, the in_mod renaming). Pure NumPy, seeded; nothing here runs a kernel. The expected values come from tests/template_ref.py.

A PROBE is a dict: `family`, `kind` ("at" = the last double that still takes the first point of its pair, "ulp-" / "ulp+" = the doubles
beside it, "tie" = d2 exactly equal on both points and equal to the minimum over all, "off" = `offset` metres along the ray, "plain" = no
boundary of its own), `offset`, `pair` (the two layers or nodes), `scen` / `veh` / `pos` (scenario of its set, vehicle, position index
among the scenario's positions), `group` (ray) and whatever its family adds. Probes with |offset| >= 1e-9 m are DECIDED (fp64 and long
double agree); "at", "ulp-", "ulp+" and "tie" are held to the fp64 evaluation.

SETS per lattice (`case_set(name, which)`, built once and left unchanged):
  layer     bisector rays between layers l, l + 1 (lateral offset within +-1.5 track widths, bisected along the chord down to adjacent
            doubles, OFFSETS on either side), the exact ties found +-64 x +-8 ulps around the bisected point, the seam pair (L - 1, 0) on
            closed lattices (a tie takes layer 0: interval 2 against interval 1 of the cell), pairs more than 10 layers apart (where two
            parts of the track face each other; on the ovals the ties around an arc's centre, where all layers of the arc are equally far).
            Every probe comes twice: alone, and with a PARTNER position exactly on a border of the closest-layer grid -- an inner cell
            border in x, in y, a corner, and the grid's outer border from inside and from outside (the latter forces the full scan).
            One vehicle of radius 0.75 layer spacings: the two sides differ in the mask and in closest_obj_node.
  fullscan  a tie probe and ONE position off the grid among n in POSITION_COUNTS positions (the others lie on the reference line behind
            the gate and decide nothing), the probe at index 0, 63, 64 or last: the scenario rescans every position, in 64 / np2 segments
            of ceil(L / nseg) layers. Per configuration and team size one tie whose layers fall into different segments and one inside a
            segment, as far as the lattice has such a layer pair (n = 1 is the probe alone: the full scan of the handle without a grid).
  gate      single positions whose closest layer is sl - 2 .. sl and el .. el + 2, from sl = 0, sl = 1, a start with el = L - 1, a start
            across the seam and (open lattice) a start whose range ends in the last layer.
  object    layer distances H - 1, H, H + 1 and L - 1; two and three vehicles at the same distance with the winner at index 0, 63, 64,
            95 of 96 and the pair (3, 70); a last position behind the gate; first and last position in different layers on opposite sides
            of the track; a first position beside node 0 with the last one off the track (the left filter empties the object's layer); const_closest
            naming another vehicle.
  node      between nodes n, n + 1 of the object's layer exactly as for layers, beyond the first and last node, and the one-node layer.
            The nodes of a layer lie on a straight line, so the closest node is one of the two beside the query's projection: a tie
            between n and n + 64 at the minimum cannot exist. What a layer of 70 nodes does offer is the tie (63, 64) -- the lower node in
            lane 63, the higher in lane 0 -- and ties (n, n + 1) with n >= 64, both in the second node of their lanes.
  template  the full table action_sets x obj_in_const x obj_besides x last_action x {object, none} x const_closest {unset, set}.
  backoff   a zone wall d in {1, 2, 3, H - 1, H} layers ahead with an object at d - 2 .. d + 1, plain, across the seam, on the open
            lattice ending in the last layer, and with obj_in_const.
"""
import numpy as np

import mask_cases as mc
import template_ref as tr

OFFSETS = tuple(s * o for o in (1e-9, 1e-6, 1e-3, 0.1) for s in (1.0, -1.0))
POSITION_COUNTS = (1, 2, 3, 5, 9, 17, 33, 63, 64, 65, 128, 192)
WALL_D = ("1", "2", "3", "H-1", "H")
LAST_ACTIONS = (None, "straight", "left", "right", "follow")
MAX_TIES_PER_RAY = 4
SET_NAMES = ("layer", "fullscan", "gate", "object", "node", "template", "backoff")
LAYER_SETS = ("layer", "fullscan", "gate")
LATTICES = ("monteblanco", "open", "C", "V", "c3")
N_RAYS = {"monteblanco": (70, 16, 24), "open": (70, 0, 0), "C": (60, 12, 0), "V": (32, 8, 0), "c3": (30, 16, 0)}     # adjacent, seam, far pairs
N_NODE_RAYS, N_NODE_TIE_RAYS = 60, 300
W_LAST = [0.0, 0.5, 0.8]

_lattices, _sets, _grids = {}, {}, {}


def lattice(name):
    if name not in _lattices:
        if name == "V":
            import sweep_cases
            _lattices[name] = sweep_cases.lattice("V")
        else:
            _lattices[name] = mc.lattice(name)
    return _lattices[name]


def grid(name):
    """(origin x, origin y, 1 / cell), (nx, ny), cells [nx * ny, 4] of the lattice's closest-layer grid (ltpl_layer_grid)."""
    if name not in _grids:
        from test_layer_grid import grid_of
        _, _, oc, dims, cells = grid_of(lattice(name))
        _grids[name] = (oc, dims, cells)
    return _grids[name]


def spacing(lat):
    return float(np.median(np.hypot(*np.diff(lat.refline, axis=0).T)))


def scenario(lat, sl, vehicles, sn=None, **kw):
    sc = mc.scenario(lat, sl, list(vehicles))
    if sn is not None:
        sc["start_node"] = (int(sl), int(sn))
    sc.update(kw)
    return sc


def one(x, y):
    return np.array([[float(x), float(y)]])


# ---- boundaries between two points of a set (layers of the reference line, nodes of a layer) -------------------------------------------
def _takes_first(ax, ay, bx, by, first_lower, qx, qy):
    """The first minimum of the pair falls on A: strictly closer, or as close and the lower index."""
    dxa, dya, dxb, dyb = ax - qx, ay - qy, bx - qx, by - qy
    da, db = dxa * dxa + dya * dya, dxb * dxb + dyb * dyb
    return (da < db) | ((da == db) & first_lower)


def bisect_rays(A, B, first_lower, lateral):
    """Rays through M + n * lateral (M = midpoint of A and B, n = normal of the chord) along the chord A -> B: (origin, direction, r0) with the
    query origin + r * direction taking A at r = r0 and B at the next double."""
    ch = B - A
    ln = np.hypot(ch[:, 0], ch[:, 1])
    u = ch / ln[:, None]
    nrm = np.stack((-u[:, 1], u[:, 0]), axis=1)
    o = (A + B) / 2 + nrm * np.asarray(lateral)[:, None]
    f = lambda r: _takes_first(A[:, 0], A[:, 1], B[:, 0], B[:, 1], first_lower, o[:, 0] + r * u[:, 0], o[:, 1] + r * u[:, 1])
    lo, hi = -ln / 2, ln / 2
    ok = f(lo) & ~f(hi)
    for _ in range(200):
        mid = lo + (hi - lo) / 2
        done = (mid <= lo) | (mid >= hi)
        if done.all():
            break
        t = f(mid)
        lo, hi = np.where(~done & t, mid, lo), np.where(~done & ~t, mid, hi)
    ok &= (np.nextafter(lo, np.inf) == hi) & f(lo) & ~f(hi)
    return o, u, lo, ok


def _ulps(q, span):
    cols, dn, up = [q], q, q
    for _ in range(span):
        dn, up = np.nextafter(dn, -np.inf), np.nextafter(up, np.inf)
        cols.insert(0, dn); cols.append(up)
    return np.stack(cols, axis=1)


def exact_ties(px, py, a, b, qx, qy):
    """[(ray, x, y)]: the doubles +-64 ulps in x and +-8 ulps in y around (qx, qy) with d2 to points a and b EXACTLY equal and equal to the
    minimum over all points (px, py); at most MAX_TIES_PER_RAY per ray, the nearest to the centre first."""
    out = []
    gx, gy = _ulps(qx, 64), _ulps(qy, 8)                                  # [n, 129], [n, 17]
    for i in range(len(qx)):
        X, Y = np.meshgrid(gx[i], gy[i], indexing="ij")
        dxa, dya, dxb, dyb = px[a[i]] - X, py[a[i]] - Y, px[b[i]] - X, py[b[i]] - Y
        tie = np.argwhere((dxa * dxa + dya * dya) == (dxb * dxb + dyb * dyb))
        tie = tie[np.argsort(np.abs(tie[:, 0] - 64) + np.abs(tie[:, 1] - 8), kind="stable")]
        n = 0
        for ix, iy in tie:
            x, y = gx[i, ix], gy[i, iy]
            d2 = tr.dist2(px, py, np.array([x]), np.array([y]), np.float64)[0]
            if d2[a[i]] == d2.min() and d2[b[i]] == d2.min():
                out.append((i, float(x), float(y)))
                n += 1
                if n == MAX_TIES_PER_RAY:
                    break
    return out


def boundary_probes(px, py, a, b, lateral, family, offsets=OFFSETS):
    """The probes of rays between points a[i] and b[i] of (px, py): per accepted ray "at", "ulp-", "ulp+", the OFFSETS and its exact ties.
    A ray is accepted when the pair holds the minimum over ALL points on both sides of its boundary. Returns (probes without scenario,
    number of rays accepted)."""
    P = np.stack((px, py), axis=1)
    o, u, r0, ok = bisect_rays(P[a], P[b], a < b, lateral)
    q = lambda r: (o[:, 0] + r * u[:, 0], o[:, 1] + r * u[:, 1])
    for r in (r0, np.nextafter(r0, np.inf)):
        d2 = tr.dist2(px, py, *q(r), np.float64)
        ok &= np.minimum(d2[np.arange(len(a)), a], d2[np.arange(len(a)), b]) == d2.min(axis=1)
    keep = np.nonzero(ok)[0]
    probes = []
    variants = [("at", 0.0, r0), ("ulp-", 0.0, np.nextafter(r0, -np.inf)), ("ulp+", 0.0, np.nextafter(r0, np.inf))]
    variants += [("off", off, r0 + off) for off in offsets]
    for kind, off, r in variants:
        x, y = q(r)
        for i in keep:
            probes.append(dict(family=family, kind=kind, offset=off, pair=(int(a[i]), int(b[i])), group=int(i), x=float(x[i]), y=float(y[i])))
    x0, y0 = q(r0)
    for i, x, y in exact_ties(px, py, a[keep], b[keep], x0[keep], y0[keep]):
        i = keep[i]
        probes.append(dict(family=family, kind="tie", offset=0.0, pair=(int(a[i]), int(b[i])), group=int(i), x=x, y=y))
    return probes, len(keep)


def far_pairs(lat):
    """Layer pairs more than 10 layers apart whose reference points face each other (the closest such partner of every layer)."""
    L = lat.num_layers
    d = np.hypot(lat.refline[:, None, 0] - lat.refline[None, :, 0], lat.refline[:, None, 1] - lat.refline[None, :, 1])
    idx = np.arange(L)
    sep = np.abs(idx[:, None] - idx[None, :])
    if lat.closed:
        sep = np.minimum(sep, L - sep)
    d[sep <= 10] = np.inf
    q = np.argmin(d, axis=1)
    order = np.argsort(d[idx, q])
    return idx[order], q[order]


def arc_centre_ties(lat, limit=40):
    """Exact ties between layers more than 10 apart around the centre of an arc of the reference line (all layers of the arc are equally
    far up to rounding): the doubles +-64 x +-8 ulps around the circumcentres of layer triples."""
    L, R = lat.num_layers, lat.refline
    out, seen = [], set()
    for i in range(0, L, max(L // 16, 1)):
        A, B, C = R[i], R[(i + 3) % L], R[(i + 6) % L]
        d = 2.0 * (A[0] * (B[1] - C[1]) + B[0] * (C[1] - A[1]) + C[0] * (A[1] - B[1]))
        if abs(d) < 1e-6:
            continue
        ux = ((A @ A) * (B[1] - C[1]) + (B @ B) * (C[1] - A[1]) + (C @ C) * (A[1] - B[1])) / d
        uy = ((A @ A) * (C[0] - B[0]) + (B @ B) * (A[0] - C[0]) + (C @ C) * (B[0] - A[0])) / d
        if (round(ux, 3), round(uy, 3)) in seen or abs(ux) > 1e5:
            continue
        seen.add((round(ux, 3), round(uy, 3)))
        # the circumcentre of three points carries their cancellation error (1e-11 m: thousands of ulps of d2); refine it by the algebraic
        # circle fit over all layers of the arc in long double (normal equations solved by Cramer's rule)
        ld = np.longdouble
        rad = np.hypot(R[:, 0] - ux, R[:, 1] - uy)
        arc = np.abs(rad - np.hypot(A[0] - ux, A[1] - uy)) < 1e-6
        if arc.sum() < 8:
            continue
        px, py = R[arc, 0].astype(ld) - ld(ux), R[arc, 1].astype(ld) - ld(uy)
        z = px * px + py * py
        mx, my, mz = px.mean(), py.mean(), z.mean()
        sxx, sxy, syy = ((px - mx) ** 2).sum(), ((px - mx) * (py - my)).sum(), ((py - my) ** 2).sum()
        sxz, syz = ((px - mx) * (z - mz)).sum(), ((py - my) * (z - mz)).sum()
        det = sxx * syy - sxy * sxy
        ux, uy = float(ld(ux) + (sxz * syy - syz * sxy) / det / 2), float(ld(uy) + (sxx * syz - sxy * sxz) / det / 2)
        X, Y = np.meshgrid(_ulps(np.array([ux]), 64)[0], _ulps(np.array([uy]), 8)[0], indexing="ij")
        d2 = tr.dist2(R[:, 0], R[:, 1], X.ravel(), Y.ravel(), np.float64)
        first = np.argmin(d2, axis=1)
        at_min = d2 == d2.min(axis=1)[:, None]
        last = L - 1 - np.argmax(at_min[:, ::-1], axis=1)
        sep = np.abs(last - first)
        if lat.closed:
            sep = np.minimum(sep, L - sep)
        for k in np.nonzero(sep > 10)[0][:limit // 2]:
            out.append(dict(family="far", kind="tie", offset=0.0, pair=(int(first[k]), int(last[k])), group=-1, x=float(X.ravel()[k]), y=float(Y.ravel()[k])))
    return out[:limit]


def start_for(lat, layer, rng):
    """A start layer whose planning range holds ``layer`` (2 .. H - 2 layers ahead where the lattice allows)."""
    return mc.start_layer_for(lat, int(layer), rng)


def reachable_layers(lat):
    t = mc.table(lat)
    L = lat.num_layers
    reach = np.zeros(L, bool)
    for s in np.nonzero(t.H > 0)[0]:
        reach[(s + np.arange(1, t.H[s] + 1)) % L] = True
    return reach


class CaseSet(object):
    """``scen`` (scenario dicts), ``probes`` (dicts, see the module docstring; a scenario may carry several probes or none)."""

    def __init__(self, lat, name, which):
        self.lat, self.name, self.which, self.scen, self.probes = lat, name, which, [], []

    def add(self, sc, *probes):
        for p in probes:
            q = dict(p)
            q["scen"] = len(self.scen)
            q.setdefault("veh", 0); q.setdefault("pos", 0)
            self.probes.append(q)
        self.scen.append(sc)
        return len(self.scen) - 1

    def pad(self, n=64):
        """At least ``n`` scenarios per call (the one-wave form): the first scenarios again, without probes."""
        k = 0
        while len(self.scen) < n:
            self.scen.append(self.scen[k]); k += 1


# ---- the sets -----------------------------------------------------------------------------------------------------------------------------
def layer_probes(name):
    """The boundary probes between layers of lattice ``name`` (no scenarios yet): adjacent pairs, the seam pair, far pairs."""
    lat = lattice(name)
    rng = np.random.default_rng(7000 + LATTICES.index(name))
    L, R = lat.num_layers, lat.refline
    n_adj, n_seam, n_far = N_RAYS[name]
    reach = reachable_layers(lat)
    tw = float(np.mean(lat.track_width_left + lat.track_width_right))
    out = []
    pool = np.nonzero(reach[1:] & reach[:-1])[0]                               # l with l and l + 1 both in some planning range
    a = rng.choice(pool, 3 * n_adj, replace=len(pool) < 3 * n_adj)
    p, n_ok = boundary_probes(R[:, 0], R[:, 1], a, a + 1, rng.uniform(-1.5 * tw, 1.5 * tw, len(a)), "adjacent")
    groups = sorted({q["group"] for q in p})[:n_adj]
    out += [q for q in p if q["group"] in groups]
    if n_seam:
        a = np.full(4 * n_seam, L - 1)
        p, _ = boundary_probes(R[:, 0], R[:, 1], a, np.zeros_like(a), rng.uniform(-1.0 * tw, 1.0 * tw, len(a)), "seam")
        groups = sorted({q["group"] for q in p})[:n_seam]
        out += [dict(q, group=q["group"] + 10000) for q in p if q["group"] in groups]
    if n_far:
        a, b = far_pairs(lat)
        a, b = np.repeat(a[:2 * n_far], 3), np.repeat(b[:2 * n_far], 3)
        p, _ = boundary_probes(R[:, 0], R[:, 1], a, b, rng.uniform(-2.0, 2.0, len(a)), "far")
        groups = sorted({q["group"] for q in p})[:n_far]
        out += [dict(q, group=q["group"] + 20000) for q in p if q["group"] in groups]
    if name in ("C", "V", "c3"):
        out += arc_centre_ties(lat)
    return out


def partner_position(name, which, layer=0):
    """A position exactly on a border of the closest-layer grid. "cell-x" / "cell-y" / "corner": on the left / lower border / the corner of
    the cell that holds the reference point of ``layer``, exactly as the kernel's look-up sees it (the smallest double whose scaled
    coordinate reaches the integer); "outer-in" / "outer-out": on the grid's left border and one double outside it."""
    lat = lattice(name)
    oc, dims, _ = grid(name)
    cell = 1.0 / oc[2]
    if which.startswith("outer"):
        # a point of the left or the lower border whose closest layer is ``layer`` or as near to it as the border offers
        f = (np.arange(32) + 0.5) / 32
        bx = np.concatenate((np.full(32, oc[0]), oc[0] + f * dims[0] * cell))
        by = np.concatenate((oc[1] + f * dims[1] * cell, np.full(32, oc[1])))
        ol = tr.closest_layers(lat, bx, by)[0]
        sep = np.abs(ol - layer)
        k = int(np.argmin(np.minimum(sep, lat.num_layers - sep) if lat.closed else sep))       # (first minimum: the same point for in and out)
        x, y = float(bx[k]), float(by[k])
        if which == "outer-out":
            x, y = (float(np.nextafter(x, -np.inf)), y) if k < 32 else (x, float(np.nextafter(y, -np.inf)))
        return x, y
    ix, iy = int((lat.refline[layer, 0] - oc[0]) * oc[2]), int((lat.refline[layer, 1] - oc[1]) * oc[2])
    bx, by = oc[0] + ix * cell, oc[1] + iy * cell
    while (bx - oc[0]) * oc[2] < ix:
        bx = np.nextafter(bx, np.inf)
    while (by - oc[1]) * oc[2] < iy:
        by = np.nextafter(by, np.inf)
    return (float(bx) if which != "cell-y" else float(lat.refline[layer, 0]), float(by) if which != "cell-x" else float(lat.refline[layer, 1]))


def behind_the_gate(lat, sl):
    """Layers whose positions fail the gate of start layer ``sl`` with room to spare (they decide nothing)."""
    L, H = lat.num_layers, int(mc.table(lat).H[sl])
    if lat.closed:
        return [(sl + H + 3 + j) % L for j in range(max(L - H - 6, 1))]
    return [j for j in range(L) if j < sl - 2 or j > sl + H + 2]


PARTNERS = ("cell-x", "cell-y", "corner", "outer-in", "outer-out")


def layer_set(name):
    lat = lattice(name)
    cs = CaseSet(lat, name, "layer")
    rng = np.random.default_rng(7100 + LATTICES.index(name))
    radius = 0.75 * spacing(lat)
    starts = {}
    for i, p in enumerate(layer_probes(name)):
        key = (p["family"], p["group"], p["pair"])
        if key not in starts:                                                   # the probes of a ray share their start layer
            target = max(p["pair"]) if p["family"] == "adjacent" else min(p["pair"])
            starts[key] = start_for(lat, target, rng)
        sl = starts[key]
        cs.add(scenario(lat, sl, [(radius, one(p["x"], p["y"]))]), dict(p, partner=None))
        which = PARTNERS[p["group"] % len(PARTNERS)]                            # (the probes of a ray share their partner)
        far = behind_the_gate(lat, sl)
        partner = partner_position(name, which, far[len(far) // 2])
        assert which.startswith("outer") or int(tr.closest_layers(lat, *partner)[0][0]) in far, (name, which, sl)
        cs.add(scenario(lat, sl, [(radius, one(p["x"], p["y"])), (1.0, one(*partner))]), dict(p, partner=which))
    return cs


def scan_shape(L, n, index, team):
    """(segments, layers per segment) of the full scan for position ``index`` of ``n`` in a team of ``team`` waves."""
    cnt = min(64, n - 64 * (index // 64))
    wave = (index % 64) % team
    cntw = (cnt - wave + team - 1) // team
    np2 = 1
    while np2 < cntw:
        np2 <<= 1
    nseg = 64 // np2
    return nseg, (L + nseg - 1) // nseg


def tie_bank(name):
    """{lower layer l: tie probe between l and l + 1} for as many l as eight rays per pair find."""
    lat = lattice(name)
    rng = np.random.default_rng(7200 + LATTICES.index(name))
    R, L = lat.refline, lat.num_layers
    reach = reachable_layers(lat)
    pool = np.nonzero(reach[1:] & reach[:-1])[0]
    a = np.repeat(pool, 8)
    p, _ = boundary_probes(R[:, 0], R[:, 1], a, a + 1, rng.uniform(-6.0, 6.0, len(a)), "adjacent")
    bank = {}
    for q in p:
        if q["kind"] == "tie":
            bank.setdefault(q["pair"][0], q)
    return bank


def fullscan_set(name):
    lat = lattice(name)
    cs = CaseSet(lat, name, "fullscan")
    rng = np.random.default_rng(7300 + LATTICES.index(name))
    L, t = lat.num_layers, mc.table(lat)
    bank = tie_bank(name)
    radius = 0.75 * spacing(lat)
    for n in POSITION_COUNTS:
        for index in sorted({0, 63, 64, n - 1}):
            if index >= n or (n > 1 and n == index + 1 and index == 0):
                continue
            for team in (1, 4):
                nseg, chunk = scan_shape(L, n, index, team)
                want = []
                if nseg >= 2:
                    want.append(("straddle", [l for l in sorted(bank) if (l + 1) % chunk == 0]))
                if chunk >= 2:
                    want.append(("inside", [l for l in sorted(bank) if (l + 1) % chunk != 0]))
                for where, ls in want:
                    if not ls:
                        continue
                    p = bank[ls[int(rng.integers(0, len(ls)))]]
                    l = p["pair"][0]
                    sl = start_for(lat, l + 1, rng)
                    # the other positions: one off the grid, the rest on reference points behind the gate (they decide nothing)
                    behind = behind_the_gate(lat, sl)
                    off_grid = partner_position(name, "outer-out", behind[len(behind) // 2])
                    vehicles, k_left, first = [], n - 1, True
                    while k_left > 0:
                        m = min(k_left, 3 if n > 90 else 1)
                        if first:
                            pts = [off_grid] + [tuple(lat.refline[behind[0]])] * (m - 1)
                            first = False
                        else:
                            pts = [tuple(lat.refline[behind[int(rng.integers(0, len(behind)))]] + rng.uniform(-0.5, 0.5, 2)) for _ in range(m)]
                        vehicles.append((1.0, np.array(pts)))
                        k_left -= m
                    # the probe's vehicle goes where its position gets index ``index``
                    slot, cnt = 0, 0
                    while slot < len(vehicles) and cnt + len(vehicles[slot][1]) <= index:
                        cnt += len(vehicles[slot][1]); slot += 1
                    if cnt != index:                                            # (a vehicle of 3 straddles the index: split it)
                        r, pts = vehicles[slot]
                        vehicles[slot:slot + 1] = [(r, pts[:index - cnt]), (r, pts[index - cnt:])]
                        slot += 1
                    vehicles.insert(slot, (radius, one(p["x"], p["y"])))
                    assert sum(len(v[1]) for v in vehicles) == n and len(vehicles) <= mc.MAX_VEH
                    s1, s4 = scan_shape(L, n, index, 1), scan_shape(L, n, index, 4)
                    cs.add(scenario(lat, sl, vehicles), dict(p, family="fullscan", veh=slot, pos=index, n_pos=n, team=team, where=where,
                                                             nseg=nseg, chunk=chunk, shape1=s1, shape4=s4))
    cs.pad()
    return cs


def gate_set(name):
    lat = lattice(name)
    cs = CaseSet(lat, name, "gate")
    L, t = lat.num_layers, mc.table(lat)
    starts = []
    valid = np.nonzero(t.H > 0)[0]
    for what, cond in (("sl=0", lambda s: s == 0), ("sl=1", lambda s: s == 1), ("el=L-1", lambda s: lat.horizon_end_layer(s) == L - 1),
                       ("seam", lambda s: lat.closed and s + t.H[s] >= L + 2), ("open-last", lambda s: not lat.closed and lat.horizon_end_layer(s) == L - 1)):
        hit = [int(s) for s in valid if cond(int(s))]
        if hit:
            starts.append((what, hit[0]))
    radius = 0.75 * spacing(lat)
    for what, sl in starts:
        el = lat.horizon_end_layer(sl)
        for rel, layer in (("sl-2", sl - 2), ("sl-1", sl - 1), ("sl", sl), ("el", el), ("el+1", el + 1), ("el+2", el + 2)):
            layer = layer % L if lat.closed else layer
            if not 0 <= layer < L:
                continue
            for lateral in (-3.0, 0.0, 2.5):
                q = lat.refline[layer] + lat.normvec[layer] * lateral
                cs.add(scenario(lat, sl, [(radius, one(*q))]), dict(family="gate", kind="plain", offset=0.0, pair=(layer, layer), group=len(cs.scen),
                                                                     start=what, rel=rel, x=float(q[0]), y=float(q[1])))
    cs.pad()
    return cs


def track_point(lat, layer, lateral=0.0):
    return lat.refline[layer % lat.num_layers] + lat.normvec[layer % lat.num_layers] * lateral


def object_set(name):
    lat = lattice(name)
    cs = CaseSet(lat, name, "object")
    L, t = lat.num_layers, mc.table(lat)
    valid = [int(s) for s in np.nonzero(t.H > 1)[0]]
    pick = {valid[0], valid[len(valid) // 3], valid[(2 * len(valid)) // 3], valid[-1]}
    if lat.closed:
        pick.add(max(s for s in valid if s + t.H[s] >= L + 2))                  # a range across the seam
    pick = sorted(pick)
    lay = lambda sl, d: (sl + d) % L if lat.closed else sl + d
    ok = lambda l: 0 <= l < L
    for sl in pick:
        H = int(t.H[sl])
        # layer distances at the bound
        for what, d in (("H-1", H - 1), ("H", H), ("H+1", H + 1), ("L-1", -1)):
            l = lay(sl, d)
            if ok(l):
                cs.add(scenario(lat, sl, [(0.8, one(*track_point(lat, l, 1.0)))]), dict(family="distance", kind="plain", offset=0.0, pair=(l, l), what=what, group=sl))
        # ties in the layer distance: the first vehicle wins
        near, far = lay(sl, max(H // 2, 1)), lay(sl, min(max(H // 2, 1) + 2, H))
        if ok(near) and ok(far):
            for n_tied in (2, 3):
                for winner, second in ((0, 1), (63, 64), (64, 65), (95, None), (3, 70)):
                    tied = [winner] + ([] if second is None else [second]) + ([winner + 20] if n_tied == 3 and second != 70 and winner + 20 < 96 else [])
                    if second == 70 and n_tied == 3:
                        tied.append(90)
                    tied = sorted(set(tied))
                    vehicles = []
                    for k in range(96):
                        lateral = -3.0 + 6.0 * ((k * 7) % 13) / 12.0             # every vehicle at a lateral position of its own
                        if k in tied:
                            vehicles.append((0.5, one(*track_point(lat, near, lateral))))
                        elif k < winner:
                            vehicles.append((0.5, np.vstack((one(*track_point(lat, near, lateral)), one(*track_point(lat, far, lateral))))))   # earlier, farther: its LAST position counts
                        else:
                            vehicles.append((0.5, one(*track_point(lat, far, lateral))))
                    cs.add(scenario(lat, sl, vehicles), dict(family="index-tie", kind="plain", offset=0.0, pair=(near, near), veh=winner,
                                                             pos=2 * winner, tied=tuple(tied), group=sl))
        # last position behind the gate, earlier ones in range
        behind = lay(sl, H + 3)
        mid = lay(sl, max(H // 2, 1))
        if ok(behind) and ok(mid) and (not lat.closed or L - H - 4 >= 1):
            pts = np.vstack((one(*track_point(lat, mid, 0.5)), one(*track_point(lat, behind, 0.5))))
            cs.add(scenario(lat, sl, [(0.8, pts)]), dict(family="last-gated", kind="plain", offset=0.0, pair=(mid, behind), group=sl))
            cs.add(scenario(lat, sl, [(0.8, pts), (0.8, one(*track_point(lat, lay(sl, min(H, max(H // 2, 1) + 1)), -1.0)))]),
                   dict(family="last-gated", kind="plain", offset=0.0, pair=(mid, behind), group=sl))
        # first and last position in different layers, on opposite sides: node from the first, layer from the last
        a, b = lay(sl, 1), lay(sl, min(3, H))
        if ok(a) and ok(b) and a != b:
            for s in (1.0, -1.0):
                pts = np.vstack((one(*track_point(lat, a, 3.0 * s)), one(*track_point(lat, b, -3.0 * s))))
                cs.add(scenario(lat, sl, [(0.5, pts)]), dict(family="first-last", kind="plain", offset=0.0, pair=(a, b), group=sl))
                cs.add(scenario(lat, sl, [(0.5, pts[::-1].copy())]), dict(family="first-last", kind="plain", offset=0.0, pair=(b, a), group=sl))
                # ... and as vehicle 70 of 72 (its first position is read from memory, not from a lane)
                others = [(0.5, one(*track_point(lat, lay(sl, min(H, 5)), -3.0 + 0.08 * k))) for k in range(72)]
                if ok(lay(sl, min(H, 5))) and min(H, 5) > min(3, H):
                    others[70] = (0.5, pts)
                    cs.add(scenario(lat, sl, others), dict(family="first-last", kind="plain", offset=0.0, pair=(a, b), veh=70, pos=70, group=sl))
        # the closest node is node 0 and nothing stands on the track: the left filter (n >= cn) leaves the object's layer no node, the right
        # filter (n < cn) removes none. First position beside node 0 of a layer in front, last position beyond the last node of the object's.
        off = lat.layer_off.astype(np.int64)
        if ok(a) and ok(b) and a != b and min(lat.nodes_in_layer[a], lat.nodes_in_layer[b]) >= 2:
            ends = lambda l: (lat.node_pos[off[l]], lat.node_pos[off[l + 1] - 1])
            (a0, ak), (b0, bk) = ends(a), ends(b)
            pts = np.vstack((one(*(a0 + (a0 - ak) / np.hypot(*(a0 - ak)) * 6.0)), one(*(bk + (bk - b0) / np.hypot(*(bk - b0)) * 6.0))))
            for k_veh in (0, 70):
                others = [(0.2, one(*track_point(lat, lay(sl, H + 3) if ok(lay(sl, H + 3)) else b, 0.1 * k))) for k in range(k_veh)]
                cs.add(scenario(lat, sl, others + [(0.2, pts)]), dict(family="left-empty", kind="plain", offset=0.0, pair=(a, b), veh=k_veh, pos=k_veh, group=sl))
        # const_closest names another vehicle than the computed one
        if ok(near) and ok(far):
            v = [(0.5, one(*track_point(lat, far, 1.0))), (0.5, one(*track_point(lat, near, -1.0))), (0.5, one(*track_point(lat, far, 0.0)))]
            for cc in (0, 2):
                cs.add(scenario(lat, sl, v, const_closest=cc), dict(family="const-closest", kind="plain", offset=0.0, pair=(near, far), veh=1, pos=1, group=sl))
    cs.pad()
    return cs


def node_probes(name):
    lat = lattice(name)
    rng = np.random.default_rng(7400 + LATTICES.index(name))
    L, off = lat.num_layers, lat.layer_off.astype(np.int64)
    reach = reachable_layers(lat)
    sp = spacing(lat)
    out = []
    layers = np.nonzero(reach & (lat.nodes_in_layer >= 2))[0]
    n_all = N_NODE_RAYS + N_NODE_TIE_RAYS                                       # (the rays behind the first N_NODE_RAYS contribute their ties only)
    pick = rng.choice(layers, n_all)
    n_lo = (rng.random(n_all) * (lat.nodes_in_layer[pick] - 1)).astype(np.int64)
    wide = np.nonzero(lat.nodes_in_layer[pick] > 65)[0]                         # layers of 70 nodes: the pairs around and behind node 64
    for j, i in enumerate(wide):
        n_lo[i] = (63, 64, 66, 68, 62, 65)[j % 6]
    for l in sorted(set(pick.tolist())):
        sel = np.nonzero(pick == l)[0]
        px, py = lat.node_pos[off[l]:off[l + 1], 0], lat.node_pos[off[l]:off[l + 1], 1]
        # (where the nodes lie no more than 0.2 m apart -- lattice V: 0.1 m -- the 0.1 m offset would land on the NEXT boundary: 0.4 node
        # spacings there)
        big = 0.1 if lat.lat_resolution > 0.2 else 0.4 * lat.lat_resolution
        offsets = tuple(o if abs(o) < 0.1 else np.sign(o) * big for o in OFFSETS)
        p, _ = boundary_probes(px, py, n_lo[sel], n_lo[sel] + 1, rng.uniform(-0.3 * sp, 0.3 * sp, len(sel)), "node", offsets)
        for q in p:
            if sel[q["group"]] >= N_NODE_RAYS and q["kind"] != "tie":
                continue
            if int(tr.closest_layers(lat, q["x"], q["y"])[0][0]) == l:
                out.append(dict(q, layer=int(l), group=q["group"] + 1000 * int(l)))
        # beyond the first and the last node
        k = len(px)
        u = (np.array([px[-1], py[-1]]) - np.array([px[0], py[0]])) / max(np.hypot(px[-1] - px[0], py[-1] - py[0]), 1e-9)
        for n, s in ((0, -1.0), (k - 1, 1.0)):
            q = np.array([px[n], py[n]]) + s * u * 1.5
            if int(tr.closest_layers(lat, q[0], q[1])[0][0]) == l:
                out.append(dict(family="beyond", kind="plain", offset=0.0, pair=(n, n), group=-1, layer=int(l), x=float(q[0]), y=float(q[1])))
    for l in np.nonzero(reach & (lat.nodes_in_layer == 1))[0]:                  # the one-node layer
        for lateral in (-2.0, 0.0, 2.0):
            q = track_point(lat, int(l), lateral)
            if int(tr.closest_layers(lat, q[0], q[1])[0][0]) == l:
                out.append(dict(family="one-node", kind="plain", offset=0.0, pair=(0, 0), group=-1, layer=int(l), x=float(q[0]), y=float(q[1])))
    return out


def node_set(name):
    lat = lattice(name)
    cs = CaseSet(lat, name, "node")
    rng = np.random.default_rng(7500 + LATTICES.index(name))
    starts = {}
    for p in node_probes(name):
        key = (p["layer"], p["group"])
        if key not in starts:
            starts[key] = start_for(lat, p["layer"], rng)
        cs.add(scenario(lat, starts[key], [(0.3, one(p["x"], p["y"]))]), p)
    cs.pad()
    return cs


def template_set(name):
    lat = lattice(name)
    cs = CaseSet(lat, name, "template")
    t = mc.table(lat)
    valid = [int(s) for s in np.nonzero(t.H > 3)[0]]
    k = 0
    for action_sets in (True, False):
        for in_const in (False, True):
            for besides in (False, True):
                for la in LAST_ACTIONS:
                    for obj in (True, False):
                        for cc in (None, 0):
                            sl = valid[k % len(valid)]; k += 1
                            veh = [(0.5, one(*track_point(lat, sl + 2, 1.5)))] if obj else []
                            if cc is not None and not obj:
                                veh = [(0.5, one(*track_point(lat, sl + int(t.H[sl]) + 3, 0.0)))] if (not lat.closed and sl + t.H[sl] + 3 < lat.num_layers) or \
                                    (lat.closed and lat.num_layers - t.H[sl] - 4 >= 1) else []
                            row = (action_sets, in_const, besides, la, obj, cc is not None)
                            cs.add(scenario(lat, sl, veh, action_sets=action_sets, obj_in_const=in_const, obj_besides=besides, last_action=la,
                                            const_closest=cc), dict(family="template", kind="plain", offset=0.0, pair=(0, 0), group=k, row=row))
    return cs


def backoff_set(name):
    lat = lattice(name)
    cs = CaseSet(lat, name, "backoff")
    L, t = lat.num_layers, mc.table(lat)
    valid = [int(s) for s in np.nonzero(t.H > 4)[0]]
    starts = [("plain", valid[len(valid) // 4])]
    if lat.closed:
        starts.append(("seam", max(s for s in valid if s + t.H[s] >= L + 2 and s < L - 2)))
        starts.append(("seam-wall", L - 2))                                     # walls and objects on either side of the seam
    else:
        starts.append(("open-last", max(s for s in valid if lat.horizon_end_layer(s) == L - 1)))
    for what, sl in starts:
        H = int(t.H[sl])
        if H <= 4:
            continue
        for in_const in (False, True):
            for dname in WALL_D:
                d = {"1": 1, "2": 2, "3": 3, "H-1": H - 1, "H": H}[dname]
                wl = (sl + d) % L
                gids = [int(lat.layer_off[wl]) + n for n in range(int(lat.nodes_in_layer[wl]))]
                for rel in (-2, -1, 0, 1):
                    k = d + rel                                                  # the object's layer distance (-1: the layer behind the start)
                    ol = (sl + k) % L if lat.closed else sl + k
                    if not 0 <= ol < L or k > H + 1:
                        continue
                    for lateral in (1.0,):
                        veh = [(0.4, one(*track_point(lat, ol, lateral)))]
                        cs.add(scenario(lat, sl, veh, sn=int(lat.raceline_index[sl]), zone_gids=gids, obj_in_const=in_const),
                               dict(family="backoff", kind="plain", offset=0.0, pair=(wl, ol), group=sl, start=what, d=dname, rel=rel, in_const=in_const))
    cs.pad()
    return cs


_BUILDERS = {"layer": layer_set, "fullscan": fullscan_set, "gate": gate_set, "object": object_set, "node": node_set, "template": template_set,
             "backoff": backoff_set}


def set_names(name):
    return LAYER_SETS if name == "c3" else SET_NAMES


def case_set(name, which):
    """The set ``which`` of lattice ``name``: built once per process, shared and left unchanged."""
    if (name, which) not in _sets:
        _sets[(name, which)] = _BUILDERS[which](name)
    return _sets[(name, which)]


def describe(cs, p):
    """One line that names a probe."""
    extra = " ".join("%s=%s" % (k, p[k]) for k in ("partner", "n_pos", "team", "where", "nseg", "start", "rel", "what", "tied", "layer", "d", "in_const", "row") if k in p)
    return "%s/%s %s %s offset %+.0e pair %s scenario %d vehicle %d position %d %s" % (
        cs.name, cs.which, p["family"], p["kind"], p["offset"], p["pair"], p["scen"], p["veh"], p["pos"], extra)
