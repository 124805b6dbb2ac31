"""Long-double reference of the path assembly (everything behind the node list: csrc/paths_team.hpp `team_assemble_rest`, the oracle's
gather + calc_splines_open + re-sampling) and the comparison against it. NumPy only, written from the mathematics:

  knots     k_0 .. k_N: the first sample of every path edge, plus the last sample of the last edge
  h_i       edge_len of edge i (the parameter length of segment i)
  end slopes  s_0 = (cos(psi_0 + pi/2), sin(psi_0 + pi/2)), s_N likewise with the heading of the last sample; psi_0 is the heading of the
            first sample, or the scenario's psi_s
  slopes m_i  of the clamped C2 cubic spline in the cumulated parameter: m_0 = s_0, m_N = s_N and, for i = 1 .. N-1,
                m_{i-1} / h_{i-1} + 2 (1 / h_{i-1} + 1 / h_i) m_i + m_{i+1} / h_i = 3 ((k_i - k_{i-1}) / h_{i-1}^2 + (k_{i+1} - k_i) / h_i^2)
            (continuity of the second derivative at the inner knots), solved by plain elimination
  segment i, t in [0, 1]:  a0 = k_i, a1 = m_i h_i, a2 = 3 (k_{i+1} - k_i) - 2 m_i h_i - m_{i+1} h_i, a3 = -2 (k_{i+1} - k_i) + m_i h_i + m_{i+1} h_i
  node_idx  every edge but the last contributes samples - 1 rows, the last one all of its rows
  rows      n_i = idx[i+1] - idx[i] + 1, t = k / (n_i - 1) (t = 1 for the last point of the path);
            psi = atan2(y', x') - pi/2 (normalised), kappa = (x' y'' - y' x'') / |r'|^3
  column 4  the lattice's own sample length: a copy
"""
import numpy as np

from graphbasedlocaltrajectoryplanner_amd.tick_replay import KAPPA_FLOOR

LD = np.longdouble

# THE bound of every comparison against `reference_assembly`: coefficients, xy, psi (radians) and kappa, each against the scale
# tick_replay.py defines for it (a0 / xy: the path's extent, at least 1 m; a1 / a2 / a3: the largest magnitude of that order, at least
# 1e-3; kappa: max |kappa|, at least KAPPA_FLOOR; psi: the angle difference modulo 2 pi).
# Derivation. The bound is measured against the long-double reference, never against the kernel. The oracle (fp64, dense LU over the
# 4 N x 4 N system) deviates from this reference, on the scenario sets of tests/assembly_cases.py, by at most
#     coefficients 1.1e-12    kappa 1.2e-12    xy 4.3e-15    psi 1.1e-15 rad
# (CPU; tests/test_spline_ref_host.py prints the values it finds). 100 x the largest of these, rounded, is 1e-10. The two orders of
# margin cover what legitimately differs in the kernel: Newton reciprocals (~1 ulp) instead of divisions, log2(N) rounds of cyclic
# reduction instead of one elimination, fma contraction inside the polynomial evaluation. The kernel's own measured deviation is in
# DESIGN.md section 2; it does not move this number.
ASSEMBLY_TOL = 1e-10


class Assembly(object):
    """One assembled path: node_idx (int), coeff (N, 8), path_param (n_pts, 5)."""

    def __init__(self, node_idx, coeff, path_param):
        self.node_idx, self.coeff, self.path_param = node_idx, coeff, path_param
        self.n_pts = int(path_param.shape[0])


def path_edges(lat, start_layer, nodes):
    """Edge ids of the path that starts on ``start_layer`` and visits ``nodes`` (one node per consecutive layer)."""
    L = lat.num_layers
    out = []
    for i in range(len(nodes) - 1):
        e = lat.find_edge((start_layer + i) % L, int(nodes[i]), (start_layer + i + 1) % L, int(nodes[i + 1]))
        assert e >= 0, "no edge (%d, %d) -> (%d, %d)" % ((start_layer + i) % L, nodes[i], (start_layer + i + 1) % L, nodes[i + 1])
        out.append(e)
    return out


def in_edge_ranks(lat, start_layer, nodes):
    """Rank of every path edge among the in-edges of its destination node (sorted by source)."""
    L = lat.num_layers
    edges = path_edges(lat, start_layer, nodes)
    return [e - int(lat.in_ptr[int(lat.layer_off[(start_layer + i + 1) % L]) + int(nodes[i + 1])]) for i, e in enumerate(edges)]


def clamped_slopes(knots, h, s0, sN):
    """Knot slopes (N + 1, 2) of the clamped C2 cubic spline through ``knots`` (N + 1, 2) with segment parameters ``h`` (N) and end slopes
    ``s0``, ``sN``: forward elimination and back substitution of the tridiagonal system, in long double."""
    knots, h = np.asarray(knots, LD), np.asarray(h, LD)
    N = h.shape[0]
    m = np.zeros((N + 1, 2), LD)
    m[0], m[N] = s0, sN
    if N < 2:
        return m
    one, two, three = LD(1), LD(2), LD(3)
    a = one / h[:-1]                 # sub-diagonal of rows 1 .. N-1: 1 / h_{i-1}
    c = one / h[1:]                  # super-diagonal: 1 / h_i
    b = two * (a + c)
    d = three * ((knots[1:N] - knots[0:N - 1]) * (a * a)[:, None] + (knots[2:N + 1] - knots[1:N]) * (c * c)[:, None])
    d[0] -= a[0] * m[0]
    d[-1] -= c[-1] * m[N]
    n = N - 1
    cp, dp = np.zeros(n, LD), np.zeros((n, 2), LD)
    cp[0], dp[0] = c[0] / b[0], d[0] / b[0]
    for i in range(1, n):
        den = b[i] - a[i] * cp[i - 1]
        cp[i] = c[i] / den
        dp[i] = (d[i] - a[i] * dp[i - 1]) / den
    x = np.zeros((n, 2), LD)
    x[n - 1] = dp[n - 1]
    for i in range(n - 2, -1, -1):
        x[i] = dp[i] - cp[i] * x[i + 1]
    m[1:N] = x
    return m


def segment_coefficients(knots, h, m):
    """Rows [a0 a1 a2 a3]x, [..]y per segment, t in [0, 1]."""
    knots, h, m = np.asarray(knots, LD), np.asarray(h, LD), np.asarray(m, LD)
    N = h.shape[0]
    coeff = np.zeros((N, 8), LD)
    for ax in range(2):
        T0, T1, dl = m[:N, ax] * h, m[1:, ax] * h, knots[1:, ax] - knots[:N, ax]
        coeff[:, 4 * ax + 0] = knots[:N, ax]
        coeff[:, 4 * ax + 1] = T0
        coeff[:, 4 * ax + 2] = LD(3) * dl - LD(2) * T0 - T1
        coeff[:, 4 * ax + 3] = -LD(2) * dl + T0 + T1
    return coeff


def evaluate_rows(coeff, node_idx, t_of=None):
    """x, y, psi, kappa (n_pts, 4) of the re-sampled path; ``t_of(k, n_i)`` overrides the sampling parameter (sensitivity tests)."""
    pi = np.arctan2(LD(0), LD(-1))
    N = coeff.shape[0]
    n_pts = int(node_idx[N]) + 1
    out = np.zeros((n_pts, 4), LD)
    for i in range(N):
        n_i = int(node_idx[i + 1]) - int(node_idx[i]) + 1
        cnt = n_i if i == N - 1 else n_i - 1
        k = np.arange(cnt)
        t = (k.astype(LD) / LD(n_i - 1)) if t_of is None else np.asarray([t_of(int(q), n_i) for q in k], LD)
        if t_of is None and cnt == n_i:
            t[-1] = LD(1)
        cx, cy = coeff[i, 0:4], coeff[i, 4:8]
        x = cx[0] + t * (cx[1] + t * (cx[2] + t * cx[3]))
        y = cy[0] + t * (cy[1] + t * (cy[2] + t * cy[3]))
        xd = cx[1] + t * (LD(2) * cx[2] + t * LD(3) * cx[3])
        yd = cy[1] + t * (LD(2) * cy[2] + t * LD(3) * cy[3])
        xdd = LD(2) * cx[2] + LD(6) * cx[3] * t
        ydd = LD(2) * cy[2] + LD(6) * cy[3] * t
        psi = np.arctan2(yd, xd) - pi / LD(2)
        psi = np.where(psi < -pi, psi + LD(2) * pi, psi)
        q = xd * xd + yd * yd
        r0 = int(node_idx[i])
        out[r0:r0 + cnt, 0], out[r0:r0 + cnt, 1], out[r0:r0 + cnt, 2] = x, y, psi
        out[r0:r0 + cnt, 3] = (xd * ydd - yd * xdd) / (q * np.sqrt(q))
    return out


def reference_assembly(lat, start_layer, nodes, psi_s=None):
    """The assembled path of ``nodes`` from ``start_layer`` in np.longdouble, from the Lattice arrays alone."""
    edges = path_edges(lat, start_layer, nodes)
    N = len(edges)
    assert N >= 1
    k0 = [int(lat.samp_ptr[e]) for e in edges]
    k1 = [int(lat.samp_ptr[e + 1]) for e in edges]
    knots = np.zeros((N + 1, 2), LD)
    for i in range(N):
        knots[i] = lat.samples[k0[i], 0:2]
    knots[N] = lat.samples[k1[-1] - 1, 0:2]
    h = np.asarray([lat.edge_len[e] for e in edges], LD)
    pi = np.arctan2(LD(0), LD(-1))
    psi0 = LD(lat.samples[k0[0], 2]) if psi_s is None else LD(psi_s)
    psiN = LD(lat.samples[k1[-1] - 1, 2])
    s0 = np.asarray([np.cos(psi0 + pi / LD(2)), np.sin(psi0 + pi / LD(2))], LD)
    sN = np.asarray([np.cos(psiN + pi / LD(2)), np.sin(psiN + pi / LD(2))], LD)
    m = clamped_slopes(knots, h, s0, sN)
    coeff = segment_coefficients(knots, h, m)
    node_idx = np.zeros(N + 1, np.int64)
    el = []
    for i in range(N):
        take = (k1[i] - k0[i]) if i == N - 1 else (k1[i] - k0[i] - 1)
        node_idx[i + 1] = node_idx[i] + take
        el.append(lat.samples[k0[i]:k0[i] + take, 4])
    node_idx[N] -= 1
    pp = np.zeros((int(node_idx[N]) + 1, 5), LD)
    pp[:, 0:4] = evaluate_rows(coeff, node_idx)
    pp[:, 4] = np.concatenate(el)
    return Assembly(node_idx, coeff, pp)


def assembly_deviation(coeff, path_param, ref):
    """{quantity: largest deviation from ``ref`` relative to the quantity's scale (psi: radians)} of one path; the scales are those of
    tick_replay.assert_coeff_close / assert_xy_close / assert_close_rel(floor=KAPPA_FLOOR), taken on the reference."""
    coeff, pp = np.asarray(coeff, LD), np.asarray(path_param, LD)
    assert coeff.shape == ref.coeff.shape and pp.shape[0] == ref.n_pts, (coeff.shape, ref.coeff.shape, pp.shape, ref.n_pts)
    dev = {}
    worst = LD(0)
    for c in (0, 4):                                               # a0 against the extent of the knots, per axis
        scale = max(LD(np.ptp(ref.coeff[:, c])), LD(1))
        worst = max(worst, np.max(np.abs(coeff[:, c] - ref.coeff[:, c])) / scale)
    for order in (1, 2, 3):
        cols = [order, 4 + order]
        scale = max(np.max(np.abs(ref.coeff[:, cols])), LD(1e-3))
        worst = max(worst, np.max(np.abs(coeff[:, cols] - ref.coeff[:, cols])) / scale)
    dev["coeff"] = float(worst)
    worst = LD(0)
    for c in (0, 1):
        scale = max(LD(np.ptp(ref.path_param[:, c])), LD(1))
        worst = max(worst, np.max(np.abs(pp[:, c] - ref.path_param[:, c])) / scale)
    dev["xy"] = float(worst)
    pi = np.arctan2(LD(0), LD(-1))
    dpsi = np.abs(np.mod(pp[:, 2] - ref.path_param[:, 2] + pi, LD(2) * pi) - pi)
    dev["psi"] = float(np.max(dpsi))
    scale = max(np.max(np.abs(ref.path_param[:, 3])), LD(KAPPA_FLOOR))
    dev["kappa"] = float(np.max(np.abs(pp[:, 3] - ref.path_param[:, 3])) / scale)
    return dev


def assert_assembly_close(actual, ref, bound=ASSEMBLY_TOL, what=""):
    """``actual`` = (coeff (N, 8), path_param (n_pts, 5)) of one path against ``ref`` (an Assembly): every quantity within ``bound`` of its
    scale, the element-length column bit-exact. Returns the deviations (for the tables of DESIGN.md section 2)."""
    coeff, pp = actual
    dev = assembly_deviation(coeff, pp, ref)
    bad = {k: v for k, v in dev.items() if not v <= bound}
    assert not bad, "%s: %s beyond %.1e of the long-double reference (all: %s)" % (
        what, ", ".join("%s %.3e" % kv for kv in sorted(bad.items())), bound, ", ".join("%s %.3e" % kv for kv in sorted(dev.items())))
    assert np.array_equal(np.asarray(pp)[:, 4], ref.path_param[:, 4].astype(np.float64)), "%s: element-length column must be a copy" % what
    return dev


def merge_worst(worst, dev):
    for k, v in dev.items():
        worst[k] = max(worst.get(k, 0.0), v)
    return worst
