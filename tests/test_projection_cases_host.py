"""CPU: the probe sets of tests/projection_cases.py are good inputs before any kernel sees them, and the forms of the projection that run on the
host satisfy on them what tests/test_gpu_projection.py asks of the device forms.
  * the conditions on the sets: every probe displaced by 1e-9 m or more is decided, undecided probes occur at o = 0 and +-1e-13 only, at
    least 90 % of each family is decided (exact d2 ties and the reference's own NaN are classes of their own and counted apart)
  * the restatement and the oracle's get_s_coord (oracle/ltpl_oracle.c through `oracle_get_s_coord`) agree bit for bit on every probe
  * both agree with the unmodified reference (tests/golden/projection_probes.npz, oracle/gen_golden_projection.py) on everything but exact d2
    ties; there the reference's closest point is one of the tied points and the oracle's is the first
  * project_on_polyline of csrc/planner_core.hpp and of csrc/fleet_core.hpp (oracle/planner_host_shim.cpp): the oracle's index pair and its s
    within the bound of tests/test_gpu_projection.py on decided probes, one forced order on undecided ones, the first minimum on exact ties.

Before the clamp rule of fleet_core.hpp (a neighbour that the index clamp puts onto the closest point never wins) its form failed here without
a GPU: on the first planned Monteblanco path alone 27 of 2 798 probes, all of the families behind / beyond -- s = NaN for collinear queries
(o = 0, +-1e-13 m) and still at o = -1e-9 m 17.3 segment lengths behind the start, the degenerate index pair (0, 0) up to o = +-1e-6 m."""
import os
import zlib

import numpy as np
import pytest

import projection_cases as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "projection_probes.npz")
_golden = {}


def golden(name):
    """(s, index pair) of the unmodified reference for the probe set of line ``name``."""
    if not _golden:
        z = np.load(GOLDEN)
        off = np.concatenate(([0], np.cumsum(z["counts"])))
        for i, nm in enumerate(z["names"].tolist()):
            _golden[nm] = (z["s"][off[i]:off[i + 1]], z["pair"][off[i]:off[i + 1]].astype(np.int64), int(z["counts"][i]), int(z["crcs"][i]))
        _golden["numpy"] = str(z["numpy_version"])
    return _golden[name]


def same_bits(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def test_probe_sets_meet_their_conditions():
    fam_total, fam_decided = np.zeros(len(pc.FAMILIES), np.int64), np.zeros(len(pc.FAMILIES), np.int64)
    n_tie = n_nan = n_und = n_all = 0
    smallest = np.inf
    for name in pc.LINE_NAMES:
        ps = pc.probe_set(name)
        p, r = ps.probes, ps.ref
        plain = ~r.tie & ~r.nan
        und = plain & ~r.decided
        far = np.abs(p.offset) >= 1e-9
        assert not np.any(und & far), "%s: undecided at %s" % (name, [pc.describe(ps, i) for i in np.nonzero(und & far)[0][:5]])
        assert set(np.abs(p.offset[und]).tolist()) <= {0.0, 1e-13}, name
        # NaN in the reference itself: only a query collinear beyond the end of an open line (0 / 0), or an exact tie that puts nb there
        assert np.all(~r.nan | (~ps.line.closed & (r.idx2 == r.nb))), name
        sel = far & plain & ~r.clamped & ~r.twin
        if sel.any():
            smallest = min(smallest, float(r.margin[sel].min()))
        np.add.at(fam_total, p.family[plain], 1)
        np.add.at(fam_decided, p.family[plain & r.decided], 1)
        n_tie += int(r.tie.sum()); n_nan += int((r.nan & ~r.tie).sum()); n_und += int(und.sum()); n_all += p.m
        if not ps.line.closed and not name.startswith("grid"):   # the end families sit where they are meant to: nb = 0 / n - 1, one neighbour clamped
            for fam, end in ((0, 0), (1, ps.line.n - 1)):
                f = p.family == fam
                assert f.sum() == len(pc.T_BEHIND) * len(pc.OFFSETS) and np.all(r.nb[f] == end) and r.clamped[f].all(), (name, fam)
        if "raceline" in name:
            assert ps.n_loci >= 150, (name, ps.n_loci)
            seam = (p.family == 2) & ((p.k == 0) | (p.k == ps.line.n - 1))
            assert int(seam.sum()) >= 100, (name, "bisector loci across the seam")
    print("%d probes on %d polylines: %d exact d2 ties, %d NaN in the reference, %d undecided; smallest margin at |o| >= 1e-9: %.2e rad" % (
        n_all, len(pc.LINE_NAMES), n_tie, n_nan, n_und, smallest))
    for f, fam in enumerate(pc.FAMILIES):
        if fam == "tie":
            assert fam_total[f] == 0                             # (every probe of the grid family is an exact tie: the class of its own)
            continue
        share = fam_decided[f] / fam_total[f]
        print("  %-12s %6d probes, %.3f decided" % (fam, fam_total[f], share))
        assert fam_total[f] >= 100 and share >= 0.9, (fam, fam_total[f], share)
    assert n_tie >= 800 and n_nan >= 20 and n_und >= 500
    assert smallest > pc.MARGIN
    # the chunk edges of the device's closest-point scans occur as nb
    for name, ks in (("synthetic-open-513", (62, 63, 64, 65, 254, 255, 256, 257, 511, 512)), ("monteblanco-raceline", (0, 63, 64, 255, 256, 794))):
        assert set(ks) <= set(pc.probe_set(name).ref.nb.tolist()), name


@pytest.mark.parametrize("name", pc.LINE_NAMES)
def test_restatement_oracle_and_reference_agree(name):
    from oracle import oracle_lib
    ps = pc.probe_set(name)
    line, p, r = ps.line, ps.probes, ps.ref
    s, pair = oracle_lib.get_s_coord(line.x, line.y, line.s, line.closed, p.qx, p.qy)
    bad = np.nonzero(~same_bits(s, r.s) | np.any(pair != r.pair, axis=1))[0]
    assert not len(bad), "restatement vs oracle: %d of %d differ, first: %s (oracle %r %s, restated %r %s)" % (
        len(bad), p.m, pc.describe(ps, bad[0]), s[bad[0]], pair[bad[0]], r.s[bad[0]], r.pair[bad[0]])
    gs, gpair, count, crc = golden(name)
    assert count == p.m and crc == zlib.crc32(p.qx.tobytes() + p.qy.tobytes()), "%s: the generators have drifted from tests/golden/projection_probes.npz" % name
    gpair = gpair % line.n                                       # (Python's idx1 = -1 on a closed line)
    differ = ~same_bits(gs, s) | np.any(gpair != pair, axis=1)
    bad = np.nonzero(differ & ~r.tie)[0]
    assert not len(bad), "reference vs oracle: %d of %d differ off the exact ties, first: %s" % (len(bad), p.m, pc.describe(ps, bad[0]))
    # exact ties: the reference's closest point (np.argpartition, numpy as recorded) is one of the tied points, the oracle's is the first of them
    for i in np.nonzero(r.tie)[0]:
        dx, dy = line.x - p.qx[i], line.y - p.qy[i]
        d2 = dx * dx + dy * dy
        tied = np.nonzero(d2 == d2.min())[0]
        assert r.nb[i] == tied[0] and r.nb[i] in pair[i]
        assert np.intersect1d(gpair[i], tied).size >= 1, pc.describe(ps, i)
    if r.tie.any():
        print("%s: %d exact ties, the reference (numpy %s) off the first minimum in %d" % (name, int(r.tie.sum()), golden("numpy"), int((differ & r.tie).sum())))


def check_form(ps, what, s, pair, with_s=True, device_atan2=False):
    """What both test modules ask of a form's (s, index pair) on a probe set; ``pair`` columns that a form does not produce hold -1. Decided
    probes -- by the margin, by a clamped neighbour or by twin neighbours alike -- must have the oracle's indices and its s within the bound.
    ``device_atan2`` (only the fleet_core form ON THE DEVICE, which calls the device's atan2 at a clamped start): where the clamp alone decides
    and the margin is below MARGIN, `>` and `>=` part only if the other angle is exactly 0 too -- the last bit of an atan2, and the device's
    is not the host's (measured: tests/test_gpu_projection.py) -- so there s must be the oracle's and the index pair that of a forced order
    on the oracle's segment. Returns the worst s error on decided probes as a multiple of the bound's unit (ulp of |s| + |q - a|)."""
    p, r = ps.probes, ps.ref
    have = pair >= 0
    with np.errstate(invalid="ignore"):
        bound = pc.s_bound(ps)
        has_s = np.full(p.m, bool(with_s))
        err = np.abs(s - r.s)
        ok_pair = np.all(~have | (pair == r.pair), axis=1)
        ok_s = ~has_s | (err <= bound)
        forced_ok = np.zeros((3, p.m), bool)
        for o in range(3):
            forced_ok[o] = np.all(~have | (pair == r.pair_forced[o]), axis=1) & (~has_s | same_bits(s, r.s_forced[o]) | (np.abs(s - r.s_forced[o]) <= bound))
        ok = np.where(r.decided, ok_pair & ok_s, forced_ok.any(axis=0))
        if device_atan2:
            last_bit = r.decided & r.clamped & ~r.twin & ~(r.margin > pc.MARGIN)
            same_segment = np.stack([(r.order > 0) == (o == 2) for o in range(3)])
            check_form.last_bit_pairs = getattr(check_form, "last_bit_pairs", 0) + int((last_bit & ~ok_pair).sum())
            ok = np.where(last_bit, ok_s & np.any(forced_ok & same_segment, axis=0), ok)
        # exact d2 ties: the first minimum (then whatever the angles say: one forced order)
        ok = np.where(r.tie, forced_ok.any(axis=0), ok)
        ok |= r.nan & ~r.tie                                    # the reference's own 0 / 0: nothing is asserted
    bad = np.nonzero(~ok)[0]
    lines_ = ["%s: got s %r pair %s, oracle s %r pair %s (%s, margin %.1e)" % (
        pc.describe(ps, i), s[i], pair[i].tolist(), r.s[i], r.pair[i].tolist(),
        "tie" if r.tie[i] else "decided" if r.decided[i] else "undecided", float(r.margin[i])) for i in bad[:12]]
    assert not len(bad), "%s: %d of %d probes fail\n%s" % (what, len(bad), p.m, "\n".join(lines_))
    sel = r.decided & has_s & ~r.nan & (bound > 0.0)
    return float(np.max(err[sel] / (bound[sel] / pc.S_ULPS))) if sel.any() else 0.0


@pytest.mark.parametrize("form", ("planner_core", "fleet_core"))
def test_host_forms_take_the_reference_branch(form):
    from oracle import oracle_lib
    worst = 0.0
    for name in pc.LINE_NAMES:
        ps = pc.probe_set(name)
        line, p = ps.line, ps.probes
        s, pair = oracle_lib.project_host(form, line.x, line.y, line.s, line.closed, p.qx, p.qy)
        pair = pair.astype(np.int64) % line.n                    # (both forms return Python's idx1 = -1 on a closed line)
        worst = max(worst, check_form(ps, "%s on %s" % (form, name), s, pair))
    print("%s: worst |s - s_oracle| on decided probes: %.2f ulp of |s| + |q - a|" % (form, worst))
