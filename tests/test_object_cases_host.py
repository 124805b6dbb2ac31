"""CPU: the probe sets of tests/object_cases.py are good inputs before any kernel sees them, and the two host forms of check_inside_bounds agree
on them.
  * the restatement and the oracle (oracle/ltpl_oracle.c through `oracle_process_objects`) give the same verdict on every probe, the `special`
    family (NaN, +-inf, +-1e300) included
  * the generators reproduce the stored probes of tests/golden/objects_boundary.npz bit for bit, and both forms reproduce the verdicts the
    UNMODIFIED reference gave on them (oracle/gen_golden_objects.py boundary) -- but for exact ties of the squared distance, among the centre
    points or among the 50 linspace points, where the project's contract is the FIRST minimum and the reference's np.argpartition takes another
    of the tied points: `REFERENCE_OFF_FIRST_MINIMUM` verdicts (numpy as recorded in the fixture), every one of them at the switch of the
    linspace index 47 -> 48 bisected to adjacent doubles, where d2[47] == d2[48] exactly and the reference takes point 48. There the oracle is
    the measure.
  * every boundary pair is observable: across the two adjacent doubles the verdict differs (bound, index), the closest centre point differs
    (centre: in the middle of a segment both closest points choose that segment, the verdict cannot show the switch)
  * every family is populated on every lattice (the `tie` family: the oval only), the tie loci of Monteblanco and Millbrook are at least as many
    as the (layer, side) pairs at which a restatement with a forced segment choice gave two verdicts: 46 of 256 and 23 of 74
  * `segment` probes: of the 21 offsets of a locus at most the three innermost (0, +-1e-13 m) are undecided -- a displacement d at lateral
    distance r changes the margin by about 2 d / r, 1e-9 m at 5 m already 4e-10 rad -- which is at most 1 / 6 of the family with room to spare.
"""
import numpy as np
import pytest

import object_cases as oc

MIN_LOCI = {"monteblanco": 46, "millbrook": 23}
MIN_RAYS = {"monteblanco": 400, "millbrook": 400, "open": 386, "c3": 200}          # open: the other rays start beyond the track's end
REFERENCE_OFF_FIRST_MINIMUM = {"monteblanco": 12, "millbrook": 3, "open": 6, "c3": 0}

_oracles = {}


def oracle_verdict(ps):
    from oracle.oracle_lib import OracleBackend
    if ps.name not in _oracles:
        _oracles[ps.name] = OracleBackend(ps.lat)
    p = ps.probes
    out = _oracles[ps.name].process_objects(p.qx, p.qy, np.zeros(p.m), np.zeros(p.m), np.full(p.m, 4.0))
    return out["on_track"].astype(bool)


@pytest.mark.parametrize("name", oc.LATTICES)
def test_restatement_oracle_and_reference_agree(name):
    ps = oc.probe_set(name)
    p, r = ps.probes, ps.ref
    assert p.m <= 20000
    v = oracle_verdict(ps)
    bad = np.nonzero(v != r.verdict)[0]
    assert not len(bad), "restatement vs oracle: %d of %d differ, first: %s" % (len(bad), p.m, oc.describe(ps, bad[0]))
    # the stored probes are the generators' output
    stored, gv = oc.fixture(name)
    n = int(oc.in_fixture(ps).sum())
    assert stored.m == n and np.all(oc.in_fixture(ps)[:n]), "%s: the generators have drifted from tests/golden/objects_boundary.npz" % name
    for f in oc.Probes.FIELDS:
        assert np.array_equal(getattr(stored, f), getattr(p, f)[:n]), "%s: %s has drifted from tests/golden/objects_boundary.npz" % (name, f)
    fs = oc.fixture_set(name)
    assert np.array_equal(fs.probes.qx, p.qx, equal_nan=True) and np.array_equal(fs.probes.qy, p.qy, equal_nan=True)
    assert np.array_equal(fs.ref.verdict, r.verdict) and np.array_equal(fs.ref.decided, r.decided)
    # ... and the unmodified reference's verdicts are the oracle's, exact ties apart
    differ = gv != v[:n]
    bad = np.nonzero(differ & ~r.tie[:n])[0]
    assert not len(bad), "reference vs oracle: %d of %d differ off the exact ties, first: %s" % (len(bad), n, oc.describe(ps, bad[0]))
    print("%s: %d probes, %d exact ties (%d among the centre points, %d among the linspace points); the reference (numpy %s) off the first "
          "minimum's verdict in %d" % (name, p.m, int(r.tie.sum()), int((r.n_min > 1).sum()), int((r.n_min50 > 1).sum()), oc.fixture("numpy"),
                                     int(differ.sum())))
    assert int(differ.sum()) == REFERENCE_OFF_FIRST_MINIMUM[name]
    on = np.nonzero(differ)[0]
    assert np.all(p.family[on] == oc.FAMILIES.index("index")) and np.all(r.bi[on] == 47) and np.all(r.n_min50[on] == 2)


@pytest.mark.parametrize("name", oc.LATTICES)
def test_probe_sets_meet_their_conditions(name):
    ps = oc.probe_set(name)
    p, r = ps.probes, ps.ref
    fam = {f: p.family == i for i, f in enumerate(oc.FAMILIES)}
    for f in oc.FAMILIES:
        n = int(fam[f].sum())
        print("%-12s %-9s %6d probes, %6d on the track, %6d decided" % (name, f, n, int((r.verdict & fam[f]).sum()), int((r.decided & fam[f]).sum())))
        assert n > 0 or (f == "tie" and name != "c3"), (name, f)
    # every boundary pair is observable
    first = np.nonzero((p.pair >= 0) & (p.pair > np.arange(p.m)))[0]
    second = p.pair[first]
    assert np.all(p.pair[second] == first) and np.all(p.family[first] == p.family[second])
    by_verdict = fam["bound"][first] | fam["index"][first]
    swapped = r.verdict[first] != r.verdict[second]
    assert np.all(swapped[by_verdict]), "%s: %d pairs whose verdicts do not differ" % (name, int((~swapped[by_verdict]).sum()))
    cen = fam["centre"][first]
    assert np.all(r.nb[first[cen]] == p.k[first[cen]]) and np.all(r.nb[second[cen]] == (p.k[first[cen]] + 1) % ps.track.L)
    assert np.all(fam["bound"][first] | fam["index"][first] | cen)
    # populated as measured
    assert ps.counts["bound"] >= MIN_RAYS[name] and int((fam["bound"][first]).sum()) == ps.counts["bound"], ps.counts
    assert {0, 48} <= ps.index_seen, ps.index_seen                # the switches 0 / 1 and 48 / 49
    if name != "c3":                                              # (one width all round the oval: no index gives another verdict than the next)
        assert ps.counts["index"] >= 40 and {0, 48} <= set(p.param[first[fam["index"][first]]].astype(int).tolist())
    assert ps.counts["centre"] >= 40
    assert {0, ps.track.L - 1} <= set(r.nb[fam["centre"]].tolist())             # the switch L - 1 -> 0 included
    if name in MIN_LOCI:
        assert ps.counts["segment"] >= MIN_LOCI[name], ps.counts
        w = ps.band_widths
        print("%s: %d tie loci with a band, widths %.3g .. %.3g m, median %.3g m" % (name, len(w), w.min(), w.max(), np.median(w)))
        seam = fam["segment"] & ((p.k == 0) | (p.k == ps.track.L - 1))
        assert seam.any(), "%s: no tie locus across the seam" % name
    if name == "c3":
        assert int((r.n_min[fam["tie"]] > 1).sum()) == int(fam["tie"].sum()) >= 100
    # the tie loci: undecided only at the three innermost offsets
    seg = fam["segment"]
    und = seg & ~r.decided
    assert set(np.abs(p.offset[und]).tolist()) <= {0.0, 1e-13}, name
    assert int(und.sum()) * 6 <= int(seg.sum())
    starts = np.nonzero(seg & (p.offset == 0.0))[0]
    for s in starts:
        assert int(und[s:s + len(oc.OFFSETS)].sum()) <= 3
    bands = seg & (r.v_forced[0] != r.v_forced[1])
    print("%s: %d segment probes, %d undecided, %d at which the forced verdicts differ" % (name, int(seg.sum()), int(und.sum()), int(bands.sum())))
    # on-point: atan2(0, 0) enters; an object exactly on an interpolated bound point is on the track
    onp = np.nonzero(fam["on-point"])[0]
    centre = onp[p.param[onp] == 0.0]
    assert len(centre) >= 3 and np.all(r.nb[centre] == p.k[centre]) and np.all(ps.track.cx[p.k[centre]] == p.qx[centre]) and r.verdict[centre].all()
    interp = onp[p.param[onp] >= 100.0]
    assert len(interp) >= 30 and r.verdict[interp].mean() > 0.9
    # special: arithmetic only
    sp = np.nonzero(fam["special"])[0]
    assert np.all(r.nb[sp] == 0) and np.all(r.bi[sp] == 0)
    nan = np.isnan(p.qx[sp]) | np.isnan(p.qy[sp])
    assert np.array_equal(r.verdict[sp], nan)
