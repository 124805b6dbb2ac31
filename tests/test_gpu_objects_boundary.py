"""
GPU: object ingestion on the device (process_object_dev of csrc/ltpl_hip.hip: the body of k_process_objects / ltpl_process_objects and, inlined,
of the simulation's k_fleet_sim_step) at its decision boundaries, on the probes of tests/object_cases.py (the stored ones of
tests/golden/objects_boundary.npz -- tests/test_object_cases_host.py shows on the CPU that they are the generators' output -- and the
`special` family), against the oracle's plain C and the verdicts of the unmodified reference.

  every probe   one call per lattice (Monteblanco, Millbrook, the open track, the C3 oval). `on_track` is the oracle's bit for bit on every
                decided probe, and the fixture's wherever the fixture and the oracle agree (they part on exact ties of the squared distance
                only, where the first minimum is the contract and the oracle the measure: tests/test_object_cases_host.py counts them). On an
                undecided `segment` probe -- on the tie locus |ang1| == |ang2| within 1e-12 rad, where the device's atan2 against libm's
                decides -- it is one of the two forced verdicts. radius: the oracle's bits; pred_x / pred_y: within `pred_bound`.
  call sizes    1, 63, 64, 65 and 129 objects cut from the probe list: the same bits as the same rows of the full call
  prediction    px - sin(theta) v dt, py + cos(theta) v dt against the same expression in np.longdouble: theta over [-pi, pi], the multiples
                of pi / 2 and their adjacent doubles, |theta| up to 1e6, v from 0 to 80 m/s. The bound is measured, not chosen: the device's
                largest deviation must not exceed 4 x the oracle's (libm's) largest deviation from the same long-double values, nor one ulp
                of |pred| + 8 eps v dt (sin and cos within 2 ulp each on either side, two roundings of the product, one of the sum),
                whichever is larger.
                MEASURED on an MI355X (21 408 inputs, 63-bit long double): device 3.123e-14 m, oracle 3.123e-14 m.
  simulation    two planners whose statics lie on `bound` pairs and beside `segment` loci (decided, 1e-9 m either side, inside the band in
                which the two segments give different verdicts), alternating inside and outside: one with 26 statics, one with 70 so that
                the survivors straddle lane 64; every third has v > 0. Three ticks in lockstep with the host loop of tests/sim_loop.py (the
                harness of tests/test_gpu_sim_differential.py: kept count, first survivor, paths and trajectories), the kept count = the
                number of inside probes, and the device's digests against the free-running host loop's. Mates are not separately driven:
                their inputs are tracked state, and the race tests cover that call site.
"""
import os

import numpy as np
import pytest

import object_cases as oc
from test_object_cases_host import REFERENCE_OFF_FIRST_MINIMUM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
DT = 0.2
CALL_SIZES = (1, 63, 64, 65, 129)


@pytest.fixture(scope="module")
def backends():
    """name -> (HipBackend, OracleBackend) of the lattices beyond the session's fixtures, made on first use and closed with the module."""
    from graphbasedlocaltrajectoryplanner_amd import _capi
    from oracle.oracle_lib import OracleBackend
    made = {}

    def get(name):
        if name not in made:
            made[name] = (_capi.HipBackend(oc.lattice(name)), OracleBackend(oc.lattice(name)))
        return made[name]
    yield get
    for hip, _ in made.values():
        hip.close()


def inputs(ps, seed):
    """theta, v, length per probe (seeded): the prediction and the radius ride along with every probe."""
    rng = np.random.default_rng(seed)
    m = ps.probes.m
    return rng.uniform(-np.pi, np.pi, m), np.where(rng.random(m) < 0.2, 0.0, rng.uniform(0.0, 80.0, m)), rng.uniform(3.0, 6.0, m)


def ulp(x):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.spacing(np.abs(np.asarray(x, np.float64)))


def pred_bound(pred, v, dt=DT):
    """One ulp of |pred| + 8 eps v dt."""
    with np.errstate(invalid="ignore", over="ignore"):
        return ulp(pred) + 8.0 * EPS * np.abs(v) * dt


def same_or_within(a, b, bound):
    with np.errstate(invalid="ignore", over="ignore"):
        return (a == b) | (np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= bound)


_full = {}


def full_call(backends, name):
    """The whole probe list of lattice ``name`` through both forms, once per module."""
    if name not in _full:
        ps = oc.fixture_set(name)
        hip, orc = backends(name)
        th, v, ln = inputs(ps, 40 + oc.LATTICES.index(name))
        p = ps.probes
        _full[name] = (ps, (th, v, ln), hip.process_objects(p.qx, p.qy, th, v, ln), orc.process_objects(p.qx, p.qy, th, v, ln))
    return _full[name]


@pytest.mark.parametrize("name", oc.LATTICES)
def test_every_probe_of_every_lattice(backends, name):
    ps, (th, v, ln), dev, ref = full_call(backends, name)
    p, r = ps.probes, ps.ref
    d_on, o_on = dev["on_track"].astype(bool), ref["on_track"].astype(bool)
    assert set(np.unique(dev["on_track"]).tolist()) <= {0, 1}
    assert np.array_equal(o_on, r.verdict)                      # (the oracle is the restatement: shown on the CPU as well)
    differ = d_on != o_on
    bad = np.nonzero(differ & r.decided)[0]
    lines = ["%s: device %d, oracle %d (margin %.2e rad, forced verdicts %s, %s)" % (
        oc.describe(ps, i), d_on[i], o_on[i], float(r.margin[i]), r.v_forced[:, i].tolist(), "tie" if r.tie[i] else "no tie") for i in bad[:12]]
    assert not len(bad), "%s: on_track differs from the oracle on %d of %d decided probes\n%s" % (name, len(bad), int(r.decided.sum()), "\n".join(lines))
    und = ~r.decided
    # (nearly all of the `segment` family; a `centre` probe at the bound lands on a tie locus by chance now and then)
    assert int((und & (p.family != oc.FAMILIES.index("segment"))).sum()) * 20 <= max(int(und.sum()), 20)
    one_of = (d_on == r.v_forced[0]) | (d_on == r.v_forced[1])
    assert np.all(one_of[und])                                  # (two booleans that differ: recorded for the shape of the claim, it cannot fail)
    print("\n%s: %d probes, %d undecided (tie locus within %.0e rad, forced verdicts differ); the device parts from the oracle on %d of them" % (
        name, p.m, int(und.sum()), oc.MARGIN, int((differ & und).sum())))
    # the unmodified reference's verdicts, wherever they are the oracle's (exact ties apart: the first minimum is the contract)
    stored, gv = oc.fixture(name)
    n = stored.m
    agree = gv == o_on[:n]
    assert int((~agree).sum()) == REFERENCE_OFF_FIRST_MINIMUM[name] and np.all(r.tie[:n][~agree])
    bad = np.nonzero(agree & r.decided[:n] & (d_on[:n] != gv))[0]
    assert not len(bad), "%s: on_track differs from the reference on %d probes, first: %s" % (name, len(bad), oc.describe(ps, bad[0]))
    # radius and prediction
    assert np.array_equal(dev["radius"], ref["radius"]) and np.array_equal(dev["radius"], ln / 2.0)
    worst = 0.0
    for key in ("pred_x", "pred_y"):
        a, b = dev[key], ref[key]
        bound = pred_bound(b, v)
        ok = same_or_within(a, b, bound)
        assert np.all(ok), "%s: %s differs at %s: %r vs %r" % (name, key, oc.describe(ps, np.nonzero(~ok)[0][0]), a[~ok][0], b[~ok][0])
        fin = np.isfinite(a) & np.isfinite(b)
        worst = max(worst, float(np.max(np.abs(a[fin] - b[fin]) / bound[fin])))
    print("%s: largest |pred - pred_oracle| = %.3f of the bound (1 ulp of |pred| + 8 eps v dt)" % (name, worst))


@pytest.mark.parametrize("name", ("monteblanco", "open"))
def test_call_sizes_cut_from_the_probe_list(backends, name):
    ps, (th, v, ln), dev, _ = full_call(backends, name)
    hip, _ = backends(name)
    p = ps.probes
    fam_start = [int(np.nonzero(p.family == f)[0][0]) for f in sorted(set(p.family.tolist()))]
    for n in CALL_SIZES:
        for lo in sorted(set(fam_start + [0, 1000, p.m - n])):
            lo = min(lo, p.m - n)
            sl = slice(lo, lo + n)
            out = hip.process_objects(p.qx[sl], p.qy[sl], th[sl], v[sl], ln[sl])
            for key in ("on_track", "pred_x", "pred_y", "radius"):
                assert out[key].shape == (n,) and np.array_equal(out[key], dev[key][sl], equal_nan=True), "%s: %d objects from row %d: %s" % (name, n, lo, key)


def prediction_inputs():
    """(px, py, theta, v): every theta with every v, at the origin (the product alone) and at a position on the track (the sum's rounding)."""
    rng = np.random.default_rng(77)
    half = np.array([k * (np.pi / 2) for k in range(-8, 9)] + [np.pi, -np.pi])
    theta = np.concatenate((half, np.nextafter(half, np.inf), np.nextafter(half, -np.inf), rng.uniform(-np.pi, np.pi, 400),
                            [0.0, -0.0, 1e-300, 1e-8, 1.0, 10.0, 1e3, -1e3, 1e5, 1e6, -1e6, 999999.5],
                            rng.uniform(-1e6, 1e6, 200)))
    v = np.concatenate(([0.0, 1e-3, 1.0, 27.5, 80.0], rng.uniform(0.0, 80.0, 11)))
    th, vv = np.repeat(theta, v.size), np.tile(v, theta.size)
    px = np.concatenate((np.zeros(th.size), np.full(th.size, -335.19407831429396)))
    py = np.concatenate((np.zeros(th.size), np.full(th.size, 256.61660572640142)))
    return px, py, np.tile(th, 2), np.tile(vv, 2)


def test_prediction_against_long_double(backends):
    LD = np.longdouble
    hip, orc = backends("monteblanco")
    px, py, th, v = prediction_inputs()
    ln = np.full(px.size, 4.0)
    dev, ref = hip.process_objects(px, py, th, v, ln), orc.process_objects(px, py, th, v, ln)
    ex = {"pred_x": LD(px) - np.sin(LD(th)) * LD(v) * LD(DT), "pred_y": LD(py) + np.cos(LD(th)) * LD(v) * LD(DT)}
    d_max = o_max = 0.0
    for key in ("pred_x", "pred_y"):
        d_err, o_err = np.abs(LD(dev[key]) - ex[key]).astype(np.float64), np.abs(LD(ref[key]) - ex[key]).astype(np.float64)
        d_max, o_max = max(d_max, float(d_err.max())), max(o_max, float(o_err.max()))
    print("\nprediction, %d inputs (long double of %d mantissa bits): largest deviation of the device %.3e m, of the oracle %.3e m" % (
        px.size, np.finfo(LD).nmant, d_max, o_max))
    for key in ("pred_x", "pred_y"):
        d_err = np.abs(LD(dev[key]) - ex[key]).astype(np.float64)
        limit = np.maximum(4.0 * o_max, pred_bound(ex[key].astype(np.float64), v))
        bad = np.nonzero(d_err > limit)[0]
        assert not len(bad), "%s: %d of %d beyond the bound, worst theta %r v %r: %.3e m against %.3e m" % (
            key, len(bad), px.size, th[bad[np.argmax(d_err[bad])]], v[bad[np.argmax(d_err[bad])]], float(d_err[bad].max()), float(limit[bad].min()))
    assert np.array_equal(dev["pred_x"][v == 0.0], px[v == 0.0]) and np.array_equal(dev["pred_y"][v == 0.0], py[v == 0.0])


# ---- the simulation's copy of the body --------------------------------------------------------------------------------------------------------
def boundary_statics(ps, n, ego_layer, seed):
    """``n`` statics (x, y, theta, v, length) alternating inside / outside, and the number of them on the track: the two probes of `bound`
    pairs and, from the 41st on, decided `segment` probes 1e-9 m either side of a tie locus whose band separates them; all at least 30
    layers from the ego."""
    p, r = ps.probes, ps.ref
    rng = np.random.default_rng(seed)
    L = ps.track.L
    far = np.minimum((p.k - ego_layer) % L, (ego_layer - p.k) % L) >= 30
    fb = oc.FAMILIES.index("bound")
    first = np.nonzero((p.family == fb) & (p.pair > np.arange(p.m)) & far)[0]
    pairs = [(int(i), int(p.pair[i])) for i in rng.permutation(first)]
    seg = np.nonzero((p.family == oc.FAMILIES.index("segment")) & (p.offset == 1e-9) & far)[0]
    seg_pairs = []
    for i in seg:                                               # (OFFSETS: +o is followed by -o)
        j = i + 1
        if p.offset[j] == -1e-9 and r.decided[i] and r.decided[j] and r.verdict[i] != r.verdict[j]:
            seg_pairs.append((int(i), int(j)) if r.verdict[i] else (int(j), int(i)))
    assert len(seg_pairs) >= 15
    seg_pairs = [seg_pairs[i] for i in rng.permutation(len(seg_pairs))]
    chosen = pairs[:min(n, 40) // 2] + seg_pairs[:max(n - 40, 0) // 2]
    idx = np.array([i for pr_ in chosen for i in pr_])
    assert len(idx) == n and np.all(r.decided[idx]) and np.all(r.verdict[idx[0::2]]) and not np.any(r.verdict[idx[1::2]])
    rows = [(float(p.qx[i]), float(p.qy[i]), float(rng.uniform(-np.pi, np.pi)), float(rng.uniform(0.0, 8.0)) if q % 3 == 0 else 0.0, 4.0)
            for q, i in enumerate(idx)]
    return rows, n // 2


def test_simulation_copy_on_boundary_statics(monteblanco, oracle_backend):
    import planner_replay as pr
    import sim_loop as sl
    import test_gpu_sim_differential as gd
    from graphbasedlocaltrajectoryplanner_amd import _capi
    from graphbasedlocaltrajectoryplanner_amd.sim import RaceLineTable
    ps = oc.fixture_set("monteblanco")
    table = RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))
    start = pr.load_ticks("c2")[0]['start']
    ego_layer = int(oc.evaluate(ps.track, start['pos'][0], start['pos'][1])[0])
    units, inside = [], []
    for name, n, seed in (("boundary26", 26, 1), ("boundary70", 70, 2)):
        rows, n_in = boundary_statics(ps, n, ego_layer, seed)
        entry = dict(opponents=[], static=rows, pref=sl.DEFAULT_PREF, pos_est=tuple(start['pos']), vel_est=0.0, zone_gids=[])
        units.append(gd.single(name, dict(entry=entry, vel=sl.C2_VEL), start))
        inside.append(n_in)
    assert inside == [13, 35]
    sc = gd.Scenario(monteblanco, table, units)
    hip = _capi.HipBackend(monteblanco)
    n_ticks = 3
    ref = gd.lockstep(sc, hip, oracle_backend, n_ticks, "boundary statics")
    gd.one_call(sc, hip, n_ticks, ref, "boundary statics")
    trace, stats = ref[0], ref[5]
    assert stats['errors'] == 0 and stats['compared_in_full'] == n_ticks * 2, stats
    # kept count = the inside probes, in every tick; the first survivor is the first static (an inside probe), bit for bit
    for k in range(n_ticks):
        for p_, n_in in enumerate(inside):
            assert trace[k, p_, 5] == n_in, (k, p_, trace[k, p_, 5])
            assert np.array_equal(trace[k, p_, 6:8], units[p_]["entries"][0]["static"][0][:2])
    # the free-running host loop's trace rows: kept count and first survivor exact, the digest's counts exact, its sums within the lockstep's scale
    loop = sc.host(oracle_backend)
    host_rows = np.array([sl.trace_rows(loop.tick()) for _ in range(n_ticks)])
    assert np.array_equal(host_rows[:, :, 5:8], trace[:, :, 5:8])
    K = _capi.PLANNER_MAX_KEYS
    dg_dev, dg_host = trace[:, :, 8:], host_rows[:, :, 8:]
    is_float = np.zeros(dg_dev.shape[2], bool)
    is_float[[5, 7]] = True
    for i in range(K):
        is_float[8 + 7 * i + 3: 8 + 7 * i + 7] = True
    assert np.array_equal(dg_dev[:, :, ~is_float], dg_host[:, :, ~is_float])
    assert np.allclose(dg_dev[:, :, is_float], dg_host[:, :, is_float], rtol=1e-5, atol=1e-9)
    hip.close()
