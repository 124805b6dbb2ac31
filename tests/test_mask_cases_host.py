"""CPU: the probe sets of tests/mask_cases.py are good inputs before any kernel sees them -- on every lattice of tests/test_gpu_mask_boundary.py
the oracle alone (OracleBackend.plan_paths_mask, pinned to the reference's own edge sets by tests/test_edge_mask.py) satisfies what the GPU
test then asks of the kernel, the probes populate the three classes of the capsule cull (restated in tests/test_capsule_cull.py, with the table
of `ltpl_edge_capsules`) and the filler scenarios keep their promises. Prints, per lattice and set, the observable share, the class shares
and the number of exact ties."""
import numpy as np
import pytest

import mask_cases as mc
from test_capsule_cull import capsules, kernel_decisions
from graphbasedlocaltrajectoryplanner_amd import _capi

W_LAST = [0.0, 0.5, 0.8]
MIN_OBSERVABLE = 0.75            # of the probes that hit under the exact test: the oracle blocks the edge (the others: closest layer outside the window)
PLAN_CLASS = {"monteblanco": "PlanFx<32,32,1>", "S": "PlanRt", "B": "PlanFx<32,40,1>", "C": "PlanFx<48,32,1>", "c3": "PlanFx<32,40,1>"}

_oracles, _caps = {}, {}


def oracle_mask(name, which):
    """Oracle's mask of a set (uint8 [n scenarios, E]); the backend is made once per lattice."""
    from oracle.oracle_lib import OracleBackend
    if name not in _oracles:
        _oracles[name] = OracleBackend(mc.lattice(name))
    return _oracles[name].plan_paths_mask(_capi.PathsBatch(mc.case_set(name, which).scen, w_last_edges=W_LAST))[1]


def cull_classes(name, p):
    """(miss, hit) of the NumPy restatement of the kernel's cull for Probes ``p``."""
    if name not in _caps:
        _caps[name] = capsules(mc.lattice(name))[:2]
    cap, slack = _caps[name]
    return kernel_decisions(cap[p.edge], slack, p.qx, p.qy, np.sqrt(p.thr2))


@pytest.mark.parametrize("name", mc.LATTICES)
def test_probes_are_observable_and_populate_the_cull_classes(name):
    lat = mc.lattice(name)
    counts = np.zeros(3, np.int64)                       # certain MISS, certain HIT, shell over the lattice's sets
    for which in mc.set_names(name):
        cs = mc.case_set(name, which)
        p = cs.probes
        assert p.n == len(cs.scen)
        blocked = oracle_mask(name, which)[np.arange(p.n), p.edge].astype(bool)
        assert not np.any(blocked & ~p.exact), "%s %s: the oracle blocks an edge its probe misses" % (name, which)
        observable = float(blocked[p.exact].mean())
        miss, hit = cull_classes(name, p)
        shell = ~miss & ~hit
        assert not np.any(miss & p.exact) and not np.any(hit & ~p.exact), "%s %s: the restatement contradicts the exact verdict" % (name, which)
        small = np.abs(p.offset) <= 1e-6
        n_tie = int((p.family == mc.FAMILIES.index("tie")).sum())
        print("%-11s %-7s %5d probes, %4d hit, observable %.3f; certain MISS %.3f, certain HIT %.3f, shell %.3f (|o| <= 1e-6: %.4f); %d ties" % (
            name, which, p.n, int(p.exact.sum()), observable, miss.mean(), hit.mean(), shell.mean(), shell[small].mean(), n_tie))
        assert observable >= MIN_OBSERVABLE, (name, which, observable)
        assert shell[small].mean() >= 0.99, (name, which)
        if which in ("sample", "gap"):
            # the large offsets on their own: both certain classes from +-0.3 on
            for o, cls in ((1.0, miss), (-1.0, hit), (0.3, miss), (-0.3, hit)):
                assert cls[p.offset == o].mean() >= (0.5 if abs(o) == 1.0 else 0.2), (name, which, o)
        if which == "seam" and lat.closed:
            quirk = p.exact & ~blocked & (lat.edge_endpoints()[2][p.edge] == 0)
            assert int(quirk.sum()) >= 20, "%s: %d probes on the seam quirk" % (name, int(quirk.sum()))
        counts += (int(miss.sum()), int(hit.sum()), int(shell.sum()))
    assert np.all(counts >= 0.05 * counts.sum()), (name, counts)
    # the exact test's own boundary: every ray's o = 0 probe hits, 1e-9 m further out it misses
    for which in ("sample", "gap"):
        p = mc.case_set(name, which).probes
        assert p.exact[p.offset == 0.0].all() and not p.exact[p.offset == 1e-9].any() and p.exact[p.offset == -1e-9].all()


@pytest.mark.parametrize("name", [n for n in mc.LATTICES if "fillers" in mc.set_names(n)])
def test_filler_scenarios_keep_their_promises(name):
    lat = mc.lattice(name)
    t = mc.table(lat)
    cs = mc.case_set(name, "fillers")
    p = cs.probes
    n = len(cs.scen)
    near = np.zeros(n, np.int64)
    for i, sc in enumerate(cs.scen):
        x, y, thr2 = mc.positions_of(lat, sc)
        k = int(cs.pos_index[i])
        assert len(x) == cs.n_fill[i] + 1 <= mc.MAX_POS and len(sc["vehicles"]) <= mc.MAX_VEH
        assert all(1 <= np.asarray(pos).reshape(-1, 2).shape[0] <= 3 for _, pos in sc["vehicles"])
        assert (x[k], y[k], thr2[k]) == (p.qx[i], p.qy[i], p.thr2[i])
        others = np.arange(len(x)) != k
        e = np.full(int(others.sum()), p.edge[i])
        assert mc.clearance(lat, e, x[others], y[others], thr2[others]).min() >= mc.FILLER_CLEARANCE, "scenario %d: a filler reaches the probe's edge" % i
        assert len(set(thr2.tolist())) >= 2                                              # thresholds differ from lane to lane
        assert cs.fill_boundary[cs.fill_off[i]:cs.fill_off[i + 1]].mean() >= 0.5
        ol = mc.closest_layer(lat, x[others], y[others])
        dl = int(t.dst_layer[p.edge[i]])
        near[i] = int(np.count_nonzero((ol == dl) | (ol + 1 == dl)))
    assert sorted(set(cs.n_fill.tolist())) == sorted(mc.FILLER_COUNTS)
    assert set(np.round(np.abs(p.offset), 15).tolist()) == set(np.round(np.abs(mc.OFFSETS), 15).tolist())
    assert int((cs.pos_index >= 64).sum()) >= 5 and int((cs.pos_index >= 128).sum()) >= 2 and int((cs.pos_index % 64 != 0).sum()) >= n // 2
    # fillers in the probe's own transition: more than one round of MQ queries there
    print("%s fillers: positions in the probe's transition besides the probe: min %d, median %d" % (name, near.min(), int(np.median(near))))
    assert np.mean(near >= 3) >= 0.9
    # a flush in the middle of a transition on the one-wave plan classes (derivation: tests/mask_cases.py)
    need = mc.SHELL_CAP[PLAN_CLASS[name]] - mc.MQ * 64 + 1
    if need > 1:
        if name not in _caps:
            _caps[name] = capsules(lat)[:2]
        cap, slack = _caps[name]
        classify = lambda e, qx, qy, thr2: kernel_decisions(cap[e], slack, qx, qy, np.sqrt(thr2))
        pairs = [mc.mid_transition_pairs(lat, cs.scen[i], int(t.dst_layer[p.edge[i]]), classify) for i in np.nonzero(cs.dense)[0]]
        print("%s fillers: shell pairs in front of the last round of the probe's transition, dense scenarios: %s (a flush needs %d)" % (name, pairs, need))
        assert max(pairs) >= need
