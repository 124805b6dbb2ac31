"""
TEST INFRASTRUCTURE (no test functions): the campaign statistics of the fleet's simulation (ltpl_fleet_sim_stats, csrc/fleet_stats.hpp) --
the case list of the rule (seeded cases plus the constructed boundaries), the mirror in the form the header's shim and the device's hook
return, and the other summation orders a wrong kernel could use. Shared by tests/test_sim_stats_host.py and tests/test_gpu_sim_stats.py.
A CASE is one group and one measure: dict(values [n], planners [n] or None (the positions), lo, hi, bins, top_dir, top_k).
"""
import math

import numpy as np

from graphbasedlocaltrajectoryplanner_amd import sim

UP, DOWN = math.inf, -math.inf
COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)
BIG, P53 = 1.0e300, 2.0 ** 53
F = {name: i for name, i, _ in sim.STATS_FIELDS}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def case(values, planners=None, lo=-2.0, hi=2.0, bins=8, top_dir=-1, top_k=3):
    return dict(values=np.asarray(values, np.float64).reshape(-1), planners=None if planners is None else np.asarray(planners, np.int64).reshape(-1),
                lo=float(lo), hi=float(hi), bins=int(bins), top_dir=int(top_dir), top_k=int(top_k))


def spec_of(c):
    return [c["lo"], c["hi"], float(c["bins"]), float(c["top_dir"]), float(c["top_k"])]


def mirror(c):
    row, top = sim.stats_reduce(c["values"], c["planners"], c["lo"], c["hi"], c["bins"], c["top_dir"], c["top_k"])
    return dict(row=row, top=top)


def compare(got, want, what):
    for k in ("row", "top"):
        a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert a.shape == b.shape, "%s: %s has shape %s, the mirror's %s" % (what, k, a.shape, b.shape)
        ne = bits(a) != bits(b)
        assert not ne.any(), "%s: %s differs at %s: %s against the mirror's %s" % (what, k, np.argwhere(ne)[:6].tolist(), a[ne][:6], b[ne][:6])


def rounded_range():
    """(lo, hi, bins) with e_bins = lo + ((hi - lo) * bins) / bins != hi: the first of a fixed sequence of candidates."""
    rng = np.random.RandomState(7)
    for _ in range(10000):
        lo, hi, bins = float(rng.uniform(-3.0, 0.0)), float(rng.uniform(0.1, 3.0)), int(rng.randint(2, 17))
        if sim.stats_edges(lo, hi, bins)[bins] != hi:
            return lo, hi, bins
    raise AssertionError("no range whose last edge rounds away from hi")


# ---- the other orders a sum could take ------------------------------------------------------------------------------------------------------
def sum_plain(x):
    t = 0.0
    for v in np.asarray(x, np.float64).reshape(-1):
        t = t + float(v)
    return t


def sum_numpy(x):
    return float(np.sum(np.asarray(x, np.float64).reshape(-1)))


def _chunk_lanes(x):
    x = np.asarray(x, np.float64).reshape(-1)
    nch = (x.size + sim.STATS_CHUNK - 1) // sim.STATS_CHUNK
    a = np.zeros(nch * sim.STATS_CHUNK)
    a[:x.size] = x
    a = a.reshape(nch, -1, sim.STATS_LANES)
    t = np.zeros((nch, sim.STATS_LANES))
    for j in range(a.shape[1]):
        t = t + a[:, j, :]
    return t


def sum_other_strides(x):
    """The specified order with the tree's strides ascending: t[l] += t[l + s] for l a multiple of 2 s, s = 1, 2, .. 32."""
    t = _chunk_lanes(x)
    s = 1
    while s < sim.STATS_LANES:
        t[:, 0::2 * s] = t[:, 0::2 * s] + t[:, s::2 * s]
        s *= 2
    total = 0.0
    for c in range(t.shape[0]):
        total = total + float(t[c, 0])
    return total


def sum_chunks_reversed(x):
    """The specified order with the chunk sums added last chunk first."""
    t = _chunk_lanes(x)
    s = sim.STATS_LANES // 2
    while s >= 1:
        t = t[:, :s] + t[:, s:2 * s]
        s //= 2
    total = 0.0
    for c in reversed(range(t.shape[0])):
        total = total + float(t[c, 0])
    return total


OTHER_ORDERS = (("left to right", sum_plain), ("numpy pairwise", sum_numpy), ("strides ascending", sum_other_strides), ("chunks reversed", sum_chunks_reversed))


def order_cases():
    """{name: values}: sums that tell the specified order from the others. 'lanes': 1e300, 1.0, -1e300 in lanes 0, 1, 2 -- the tree adds
    lanes 0 and 2 first (exactly 0) and keeps the 1.0; left to right, numpy and ascending strides lose it in 1e300. 'chunks': chunk sums 1.0,
    1e300, -1e300 -- ascending loses the 1.0, descending keeps it. 'p53': 2^53, 1.0, 1.0, -2^53 the same way round at the rounding step of
    2^53. 'all': a seeded placement of such values over three chunks on which ALL four other orders miss the specified bits."""
    out = {}
    out["lanes"] = np.array([BIG, 1.0, -BIG])
    ch = np.zeros(2 * sim.STATS_CHUNK + 1)
    ch[0], ch[sim.STATS_CHUNK], ch[2 * sim.STATS_CHUNK] = 1.0, BIG, -BIG
    out["chunks"] = ch
    p = np.zeros(sim.STATS_CHUNK + 70)
    p[0], p[1], p[67], p[2], p[sim.STATS_CHUNK + 3] = P53, 1.0, 1.0, -P53, 1.0      # lanes 0, 1, 3 (its second round), 2; the next chunk
    out["p53"] = p
    pool = np.array([BIG, -BIG, 1.0, P53, -P53, 1.0, 3.0, -BIG / 2.0, BIG / 2.0, P53 * 4.0, -P53 * 4.0, 0.5])
    for seed in range(2000):
        rng = np.random.RandomState(seed)
        x = np.zeros(2 * sim.STATS_CHUNK + 200)
        x[rng.choice(x.size, 40, replace=False)] = pool[rng.randint(0, pool.size, 40)]
        want = sim.stats_sum(x)
        if math.isfinite(want) and all(bits(f(x)) != bits(want) for _, f in OTHER_ORDERS):
            out["all"] = x
            break
    return out


# ---- the case list ---------------------------------------------------------------------------------------------------------------------------
def cases():
    """(cases, groups): groups name -> indices into cases."""
    cs, groups = [], {}

    def add(group, c):
        groups.setdefault(group, []).append(len(cs))
        cs.append(c)

    rng = np.random.RandomState(20261021)
    for k in range(40):                     # seeded: sizes up to three chunks, every kind of value, every spec
        n = int(rng.choice([0, 1, 5, 64, 200, 1024, 1500, 2500])) if k % 4 else int(rng.randint(0, 3000))
        v = rng.normal(0.0, 1.5, n)
        kind = rng.uniform(size=n)
        v[kind < 0.05] = np.nan
        v[(kind >= 0.05) & (kind < 0.08)] = np.inf
        v[(kind >= 0.08) & (kind < 0.11)] = -np.inf
        v[(kind >= 0.11) & (kind < 0.2)] = np.round(v[(kind >= 0.11) & (kind < 0.2)])       # ties
        planners = None if k % 3 == 0 else rng.permutation(4 * n + 3)[:n] if k % 3 == 1 else np.sort(rng.permutation(4 * n + 3)[:n])
        lo = float(rng.uniform(-3.0, 0.0))
        add("random", case(v, planners, lo=lo, hi=lo + float(rng.uniform(0.5, 5.0)), bins=int(rng.randint(1, 17)), top_dir=int(rng.randint(-1, 2)),
                           top_k=int(rng.randint(0, 9))))
    for n in COUNTS:
        add("counts", case(rng.normal(0.0, 1.0, n), top_dir=1 if n % 2 else -1, top_k=8))
    add("all_nan", case(np.full(70, np.nan), top_k=4))
    v = rng.normal(0.0, 1.0, 300)
    v[[3, 64, 200]], v[[4, 130]], v[[5, 299]] = np.nan, np.inf, -np.inf
    add("nan_inf", case(v, top_dir=-1, top_k=4))
    add("nan_inf", case(v, top_dir=1, top_k=4))
    for bins in (1, 16):                    # a value on every edge and one double either side of e_0 and e_bins
        lo, hi = 0.1, 0.7
        e = sim.stats_edges(lo, hi, bins)
        v = list(e) + [np.nextafter(e[0], DOWN), np.nextafter(e[0], UP), np.nextafter(e[bins], DOWN), np.nextafter(e[bins], UP)]
        add("edges", case(v, lo=lo, hi=hi, bins=bins, top_k=0))
    lo, hi, bins = rounded_range()
    e = sim.stats_edges(lo, hi, bins)
    add("rounded", case([hi, e[bins], np.nextafter(min(hi, e[bins]), DOWN), np.nextafter(max(hi, e[bins]), UP), lo], lo=lo, hi=hi, bins=bins))
    for a, b in ((5, 5 + 64), (5, 9), (5, 1500)):               # equal extrema: the same lane, two lanes, two chunks
        v = rng.uniform(-1.0, 1.0, 1600)
        v[[a, b]] = -1.5
        v[[a + 1, b + 1]] = 1.75
        add("equal_extrema", case(v, top_dir=-1, top_k=3))
        add("equal_extrema", case(v, planners=np.arange(1600)[::-1] + 7, top_dir=1, top_k=3))
    for first, second in ((-0.0, 0.0), (0.0, -0.0)):            # -0.0 against +0.0, as minimum and as maximum, in a chunk and across two
        for at in ((2, 40), (2, 1100)):
            for sign in (1.0, -1.0):
                v = sign * rng.uniform(0.5, 1.0, 1200)
                v[at[0]], v[at[1]] = first, second
                add("zeros", case(v, top_dir=-1 if sign > 0 else 1, top_k=2))
    add("top", case([3.0, np.nan, 1.0, 2.0, np.nan], top_dir=-1, top_k=8))            # K above the eligible values
    add("top", case([2.0, 1.0, 2.0, 1.0, 2.0, 5.0, 1.0], top_dir=-1, top_k=5))        # ties inside the list
    add("top", case([2.0, 1.0, 2.0, 1.0, 2.0, 5.0, 1.0], planners=[9, 8, 7, 6, 5, 4, 3], top_dir=1, top_k=5))
    add("top", case([2.0, np.inf, -np.inf, 1.0], top_dir=1, top_k=3))                 # an infinity in the list
    add("top", case([2.0, np.inf, -np.inf, 1.0], top_dir=-1, top_k=3))
    add("top", case(rng.normal(0.0, 1.0, 100), top_dir=0, top_k=8))                   # no list asked for
    v = np.round(rng.normal(0.0, 2.0, 1300))
    add("unordered", case(v, planners=rng.permutation(5000)[:1300], top_dir=-1, top_k=8))
    add("unordered", case(v, planners=rng.permutation(5000)[:1300], top_dir=1, top_k=8))
    for name, x in sorted(order_cases().items()):
        add("order", case(x, lo=-1.0, hi=4.0, bins=5, top_dir=1, top_k=2))
    return cs, groups
