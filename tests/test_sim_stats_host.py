"""
CPU: the campaign statistics of the fleet's simulation (ltpl_fleet_sim_stats) off the device --

  1. csrc/fleet_stats.hpp, compiled alone with the host compiler (-ffp-contract=off, no sanitizer), equals the Python mirror
     sim.stats_reduce bit for bit on the case list of sim_stats_util.cases: 40 seeded cases plus the constructed ones (0, 1, 63, 64, 65,
     1023, 1024, 1025 and 2049 members; all NaN; NaN and +-inf among good values; a value on every edge and one double either side of e_0
     and e_bins, with 1 and 16 cells; a range whose last edge is not hi; equal extrema in one lane, in two lanes and in two chunks; -0.0
     against +0.0; lists longer than the eligible values, with ties, with an infinity; planners that do not ascend); every group shows
     what it is there for;
  2. the sum order is observable: on cases of 1e300 / -1e300 / 1.0 and of cancellations at 2^53 a left-to-right sum, numpy's pairwise
     sum, the tree with its strides the other way round and the chunks added last first each give other bits than the specified order
     -- asserted on the mirror, so a kernel with one of those orders cannot equal it;
  3. sim.StatsModel on the race4 recording (telemetry and safety mirrors): n, min, argmin and the cells of clear_min / gap_min against
     a direct numpy evaluation of the mirrors' records, per race and over everyone; the counts of a row add up to the members;
  4. the entry points check their arguments without a device (tools/fakehip/sim_stats_args.py on the plain stand-in build);
  5. the declarations.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import planner_replay as pr
import sim_stats_util as xu
import telemetry_util as tu
from graphbasedlocaltrajectoryplanner_amd import sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "sim_stats_shim.cpp")
F = xu.F
bits = xu.bits


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("stats") / "sim_stats_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, SHIM], check=True)
    lib = ctypes.CDLL(so)
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.stats_reduce_host.argtypes = [P, P, I, D, D, I, I, I, P, P]
    lib.stats_edges_host.argtypes = [D, D, I, P]
    return lib


@pytest.fixture(scope="module")
def case_list():
    cs, groups = xu.cases()
    return cs, groups, [xu.mirror(c) for c in cs]


def header(shim, c):
    """A case by the compiled header, in the form of sim_stats_util.mirror."""
    n = c["values"].size
    v = np.ascontiguousarray(np.concatenate((c["values"], [0.0])))
    p = np.ascontiguousarray(np.concatenate((np.arange(n) if c["planners"] is None else c["planners"], [0])).astype(np.int32))
    row, top = np.zeros(sim.STATS_DOUBLES), np.zeros((sim.STATS_MAX_TOP, 2))
    shim.stats_reduce_host(v.ctypes.data, p.ctypes.data, n, c["lo"], c["hi"], c["bins"], c["top_dir"], c["top_k"], row.ctypes.data, top.ctypes.data)
    return dict(row=row, top=top)


# ---- 1. header against mirror -------------------------------------------------------------------------------------------------------------
def test_header_equals_the_mirror_bit_for_bit(shim, case_list):
    cs, groups, ref = case_list
    assert len(groups["random"]) == 40 and shim.stats_row_doubles() == sim.STATS_DOUBLES == 27 and shim.stats_chunk_members() == sim.STATS_CHUNK
    assert shim.stats_max_top() == sim.STATS_MAX_TOP and shim.stats_families() == len(sim.STATS_FAMILIES)
    for k, (c, m) in enumerate(zip(cs, ref)):
        xu.compare(header(shim, c), m, "case %d" % k)
    for lo, hi, b in ((0.1, 0.7, 16), (-3.0, 1e-3, 7), xu.rounded_range()):
        e = np.zeros(b + 1)
        shim.stats_edges_host(lo, hi, b, e.ctypes.data)
        assert np.array_equal(bits(e), bits(sim.stats_edges(lo, hi, b)))


def test_every_group_shows_what_it_is_there_for(case_list):
    cs, groups, ref = case_list
    row = lambda i: ref[i]["row"]                                                     # noqa: E731
    top = lambda i: ref[i]["top"]                                                     # noqa: E731
    assert [cs[i]["values"].size for i in groups["counts"]] == list(xu.COUNTS)
    for i in groups["counts"]:
        n = cs[i]["values"].size
        assert row(i)[F["n"]] == n and row(i)[F["under"]] + row(i)[F["over"]] + row(i)[F["hist"]:].sum() == n
        assert np.sum(top(i)[:, 1] >= 0) == min(n, 8)
    i = groups["counts"][0]                                                           # the empty group
    assert row(i)[F["min"]] == np.inf and row(i)[F["argmin"]] == -1 and row(i)[F["max"]] == -np.inf and row(i)[F["argmax"]] == -1
    assert bits(row(i)[F["sum"]]) == bits(0.0) and np.all(np.isnan(top(i)[:, 0])) and np.all(top(i)[:, 1] == -1)
    i = groups["all_nan"][0]
    assert row(i)[F["n_nan"]] == 70 and row(i)[F["n"]] == 0 and row(i)[F["argmin"]] == -1 and np.all(top(i)[:, 1] == -1) and row(i)[F["hist"]:].sum() == 0
    for i in groups["nan_inf"]:
        r = row(i)
        assert r[F["n_nan"]] == 3 and r[F["n_inf"]] == 4 and r[F["n"]] == 293 and r[F["min"]] == -np.inf and r[F["max"]] == np.inf
        assert r[F["argmin"]] == 5 and r[F["argmax"]] == 4 and np.isfinite(r[F["sum"]]) and np.isfinite(r[F["sumsq"]])
        assert r[F["under"]] >= 2 and r[F["over"]] >= 2 and r[F["under"]] + r[F["over"]] + r[F["hist"]:].sum() == 297
        assert np.isinf(top(i)[0, 0]) and np.isinf(top(i)[1, 0]) and np.isfinite(top(i)[2, 0])
    for i in groups["edges"]:
        b = cs[i]["bins"]
        r = row(i)
        # e_0 .. e_(bins-1) open their cells, one double under e_0 is under, e_bins and one above it are over; the doubles next to e_0 and
        # under e_bins fall into the first and the last cell
        want = np.ones(b)
        want[0] += 1
        want[b - 1] += 1
        assert r[F["under"]] == 1 and r[F["over"]] == 2 and np.array_equal(r[F["hist"]:F["hist"] + b], want) and r[F["hist"] + b:].sum() == 0
    assert sorted(cs[i]["bins"] for i in groups["edges"]) == [1, 16]
    i = groups["rounded"][0]
    e = sim.stats_edges(cs[i]["lo"], cs[i]["hi"], cs[i]["bins"])
    assert e[-1] != cs[i]["hi"] and row(i)[F["over"]] == (3 if e[-1] < cs[i]["hi"] else 2) and row(i)[F["under"]] == 0
    for k, i in enumerate(groups["equal_extrema"]):
        v, r = cs[i]["values"], row(i)
        lo_at, hi_at = np.flatnonzero(v == -1.5), np.flatnonzero(v == 1.75)
        assert lo_at.size == 2 and hi_at.size == 2 and r[F["min"]] == -1.5 and r[F["max"]] == 1.75
        if cs[i]["planners"] is None:                                                 # ties go to the lower planner, wherever it sits
            assert r[F["argmin"]] == lo_at[0] and r[F["argmax"]] == hi_at[0] and top(i)[:2, 1].tolist() == lo_at.tolist()
        else:
            p = cs[i]["planners"]
            assert r[F["argmin"]] == p[lo_at].min() == p[lo_at[1]] and r[F["argmax"]] == p[hi_at[1]] and top(i)[:2, 1].tolist() == sorted(p[hi_at])
    spans = {(tuple(np.flatnonzero(cs[i]["values"] == -1.5) % 64), tuple(np.flatnonzero(cs[i]["values"] == -1.5) // 1024)) for i in groups["equal_extrema"]}
    assert spans == {((5, 5), (0, 0)), ((5, 9), (0, 0)), ((5, 28), (0, 1))}           # the same lane, two lanes, two chunks
    seen = set()
    for i in groups["zeros"]:
        v, r = cs[i]["values"], row(i)
        z = np.flatnonzero(v == 0.0)
        at = "min" if cs[i]["top_dir"] < 0 else "max"
        assert z.size == 2 and r[F[at]] == 0.0 and r[F["arg" + at]] == z[0] and bits(r[F[at]]) == bits(v[z[0]])   # the lower planner's bits
        assert bits(top(i)[0, 0]) == bits(v[z[0]]) and bits(top(i)[1, 0]) == bits(v[z[1]])
        seen.add((at, bool(np.signbit(v[z[0]])), int(z[1] // 1024)))
    assert len(seen) == 8
    t = [top(i) for i in groups["top"]]
    assert t[0][:3].tolist() == [[1.0, 2.0], [2.0, 3.0], [3.0, 0.0]] and np.all(t[0][3:, 1] == -1)
    assert t[1][:5].tolist() == [[1.0, 1.0], [1.0, 3.0], [1.0, 6.0], [2.0, 0.0], [2.0, 2.0]] and np.all(t[1][5:, 1] == -1)
    assert t[2][:5].tolist() == [[5.0, 4.0], [2.0, 5.0], [2.0, 7.0], [2.0, 9.0], [1.0, 3.0]]
    assert t[3][:3].tolist() == [[np.inf, 1.0], [2.0, 0.0], [1.0, 3.0]] and t[4][:3].tolist() == [[-np.inf, 2.0], [1.0, 3.0], [2.0, 0.0]]
    assert np.all(t[5][:, 1] == -1) and np.all(np.isnan(t[5][:, 0]))
    for i in groups["unordered"]:
        p = cs[i]["planners"]
        assert np.any(np.diff(p) < 0) and np.all(np.isin(top(i)[:, 1], p)) and row(i)[F["argmin"]] in p
        k = top(i)[:, 0] * (1.0 if cs[i]["top_dir"] < 0 else -1.0)
        assert np.all(np.diff(k) >= 0) and np.any(np.diff(k) == 0)                    # in order, with ties -- which go by planner:
        assert all(top(i)[j, 1] < top(i)[j + 1, 1] for j in range(7) if k[j] == k[j + 1])
    assert len(groups["order"]) == 4


# ---- 2. the sum order ---------------------------------------------------------------------------------------------------------------------
def test_the_sum_order_is_observable(case_list):
    oc = xu.order_cases()
    assert sorted(oc) == ["all", "chunks", "lanes", "p53"], "no seeded placement tells all four orders apart"
    want = {k: sim.stats_sum(x) for k, x in oc.items()}
    assert want["lanes"] == 1.0 and want["chunks"] == 0.0 and all(np.isfinite(w) for w in want.values())
    differs = {name: [k for k, x in sorted(oc.items()) if bits(f(x)) != bits(want[k])] for name, f in xu.OTHER_ORDERS}
    print("sums in the specified order: %s; cases on which another order gives other bits: %s" % (want, differs))
    assert "lanes" in differs["left to right"] and "lanes" in differs["numpy pairwise"] and "lanes" in differs["strides ascending"]
    assert "chunks" in differs["chunks reversed"]
    assert "p53" in differs["left to right"] and "p53" in differs["strides ascending"]
    assert all("all" in d for d in differs.values())
    # ... and the row carries exactly that sum, sumsq the same order over the squares
    cs, groups, ref = case_list
    for i in groups["order"]:
        x = cs[i]["values"]
        with np.errstate(over="ignore"):
            assert bits(ref[i]["row"][F["sum"]]) == bits(sim.stats_sum(x)) and bits(ref[i]["row"][F["sumsq"]]) == bits(sim.stats_sum(x * x))


# ---- 3. the model on a recording ----------------------------------------------------------------------------------------------------------
def test_stats_model_on_the_race4_recording(monteblanco, oracle_backend):
    tele = tu.recording_mirror("race4", monteblanco, oracle_backend)["rows"]
    cars = [pr.load_ticks("race4_car%d" % k) for k in range(4)]
    saf = sim.SafetyModel(4, r_ego=1.25)
    for k in range(120):
        for p, c in enumerate(cars):
            pos = np.asarray(c[k]['obj_pos'], float).reshape(-1, 2)
            pred = np.asarray(c[k]['obj_pred'], float).reshape(pos.shape[0], -1)[:, :2]
            saf.step(p, c[k]['pos_est'], np.concatenate((pos, pred, np.asarray(c[k]['obj_radius'], float).reshape(-1, 1)), axis=1), tu.DT)
        saf.advance()
    records = dict(telemetry=tele, safety=saf.rec)
    measures = [("telemetry", "clear_min", 0.0, 8.0, 8, -1), ("safety", "gap_min", -2.0, 6.0, 16, -1), ("safety", "ttc_min", 0.0, 10.0, 5, -1),
                ("state", "failed", 0.0, 2.0, 2, 1)]
    for groups in ([0, 0, 0, 0], [0, 0, 1, -1]):
        model = sim.StatsModel(groups, measures, top_k=3)
        rows, tops = model.reduce(records)
        assert rows.shape == (max(groups) + 1, 4, 27) and tops.shape == (max(groups) + 1, 4, 3, 2)
        for g in range(max(groups) + 1):
            mem = np.flatnonzero(np.asarray(groups) == g)
            for m, (fam, field, lo, hi, b, _) in enumerate(measures[:3]):
                v = records[fam][mem, sim.stats_column(fam, field)[1]]
                r = rows[g, m]
                fin = np.isfinite(v)
                assert r[F["n"]] == fin.sum() and r[F["n_inf"]] == np.isinf(v).sum() and r[F["n_nan"]] == np.isnan(v).sum()
                assert r[F["min"]] == v.min() and r[F["argmin"]] == mem[np.argmin(v)]
                edges = np.array(sim.stats_edges(lo, hi, b))
                assert np.array_equal(r[F["hist"]:F["hist"] + b], np.histogram(v[fin & (v < edges[-1])], bins=edges)[0])
                # every member is somewhere: the cells hold the finite values inside, under / over the rest and the infinities, n_nan the NaN
                assert r[F["hist"]:].sum() + r[F["under"]] + r[F["over"]] + r[F["n_nan"]] == mem.size
                assert r[F["under"]] == np.sum(v < lo) and r[F["over"]] == np.sum(v >= edges[-1])
                assert tops[g, m, 0, 0] == r[F["min"]] and tops[g, m, 0, 1] == r[F["argmin"]]
            assert rows[g, 3, F["sum"]] == 0 and rows[g, 3, F["n"]] == mem.size                  # nobody failed
    d = sim.stats_dict(rows)
    assert np.allclose(d["mean"][0, 1], saf.rec[:2, 5].mean()) and np.all(d["var"][..., 3] == 0)
    assert np.isinf(saf.rec[:, 8]).any() or np.isfinite(saf.rec[:, 8]).all()
    # the series: period 4 over 10 ticks from tick0 = 1 -- rows at the ticks 3 and 7, a ring of depth 1 keeps the last
    model = sim.StatsModel([0, 0, 1, -1], measures, period=4, depth=1, tick0=1)
    hits = [model.tick(records) for _ in range(10)]
    assert [k for k, hit in enumerate(hits) if hit] == [2, 6]
    ticks, ring, total = model.series()
    assert ticks.tolist() == [7] and total == 2 and np.array_equal(bits(ring[0]), bits(model.reduce(records)[0]))


# ---- 4. the entry points ------------------------------------------------------------------------------------------------------------------
def test_stats_entry_points_check_their_arguments_without_a_device():
    """The real library refuses a null fleet; tools/fakehip/sim_stats_args.py on the stand-in runtime (plain build): every bad argument is
    refused with a message that names it, without allocation or launch; a failing allocation keeps the previous plan; the two kernels run
    on the ticks of the period's rule and never without a plan."""
    import sys
    lib = ctypes.CDLL(os.path.join(ROOT, "graphbasedlocaltrajectoryplanner_amd", "csrc", "libltpl_hip.so"))
    assert lib.ltpl_fleet_sim_stats(None, None) == 1 and lib.ltpl_fleet_sim_stats_reduce(None, None, 27, None, 0) == 1
    assert lib.ltpl_fleet_sim_stats_series(None, None, None, 27, None, None) == 1 and lib.ltpl_fleet_sim_stats_eval(None, 0, *([None] * 6)) == 1
    env = dict(os.environ, FAKEHIP_SAN="none", LTPL_NO_SELFTEST="1")
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "sim_stats_args.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and "sim stats args OK" in p.stdout, p.stdout[-3000:]
    assert "launches per tick" in p.stdout and "period 3, tick0 0: reductions on ticks [2, 5] of 7" in p.stdout, p.stdout[-3000:]


# ---- 5. the declarations ------------------------------------------------------------------------------------------------------------------
def test_python_binding_and_header_declare_the_entry_points():
    from graphbasedlocaltrajectoryplanner_amd import fleet
    for name in ("sim_stats", "sim_stats_reduce", "sim_stats_series", "sim_stats_eval"):
        assert callable(getattr(fleet.Fleet, name)), name
    with open(os.path.join(ROOT, "include", "ltpl_hip.h")) as fh:
        hdr = fh.read()
    for name in ("ltpl_fleet_sim_stats(", "ltpl_fleet_sim_stats_reduce(", "ltpl_fleet_sim_stats_series(", "ltpl_fleet_sim_stats_eval(",
                 "#define LTPL_ABI_VERSION 9", "#define LTPL_FLEET_SIM_STATS_DOUBLES 27", "#define LTPL_FLEET_SIM_STATS_MAX_BINS 16",
                 "#define LTPL_FLEET_SIM_STATS_MAX_TOP 8", "#define LTPL_SIM_STATS_KEEP_SERIES 1u"):
        assert name in hdr, name
    for k, fam in enumerate(sim.STATS_FAMILIES):
        assert "#define LTPL_SIM_STATS_%s" % fam.upper() in hdr and ("LTPL_SIM_STATS_%-9s %d\n" % (fam.upper(), k)) in hdr, fam
    assert sim.STATS_DOUBLES == 27 == sim.STATS_FIELDS[-1][1] + sim.STATS_BINS and fleet.STATS_FIELDS is sim.STATS_FIELDS
    assert [f[1] for f in sim.STATS_FIELDS] == list(range(12)) and len(sim.STATS_FAMILIES) == 9 and sim.STATS_FAMILIES[-1] == "state"
    assert [f[0] for f in fleet.SimStatsIn._fields_] == ["n_groups", "group", "n_measures", "family", "column", "lo", "hi", "bins", "top_dir", "top_k",
                                                        "period", "depth", "tick0", "flags"]
    assert sum(sim.STATS_FAMILY_DOUBLES[f] for f in sim.STATS_FAMILIES[:-1]) == 129
    assert sim.stats_column("safety", "ttc_min") == (6, 8) and sim.stats_column("telemetry", "act[4]") == (0, 13) and sim.stats_column("state", "failed") == (8, 0)
    assert sim.stats_column(7, 3) == (7, 3) and sim.stats_column("safety", "hist[7]") == (6, 30)
    for bad in (("bogus", "x"), ("safety", "bogus")):
        with pytest.raises(ValueError):
            sim.stats_column(*bad)
    d = sim.stats_dict(np.array([[4.0, 0, 0, 1.0, 0, 3.0, 3, 8.0, 20.0, 0, 0] + [0.0] * 16, [0.0] * 27]))
    assert d["mean"][0] == 2.0 and d["var"][0] == 1.0 and np.isnan(d["mean"][1]) and d["hist"].shape == (2, 16) and d["n"].dtype == np.int64
