"""
CPU: the behaviour selector of the fleet's simulation (ltpl_fleet_sim_selector) off the device --

  1. csrc/fleet_select.hpp, compiled alone with the host compiler (-ffp-contract=off), equals the Python mirror sim.SelectorModel bit for
     bit on the case list of sim_selector_util.cases (seeded cases plus the boundaries: 0 .. 3 rows, t_i == T, standstill at row 1 and in
     the middle, v_i + v_{i-1} == 0, a trajectory ending inside the horizon, t_last == 0, 0 / 1 / 96 objects, equal clearances, clearance
     at c_hard and one double either side, no objects with w_clear > 0, equal scores, w_switch that flips and does not flip, sel_prev
     outside the list, lists of 1 .. 5 entries with emergency at every position, everything unsafe, NaN rows) and on the size cases of the
     device's lane-stride edges; every boundary group shows what it is there for;
  2. properties: the output is a permutation of the user's list, a one-entry list, an unstarted and a failed planner get the copy;
  3. behaviour in a closed loop on Monteblanco under the oracle's planner (sim_selector_util.Selecting over sim_loop.HostSimLoop): behind
     one slower race-line opponent, with the user's list follow, straight, left, right, the static list never passes, the selector does;
  4. the entry points check their arguments without a device (tools/fakehip/sim_selector_args.py on the plain stand-in build);
  5. the field tables.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import sim_selector_util as su
from graphbasedlocaltrajectoryplanner_amd import sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "sim_selector_shim.cpp")
S, F, L, R, E = su.STRAIGHT, su.FOLLOW, su.LEFT, su.RIGHT, su.EMERGENCY


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("selector") / "sim_selector_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, SHIM], check=True)
    lib = ctypes.CDLL(so)
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.selector_eval_host.argtypes = [P, P, I, I, P, P, P, I, P, P, P, P]
    return lib


@pytest.fixture(scope="module")
def case_list():
    cs, groups = su.cases()
    return cs, groups, [su.mirror(c) for c in cs]


def header(shim, c, rec=None):
    """A case by the compiled header, in the form of sim_selector_util.mirror."""
    par, user = np.array(c["params"], float), np.array(c["user"], np.int32)
    n_rows, rows = np.full(5, -1, np.int32), np.zeros((4, 4, sim.SELECTOR_MAX_ROWS))
    for a in range(4):
        if c["actions"][a] is not None:
            t = c["actions"][a]
            n_rows[a] = t.shape[0]
            rows[a, :, :t.shape[0]] = t.T
    n_rows[4] = 0 if c["emergency"] else -1
    objs = np.ascontiguousarray(np.concatenate((c["objs"], np.zeros((1, 5)))))
    order, act_d, act_i = np.zeros(5, np.int32), np.zeros((4, 3)), np.zeros((4, 2), np.int32)
    r = np.zeros(sim.SELECTOR_DOUBLES) if rec is None else np.array(rec, float)
    if rec is None:
        r[10] = np.inf
    shim.selector_eval_host(par.ctypes.data, user.ctypes.data, len(user), c["sel_prev"], n_rows.ctypes.data, rows.ctypes.data, objs.ctypes.data,
                            c["objs"].shape[0], order.ctypes.data, act_d.ctypes.data, act_i.ctypes.data, r.ctypes.data)
    return dict(order=order[:len(user)].copy(), act_d=act_d, act_i=act_i, rec=r)


# ---- 1. header against mirror -------------------------------------------------------------------------------------------------------------
def test_header_equals_the_mirror_bit_for_bit(shim, case_list):
    cs, groups, ref = case_list
    assert len(groups["random"]) == 40 and shim.selector_record_doubles() == sim.SELECTOR_DOUBLES
    for i, (c, r) in enumerate(zip(cs, ref)):
        su.compare(header(shim, c), r, "case %d" % i)
    for i, c in enumerate(su.size_cases()):
        su.compare(header(shim, c), su.mirror(c), "size case %d" % i)
    # a record carried over several evaluations accumulates the same way on both sides
    rec_h, rec_m = None, None
    for i in groups["lists"] + groups["all unsafe"]:
        rec_h, rec_m = header(shim, cs[i], rec_h)["rec"], su.mirror(cs[i], rec_m)["rec"]
    assert np.array_equal(su.bits(rec_h), su.bits(rec_m)) and rec_m[0] == len(groups["lists"]) + len(groups["all unsafe"])
    total = np.sum([r["rec"][:10] for r in ref], axis=0)
    print("case list: %d cases; counters %s" % (len(cs), dict(zip([f[0] for f in sim.SELECTOR_FIELDS], total.tolist()))))
    assert np.all(total > 0)                 # every counter moves somewhere in the list


def test_every_boundary_group_shows_what_it_is_there_for(case_list):
    cs, groups, ref = case_list

    def of(name):
        return [(cs[i], ref[i]) for i in groups[name]]

    def flags(r, a):
        return int(r["act_i"][a, 1])
    for n in (0, 1, 2, 3):
        (c, r), = of("rows %d" % n)
        assert bool(flags(r, S) & sim.SEL_SCORED) == (n >= 2) and flags(r, S) & sim.SEL_EXPORTED
        if n < 2:
            assert r["order"].tolist() == [L, S]                # not scored: behind the scored action, whatever its score
    (c, r), = of("t == T")
    t, n_r, last, vbar = sim.SelectorModel.times(c["actions"][S][:, 0].tolist(), c["actions"][S][:, 3].tolist(), 3.0)
    assert t[3] == 3.0 and last == 3 and vbar == 1.0
    assert r["act_d"][S, 1] == -2.0 and r["act_i"][S, 0] == 0    # the object on row 3 is met AT t == T: the row is in the window
    (c1, r1), (cm, rm), (cn, rn) = of("standstill")
    assert sim.SelectorModel.times(c1["actions"][S][:, 0].tolist(), c1["actions"][S][:, 3].tolist(), 2.0)[1:] == (1, 0, 0.0)
    assert sim.SelectorModel.times(cm["actions"][S][:, 0].tolist(), cm["actions"][S][:, 3].tolist(), 2.0)[1:3] == (5, 4) and rm["act_d"][S, 0] == 4.0 / 2.0
    assert sim.SelectorModel.times(cn["actions"][S][:, 0].tolist(), cn["actions"][S][:, 3].tolist(), 2.0)[1] == 2
    (c, r), = of("ends inside")
    assert r["act_d"][S, 0] == 1.0                               # (s_last - s_0) / t_last = 4 / 4
    (c, r), = of("t_last == 0")
    assert r["act_d"][S, 0] == 10.0 and not flags(r, S) & sim.SEL_NAN      # v_0
    r0, r1, r96 = [r for _, r in of("objects")]
    assert r0["act_d"][S, 1] == np.inf and r0["act_i"][S, 0] == -1 and r1["act_i"][S, 0] == 0 and 0 <= r96["act_i"][S, 0] < 96
    (c, r), (c2, r2) = of("equal clearance")
    assert r["act_i"][S, 0] == 1 and r2["act_i"][S, 0] == 0      # ties go to the lower object
    at, above, below = [r for _, r in of("c_hard")]
    assert not flags(at, S) & sim.SEL_UNSAFE and flags(above, S) & sim.SEL_UNSAFE and not flags(below, S) & sim.SEL_UNSAFE
    assert at["order"].tolist() == [S, L] and above["order"].tolist() == [L, S]
    (c, r), = of("no objects, w_clear > 0")
    assert r["act_d"][S, 2] == r["act_d"][S, 0] and np.isfinite(r["act_d"][S, 2])         # no penalty, no NaN out of inf
    (c, r), (c2, r2) = of("equal J")
    assert r["act_d"][L, 2] == r["act_d"][R, 2] and r["order"].tolist() == [R, L, S] and r2["order"].tolist() == [L, R, S]
    (c, r), (c2, r2) = of("w_switch")
    assert r["order"].tolist() == [L, S] and r2["order"].tolist() == [S, L]
    assert r["rec"][2] == 1 and r["rec"][3] == 1 and r2["rec"][2] == 0 and r2["rec"][3] == 0       # n_switch, n_override
    for c, r in of("sel_prev not listed"):
        assert r["order"].tolist() == [L, S]                     # both pay w_switch: the faster one wins
    seen = set()
    for c, r in of("lists"):
        assert sorted(r["order"].tolist()) == sorted(c["user"])
        if E in c["user"]:
            seen.add((len(c["user"]), c["user"].index(E)))
    assert seen == {(n, p) for n in range(1, 6) for p in range(n)}
    (c, r), (c2, r2), (c3, r3) = of("all unsafe")
    assert r["order"].tolist()[0] == E and r["rec"][4] == 1 and r["rec"][5] == 1
    assert r2["rec"][4] == 1 and r2["act_d"][r2["order"][0], 1] >= r2["act_d"][r2["order"][1], 1]     # the least bad first
    assert r3["order"].tolist()[2] == F                          # not exported: last
    nan_s, nan_x, nan_v, nan_o = [r for _, r in of("NaN row")]
    assert flags(nan_s, S) & sim.SEL_NAN and nan_s["order"].tolist() == [L, S]
    assert not flags(nan_x, S) & sim.SEL_NAN and np.isfinite(nan_x["act_d"][S, 1])        # a NaN distance never wins the minimum
    assert not flags(nan_v, S) & sim.SEL_NAN                      # a NaN speed: the car stands from that row on
    assert nan_o["act_i"][S, 0] == 1


# ---- 2. properties ------------------------------------------------------------------------------------------------------------------------
def test_properties_of_the_mirror(case_list):
    cs, groups, ref = case_list
    for c, r in zip(cs, ref):
        assert sorted(r["order"].tolist()) == sorted(c["user"])
        if len(c["user"]) == 1:
            assert r["order"].tolist() == c["user"]
    c = cs[groups["w_switch"][0]]
    m = sim.SelectorModel(3, on=[True, False, True], **dict(zip(sim.SELECTOR_PARAMS, c["params"])))
    assert m.select(0, c["user"], c["sel_prev"], c["actions"], c["objs"]) == [L, S] and m.rec[0, 0] == 1
    before = m.rec.copy()
    assert m.select(1, c["user"], c["sel_prev"], c["actions"], c["objs"]) == c["user"]                  # switched off
    assert m.select(0, c["user"], c["sel_prev"], c["actions"], c["objs"], started=False) == c["user"]   # not started
    assert m.select(0, c["user"], c["sel_prev"], c["actions"], c["objs"], failed=True) == c["user"]     # error word set
    assert m.select(2, [L], c["sel_prev"], c["actions"], c["objs"]) == [L]                              # a one-entry list
    assert np.array_equal(m.rec, before)
    with pytest.raises(ValueError):
        sim.SelectorModel(1, bogus=1.0)


# ---- 3. behaviour -------------------------------------------------------------------------------------------------------------------------
class Loop(su.Selecting, sl.HostSimLoop):
    pass


# the opponent starts 100 m ahead of the ego on the race line and drives 0.3 of the race-line speed; 400 ticks of 0.05 s. Chosen on the
# CPU: under the reference's behaviour (the first preferred key) the car closes up and follows to the end of the run
BEHAVIOUR = dict(gap=100.0, scale=0.3, ticks=400,
                 selector=dict(horizon=2.0, r_ego=1.0, c_hard=0.0, c_soft=1.0, w_clear=1.0, w_switch=2.0))


def arc_length(tab, pos):
    return float(tab.s_rl[int(np.argmin((tab.x - pos[0]) ** 2 + (tab.y - pos[1]) ** 2))])


def run_behaviour(monteblanco, oracle_backend, tab, start, selector):
    from oracle.planner_host import HostPlannerBackend
    s0 = arc_length(tab, start['pos'])
    entry = dict(opponents=[(s0 + BEHAVIOUR["gap"], BEHAVIOUR["scale"], 5.0)], static=[], pref=("follow", "straight", "left", "right"),
                 pos_est=tuple(start['pos']), vel_est=0.0, zone_gids=[])
    loop = Loop(monteblanco, tab, [entry], [HostPlannerBackend(monteblanco).planner(1)], oracle=oracle_backend)
    assert loop.set_start(0, start['pos'], start['heading'], start['vel'], start['max_heading_offset'])[0]
    loop.sim_vel(0, **sl.C2_VEL)
    if selector:
        loop.set_selector(sim.SelectorModel(1, **selector))
    out = []
    for k in range(BEHAVIOUR["ticks"]):
        r = loop.tick()[0]
        assert not r["failed"], (k, r.get("error"))
        on_track = bool(loop.ingest([(r["pos"][0], r["pos"][1], 0.0, 0.0, 0.0)])[0][0])
        out.append(dict(sel=r["sel"], s=arc_length(tab, r["pos"]), opp=loop.opp_s[0][0], on_track=on_track))
    return out, loop


def test_the_selector_overtakes_where_the_static_list_follows(monteblanco, oracle_backend):
    tab = sim.RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))
    start = pr.load_ticks("c2")[0]['start']
    static, _ = run_behaviour(monteblanco, oracle_backend, tab, start, None)
    chosen, loop = run_behaviour(monteblanco, oracle_backend, tab, start, BEHAVIOUR["selector"])
    d = loop.selector.as_dict()
    print("static list: actions %s, final gap %.1f m; selector: actions %s, final gap %.1f m; record %s" % (
        sorted(set(r["sel"] for r in static)), static[-1]["opp"] - static[-1]["s"], sorted(set(r["sel"] for r in chosen)),
        chosen[-1]["opp"] - chosen[-1]["s"], {k: v.tolist() for k, v in d.items()}))
    assert all(r["s"] < r["opp"] for r in static), "the static list passed the opponent"
    assert chosen[-1]["s"] > chosen[-1]["opp"], "the selector's car did not end ahead"
    assert d["n_override"][0] > 0 and [r["sel"] for r in static] != [r["sel"] for r in chosen]
    assert all(r["on_track"] for r in chosen)


# ---- 4. the entry points ------------------------------------------------------------------------------------------------------------------
def test_selector_entry_points_check_their_arguments_without_a_device():
    """The real library refuses a null fleet; tools/fakehip/sim_selector_args.py on the stand-in runtime (plain build): every bad argument
    is refused with a message that names it, without allocation or launch; a failing allocation keeps the previous state; a tick with the
    selector on launches k_fleet_sim_select once, a tick with it off never."""
    import sys
    lib = ctypes.CDLL(os.path.join(ROOT, "graphbasedlocaltrajectoryplanner_amd", "csrc", "libltpl_hip.so"))
    assert lib.ltpl_fleet_sim_selector(None, None) == 1 and lib.ltpl_fleet_sim_selector_read(None, None, 12, None, 0) == 1
    assert lib.ltpl_fleet_sim_selector_eval(None, 0, *([None] * 10)) == 1
    env = dict(os.environ, FAKEHIP_SAN="none", LTPL_NO_SELFTEST="1")
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "sim_selector_args.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and "sim selector args OK" in p.stdout, p.stdout[-3000:]
    assert "launches per tick" in p.stdout, p.stdout[-3000:]


# ---- 5. the field tables ------------------------------------------------------------------------------------------------------------------
def test_python_binding_and_header_declare_the_entry_points():
    from graphbasedlocaltrajectoryplanner_amd import fleet
    for name in ("sim_selector", "sim_selector_read", "sim_selector_eval"):
        assert callable(getattr(fleet.Fleet, name)), name
    with open(os.path.join(ROOT, "include", "ltpl_hip.h")) as fh:
        hdr = fh.read()
    for name in ("ltpl_fleet_sim_selector(", "ltpl_fleet_sim_selector_read(", "ltpl_fleet_sim_selector_eval(", "#define LTPL_ABI_VERSION 9",
                 "#define LTPL_FLEET_SIM_SELECTOR_DOUBLES 12"):
        assert name in hdr, name
    assert sim.SELECTOR_DOUBLES == 12 == len(sim.SELECTOR_FIELDS) and fleet.SELECTOR_FIELDS is sim.SELECTOR_FIELDS
    assert [f[1] for f in sim.SELECTOR_FIELDS] == list(range(12))
    assert set(sim.SELECTOR_PARAMS) == set(sim.SELECTOR_DEFAULTS) and len(sim.SELECTOR_PARAMS) == 6
    assert [f.name if hasattr(f, "name") else f[0] for f in fleet.SimSelectorIn._fields_] == ["on"] + list(sim.SELECTOR_PARAMS)
