"""
CPU: the reactive opponents of the fleet's simulation (ltpl_fleet_sim_react) off the device --

  1. csrc/fleet_react.hpp, compiled alone with the host compiler (-ffp-contract=off, no sanitizer), equals the Python mirror
     sim.ReactModel / sim.react_tick bit for bit on the case list of sim_react_util.cases: 40 seeded cases plus the constructed ones (0, 1,
     2, 64, 65 and 96 opponents; two opponents at the same s both ways round and three at the same s; a leader across the wrap; s below
     S[0]; D == look and one double beyond; |d_e| == lat_gate and one double beyond; ego and an opponent at equal D; gap == 0 and one
     double either side; dv < 0 with z clamped to 0; c == 0; a table row with V == 0; acc on and beyond the clamps; e' clamped at c and at
     0; an ego with no candidate segment; a NaN ego pose; look = +inf) and on a 12-tick sequence with scales and record carried over;
     every group shows what it is there for. acc BEYOND the upper clamp cannot be constructed: free = 1 - r^4 <= 1 and k k >= 0 give
     acc <= a_max for every input, so that clamp is exercised ON the bound only (e == 0 on a free road);
  2. the free-road invariant: e == c and no leader gives e' == c bitwise, for 1 000 seeded (c, s);
  3. behaviour on the host loop (sim_react_util.ReactiveSimLoop over the oracle's planner, Monteblanco): (a) a fast opponent behind a slow
     one -- blind it drives through, reactive it follows with gap > 0 on every tick; (b) a slow ego with a faster opponent behind it --
     blind the safety mirror counts overlap ticks, reactive none, and the opponent follows the ego;
  4. the entry points check their arguments without a device (tools/fakehip/sim_react_args.py on the plain stand-in build);
  5. the field tables.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import sim_react_util as ru
import sim_selector_util as slu
from graphbasedlocaltrajectoryplanner_amd import sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "sim_react_shim.cpp")
LEADER, DELTA, GAP, ACC = ru.LEADER, ru.DELTA, ru.GAP, ru.ACC
F = {name: i for name, i, _ in sim.REACT_FIELDS}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("react") / "sim_react_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, SHIM], check=True)
    lib = ctypes.CDLL(so)
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.react_tick_host.argtypes = [P, P, P, P, P, I, D, D, D, D, D, P, I, P, P, P, P]
    lib.react_start_host.argtypes = [P]
    return lib


@pytest.fixture(scope="module")
def case_list():
    cs, groups = ru.cases()
    return cs, groups, [ru.mirror(c) for c in cs]


def header(shim, c, rec=None):
    """A case by the compiled header, in the form of sim_react_util.mirror."""
    t = ru.tables()[c["table"]]
    rec = np.array(sim.react_start(1)[0] if rec is None else rec, float)
    par, n = np.array(c["par"], float), c["opp"].shape[0]
    opp = np.ascontiguousarray(np.concatenate((c["opp"], np.zeros((1, 4)))))
    e, po, ego = np.zeros(n + 1), np.zeros((n + 1, 4)), np.zeros(3)
    shim.react_tick_host(par.ctypes.data, t.s_rl.ctypes.data, t.x.ctypes.data, t.y.ctypes.data, t.vel_rl.ctypes.data, len(t.s_rl), c["ego"][0],
                         c["ego"][1], c["ego"][2], c["dt"], float(c["tick"]), opp.ctypes.data, n, rec.ctypes.data, e.ctypes.data, po.ctypes.data,
                         ego.ctypes.data)
    return dict(rec=rec, e=e[:n], per_opp=po[:n], ego=ego)


# ---- 1. header against mirror -------------------------------------------------------------------------------------------------------------
def test_header_equals_the_mirror_bit_for_bit(shim, case_list):
    cs, groups, ref = case_list
    assert len(groups["random"]) == 40 and shim.react_record_doubles() == sim.REACT_DOUBLES and shim.react_param_doubles() == len(sim.REACT_PARAMS)
    r = np.zeros(16)
    shim.react_start_host(r.ctypes.data)
    assert np.array_equal(ru.bits(r), ru.bits(sim.react_start(1)[0]))
    for k, (c, m) in enumerate(zip(cs, ref)):
        ru.compare(header(shim, c), m, "case %d" % k)
    seq = ru.sequence()
    got, want = ru.run_sequence(seq, lambda c, r: header(shim, c, r)), ru.run_sequence(seq)
    for k, (a, b) in enumerate(zip(got, want)):
        ru.compare(a, b, "sequence tick %d" % k)
    # the sequence is a closing pair behind the ego: both follow, and the scales move from tick to tick
    assert want[-1]["rec"][F["follow_ticks"]] == 2 * len(seq) and want[-1]["rec"][F["ego_lead_ticks"]] == len(seq)
    assert want[-1]["e"][0] < want[0]["e"][0] < 0.5
    # every field of the record moves somewhere in the list
    moved = np.zeros(16, bool)
    for m in ref:
        moved |= ru.bits(m["rec"]) != ru.bits(sim.react_start(1)[0])
    assert np.all(moved), [sim.REACT_FIELDS[i][0] for i in np.nonzero(~moved)[0]]


def test_every_group_shows_what_it_is_there_for(case_list):
    cs, groups, ref = case_list
    t = ru.tables()["mb"]
    lap = float(t.s_rl[-1])

    def of(name):
        return [(cs[i], ref[i]) for i in groups[name]]
    assert [c["opp"].shape[0] for c, _ in of("opponents")] == [0, 1, 2, 64, 65, 96]
    seen = set()
    for _, m in of("random") + of("opponents"):
        seen |= set(np.unique(np.minimum(m["per_opp"][:, LEADER], 0)).astype(int).tolist())
    assert seen == {sim.REACT_NONE, sim.REACT_EGO, 0}, seen          # no leader, the ego, an opponent: all among the seeded cases
    assert sum(m["rec"][F["ego_outside"]] for _, m in of("random")) >= 5 and sum(m["rec"][F["ego_lead_ticks"]] for _, m in of("random")) >= 5
    # the same s: the lower index is ahead at 0 (an overlap), the higher one a lap ahead -- beyond look, or the leader with look = +inf
    (ca, ma), (cb, mb), (c3, m3), (ci, mi) = of("same s")
    for m in (ma, mb):
        assert m["per_opp"][0, LEADER] == sim.REACT_NONE and m["per_opp"][1, LEADER] == 0 and m["per_opp"][1, DELTA] == 0.0
        assert m["per_opp"][1, ACC] == -9.0 and m["rec"][F["overlaps"]] == 1
    assert ma["e"][1] != mb["e"][1]                                  # (the other way round it is the other car that brakes)
    assert m3["per_opp"][:, LEADER].tolist() == [sim.REACT_NONE, 0, 0] and m3["rec"][F["overlaps"]] == 2
    assert mi["per_opp"][0, LEADER] == 1 and mi["per_opp"][0, DELTA] == lap and mi["per_opp"][1, LEADER] == 0
    (c, m), = of("wrap")
    assert c["opp"][1, 0] < c["opp"][0, 0] and m["per_opp"][0, LEADER] == 1 and 0.0 < m["per_opp"][0, DELTA] < 60.0
    assert m["per_opp"][1, LEADER] == sim.REACT_NONE
    (c, m), = of("below S[0]")
    assert np.all(c["opp"][:2, 0] < t.s_rl[0]) and m["per_opp"][:, LEADER].tolist() == [1, 2, sim.REACT_NONE] and m["rec"][F["passive"]] == 0
    (c_on, m_on), (c_off, m_off) = of("look")
    assert m_on["per_opp"][0, DELTA] == c_on["par"][6] and m_on["per_opp"][0, LEADER] == 1
    assert m_off["per_opp"][0, LEADER] == sim.REACT_NONE and c_off["par"][6] < c_on["par"][6] and m_off["e"][0] == 0.5
    (c_in, m_in), (c_out, m_out) = of("lat_gate")
    assert abs(m_in["ego"][1]) == c_in["par"][7] and m_in["per_opp"][0, LEADER] == sim.REACT_EGO and m_in["rec"][F["ego_outside"]] == 0
    assert m_out["per_opp"][0, LEADER] == sim.REACT_NONE and m_out["rec"][F["ego_outside"]] == 1 and m_out["ego"][2] == 1.0
    (c1, m1), (c2, m2) = of("ego tie")
    assert m1["per_opp"][0, LEADER] == sim.REACT_EGO and m2["per_opp"][1, LEADER] == sim.REACT_EGO          # the ego wins the tie at equal D
    assert m1["per_opp"][0, DELTA] == c1["opp"][1, 0] - c1["opp"][0, 0] == m1["ego"][0] - c1["opp"][0, 0]
    (c0, m0), (cu, mu), (cd, md) = of("gap 0")
    assert m0["per_opp"][0, GAP] == 0.0 and m0["rec"][F["overlaps"]] == 1 and m0["rec"][F["clamped"]] == 0 and m0["per_opp"][0, ACC] == -9.0
    assert 0.0 < mu["per_opp"][0, GAP] < 1e-12 and mu["rec"][F["overlaps"]] == 0 and mu["rec"][F["clamped"]] == 1
    assert -1e-12 < md["per_opp"][0, GAP] < 0.0 and md["rec"][F["overlaps"]] == 1
    (c, m), = of("z clamped")
    proj = ru.projector("mb")
    v_q, u = (c["opp"][q, 2] * proj._interp(c["opp"][q, 0], proj.vrl, proj._segment(c["opp"][q, 0])) for q in (0, 1))
    assert v_q < u and v_q * 0.0 + (v_q * (v_q - u)) / (2.0 * math.sqrt(3.0 * 4.0)) < 0.0
    r4 = ((0.1 / 0.5) * (0.1 / 0.5)) * ((0.1 / 0.5) * (0.1 / 0.5))
    assert m["per_opp"][0, ACC] == 3.0 * ((1.0 - r4) - (2.0 / m["per_opp"][0, GAP]) * (2.0 / m["per_opp"][0, GAP]))      # k = gap0 / gap: z == 0
    (c, m), = of("c == 0")
    assert m["rec"][F["passive"]] == 2 and m["e"].tolist() == [0.0, m["e"][1], -0.1] and m["per_opp"][1, LEADER] == 0       # passive, still a leader
    (c, m), = of("V == 0")
    assert m["rec"][F["passive"]] == 1 and m["e"][0] == 0.5 and m["per_opp"][1, LEADER] == 0 and m["e"][1] < 0.5            # ... at speed 0
    (c_ov, m_ov), (c_cl, m_cl), (c_up, m_up) = of("clamps")
    assert m_ov["per_opp"][0, ACC] == -9.0 and m_ov["rec"][F["clamped"]] == 0 and m_ov["rec"][F["overlaps"]] == 1
    assert m_cl["per_opp"][0, ACC] == -9.0 and m_cl["rec"][F["clamped"]] == 1 and m_cl["rec"][F["overlaps"]] == 0 and m_cl["per_opp"][0, GAP] == 0.5
    assert m_up["per_opp"][0, ACC] == 3.0 and m_up["e"][0] > 0.0
    (c_c, m_c), (c_0, m_0) = of("e clamps")
    assert c_c["opp"][0, 2] < 0.5 and m_c["e"][0] == 0.5 and m_c["per_opp"][0, ACC] > 0.0
    assert m_0["e"][0] == 0.0 and m_0["per_opp"][0, ACC] < 0.0
    (c, m), = of("no segment")
    assert m["ego"][2] == 0.0 and m["rec"][F["ego_outside"]] == 0 and m["per_opp"][:, LEADER].tolist() == [1, 0]       # (the ego leads nobody, whatever the gate)
    for c, m in of("NaN ego"):
        assert m["ego"][2] == 1.0 and math.isnan(m["ego"][1]) and m["rec"][F["ego_outside"]] == 1 and m["per_opp"][0, LEADER] == 1
    (c1, m1), (c2, m2) = of("look inf")
    assert m1["per_opp"][0, LEADER] == sim.REACT_NONE and m1["e"][0] == 0.5                  # alone on the track: +inf <= +inf finds nobody
    assert m2["per_opp"][0, LEADER] == 1 and m2["per_opp"][0, DELTA] == lap - 100.0 and m2["per_opp"][1, LEADER] == 0


# ---- 2. the free road ---------------------------------------------------------------------------------------------------------------------
def test_on_a_free_road_the_scale_stays_the_configured_one_bitwise(shim):
    rng = np.random.default_rng(7)
    lap = float(ru.tables()["mb"].s_rl[-1])
    n = 0
    for k in range(1000):
        c, s = float(rng.uniform(1e-3, 2.0)), float(rng.uniform(-5.0, lap + 5.0))
        cs = ru.case([(s, c, c, 5.0)], dt=float(rng.choice([0.01, 0.05, 0.1, 1.0])), look=float(rng.choice([10.0, 150.0, math.inf])))
        m = ru.mirror(cs)
        assert m["per_opp"][0, LEADER] == sim.REACT_NONE and ru.bits(m["e"])[0] == ru.bits([c])[0] and m["per_opp"][0, ACC] == 0.0, (k, c, s)
        if k % 10 == 0:
            ru.compare(header(shim, cs), m, "free road %d" % k)
            n += 1
    assert n == 100


# ---- 3. behaviour -------------------------------------------------------------------------------------------------------------------------
REACT = dict(sim.REACT_DEFAULTS)


def host_loop(monteblanco, oracle_backend, tab, start, entry, vel, start_vel, react):
    from oracle.planner_host import HostPlannerBackend
    loop = ru.ReactiveSimLoop(monteblanco, tab, [entry], [HostPlannerBackend(monteblanco).planner(1)], oracle=oracle_backend, react=react)
    assert loop.set_start(0, start['pos'], start['heading'], start_vel, start['max_heading_offset'])[0]
    loop.sim_vel(0, **vel)
    return loop


def closing_speed(tab, s_fast, c_fast, s_slow, c_slow):
    proj = sim.react_projector(tab)
    return c_fast * proj._interp(s_fast, proj.vrl, proj._segment(s_fast)) - c_slow * proj._interp(s_slow, proj.vrl, proj._segment(s_slow))


def test_a_fast_opponent_follows_a_slow_one_instead_of_driving_through(monteblanco, oracle_backend):
    tab = ru.tables()["mb"]
    start = pr.load_ticks("c2")[0]['start']
    s0 = slu.arc_length(tab, start['pos'])
    opp = [(s0 + 300.0, 0.5, 5.0), (s0 + 330.0, 0.2, 5.0)]             # far ahead of the ego: it leads neither
    entry = dict(opponents=opp, static=[], pref=sl.DEFAULT_PREF, pos_est=tuple(start['pos']), vel_est=0.0, zone_gids=[])
    closing = closing_speed(tab, opp[0][0], opp[0][1], opp[1][0], opp[1][1])
    assert closing > 5.0 and closing * closing / (2.0 * REACT["b_max"]) < REACT["look"] - 5.0, closing      # the set-up: it can stop in sight
    lap = float(tab.s_rl[-1])
    out = {}
    for name, on in (("blind", 0), ("reactive", 1)):
        loop = host_loop(monteblanco, oracle_backend, tab, start, entry, sl.C2_VEL, start['vel'], dict(REACT, on=on))
        dist, gaps = [], []
        for k in range(120):
            r = loop.tick()[0]
            assert not r["failed"], (name, k, r.get("error"))
            dist.append((r["opp_s"][1] - r["opp_s"][0]) % lap)
            if on:
                po = loop.model.last[0][0]
                assert po[0, LEADER] == 1 and po[1, LEADER] == sim.REACT_NONE, (k, po)
                gaps.append(po[0, GAP])
        out[name] = (np.array(dist), np.array(gaps), loop.model.as_dict())
    blind, reactive = out["blind"], out["reactive"]
    print("blind: smallest distance %.3f m; reactive: smallest distance %.3f m, smallest gap %.3f m, record %s" % (
        blind[0].min(), reactive[0].min(), reactive[1].min(), {k: v[0].tolist() for k, v in reactive[2].items()}))
    assert np.min(np.minimum(blind[0], lap - blind[0])) < 5.0                       # blind: the centres closer than half the summed lengths
    assert blind[2]["ticks"][0] == 0                                                # (on == 0: the model does nothing)
    assert np.all(reactive[1] > 0.0) and reactive[2]["follow_ticks"][0] == 120 and reactive[2]["overlaps"][0] == 0
    assert reactive[2]["gap_min"][0] == reactive[1].min() and reactive[0].min() > 5.0


def test_a_faster_opponent_behind_a_slow_ego_follows_it(monteblanco, oracle_backend):
    tab = ru.tables()["mb"]
    start = pr.load_ticks("c2")[0]['start']
    s0 = slu.arc_length(tab, start['pos'])
    opp = [((s0 - 30.0) % float(tab.s_rl[-1]), 0.5, 5.0)]            # 30 m behind the ego, across the start line: the ego leads over the wrap
    v_ego = 6.0
    entry = dict(opponents=opp, static=[], pref=("straight",), pos_est=tuple(start['pos']), vel_est=v_ego, zone_gids=[])
    proj = sim.react_projector(tab)
    closing = opp[0][1] * proj._interp(opp[0][0], proj.vrl, proj._segment(opp[0][0])) - v_ego
    assert closing > 5.0 and closing * closing / (2.0 * REACT["b_max"]) < REACT["look"] - 5.0, closing
    safety = dict(r_ego=1.5)
    out = {}
    for name, on in (("blind", 0), ("reactive", 1)):
        loop = host_loop(monteblanco, oracle_backend, tab, start, entry, dict(sl.C2_VEL, vel_max=v_ego), v_ego, dict(REACT, on=on))
        saf = sim.SafetyModel(1, **safety)
        for k in range(100):
            r = loop.tick()[0]
            if not on and r["failed"]:
                break                        # (driven into from behind, the planner loses `straight`: the blind run ends in a failure no planner could avoid)
            assert not r["failed"] and r["sel"] == "straight", (name, k, r.get("error"))
            saf.step(0, r["pos"], [(v[2][0, 0], v[2][0, 1], v[2][1, 0], v[2][1, 1], v[0]) for v in r["veh"]], loop.dt)
            saf.advance()
        out[name] = (saf.as_dict(), loop.model.as_dict())
    print("blind: %s\nreactive: %s\n%s" % ({k: v[0].tolist() for k, v in out["blind"][0].items()},
                                            {k: v[0].tolist() for k, v in out["reactive"][0].items()},
                                            {k: v[0].tolist() for k, v in out["reactive"][1].items()}))
    assert out["blind"][0]["overlap_ticks"][0] > 0
    assert out["reactive"][0]["overlap_ticks"][0] == 0 and out["reactive"][1]["ego_lead_ticks"][0] > 0 and out["reactive"][1]["overlaps"][0] == 0


# ---- 4. the entry points ------------------------------------------------------------------------------------------------------------------
def test_react_entry_points_check_their_arguments_without_a_device():
    """The real library refuses a null fleet; tools/fakehip/sim_react_args.py on the stand-in runtime (plain build): every bad argument is
    refused with a message that names it, without allocation or launch; a failing allocation keeps the previous model; a tick with the
    model on launches k_fleet_sim_react once, a tick with it off never."""
    import sys
    lib = ctypes.CDLL(os.path.join(ROOT, "graphbasedlocaltrajectoryplanner_amd", "csrc", "libltpl_hip.so"))
    assert lib.ltpl_fleet_sim_react(None, None) == 1 and lib.ltpl_fleet_sim_react_read(None, None, 16, None) == 1
    assert lib.ltpl_fleet_sim_react_eval(None, 0, *([None] * 10)) == 1
    env = dict(os.environ, FAKEHIP_SAN="none", LTPL_NO_SELFTEST="1")
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "sim_react_args.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and "sim react args OK" in p.stdout, p.stdout[-3000:]
    assert "launches per tick" in p.stdout, p.stdout[-3000:]


# ---- 5. the field tables ------------------------------------------------------------------------------------------------------------------
def test_python_binding_and_header_declare_the_entry_points():
    from graphbasedlocaltrajectoryplanner_amd import fleet
    for name in ("sim_react", "sim_react_read", "sim_react_eval"):
        assert callable(getattr(fleet.Fleet, name)), name
    with open(os.path.join(ROOT, "include", "ltpl_hip.h")) as fh:
        hdr = fh.read()
    for name in ("ltpl_fleet_sim_react(", "ltpl_fleet_sim_react_read(", "ltpl_fleet_sim_react_eval(", "#define LTPL_ABI_VERSION 9",
                 "#define LTPL_FLEET_SIM_REACT_DOUBLES 16", "#define LTPL_FLEET_SIM_REACT_PARAMS 9", "#define LTPL_SIM_REACT_KEEP_STATE 1u"):
        assert name in hdr, name
    assert sim.REACT_DOUBLES == 16 == len(sim.REACT_FIELDS) and fleet.REACT_FIELDS is sim.REACT_FIELDS
    assert [f[1] for f in sim.REACT_FIELDS] == list(range(16)) and len(sim.REACT_PARAMS) == 9 and sim.REACT_PARAMS[0] == "on"
    assert set(sim.REACT_PARAMS[1:]) == set(sim.REACT_DEFAULTS)
    assert [f[0] for f in fleet.SimReactIn._fields_] == list(sim.REACT_PARAMS) + ["tick0", "flags"]
    with pytest.raises(ValueError):
        sim.ReactModel(1, ru.tables()["mb"], [[0.3]], bogus=1.0)
    rec = sim.react_start(2)
    assert math.isinf(rec[1, 7]) and rec[1, 8] == -1.0 and sim.react_dict(rec)["gap_slot"].tolist() == [-1, -1]
