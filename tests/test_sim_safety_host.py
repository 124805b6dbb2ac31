"""
CPU: the safety monitor of the fleet's simulation (ltpl_fleet_sim_safety) off the device --

  1. csrc/fleet_safety.hpp, compiled alone with the host compiler (-ffp-contract=off), equals the Python mirror sim.SafetyModel /
     sim.safety_tick bit for bit on the case list of sim_safety_util.cases (40 seeded cases plus the boundaries: 0, 1, 64, 65 and 96
     objects, gap exactly 0 and one double either side, c and gap of different sign by rounding, b == 0, disc exactly 0 and just negative,
     a == 0, dist == 0, wn == 0, an object on the corridor edge and one double outside, lon - rho negative inside the corridor, equal TTC
     in two slots, all TTC +inf, NaN / inf objects among good ones, ttc_t on each of the 7 bin edges and on ttc_thr, a tick without a
     previous pose) and on sequences (an incident that opens, deepens, closes and reopens; the ninth incident wrapping the ring); every
     boundary group shows what it is there for;
  2. properties: TTC against a brute-force time march of the two discs to 1e-9 (both solve the same quadratic; the formula's own error at
     these magnitudes is ~1e-13), gap_min == clear_min - r_ego bitwise against sim.Telemetry on the race4 recording,
     tet == dt x (ticks under the threshold), sum(hist) == ticks_eval;
  3. behaviour on the host loop (sim_loop.HostSimLoop over the oracle's planner, Monteblanco) behind a slower race-line opponent with
     `follow` first: the scenario exercises the rule, and a twin with a larger perception error scores worse -- as monitored (true
     positions, perceived velocities) and on the objects' true velocities, with a smaller true gap: the drive, not only the input;
  4. the entry points check their arguments without a device (tools/fakehip/sim_safety_args.py on the plain stand-in build);
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
import sim_noise_util as nu
import sim_safety_util as su
import telemetry_util as tu
from graphbasedlocaltrajectoryplanner_amd import sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "sim_safety_shim.cpp")
TTC, DRAC, THW, GAP, CLOSING, FLAGS = range(6)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("safety") / "sim_safety_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, SHIM], check=True)
    lib = ctypes.CDLL(so)
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.safety_tick_host.argtypes = [P, D, D, D, D, P, I, P, P, P, P]
    lib.safety_start_host.argtypes = [P, P]
    return lib


@pytest.fixture(scope="module")
def case_list():
    cs, groups = su.cases()
    return cs, groups, [su.mirror(c) for c in cs]


def header(shim, c, rec=None, inc=None):
    """A case by the compiled header, in the form of sim_safety_util.mirror."""
    r0, i0 = su.start_of(c)
    rec, inc = np.array(r0 if rec is None else rec, float), np.array(i0 if inc is None else inc, float)
    par, n = np.array(c["par"], float), c["objs"].shape[0]
    objs = np.ascontiguousarray(np.concatenate((c["objs"], np.zeros((1, 5)))))
    po, pt = np.zeros((n + 1, 6)), np.zeros(8)
    shim.safety_tick_host(par.ctypes.data, c["pose"][0], c["pose"][1], c["dt"], float(c["tick"]), objs.ctypes.data, n, rec.ctypes.data,
                          inc.ctypes.data, po.ctypes.data, pt.ctypes.data)
    return dict(rec=rec, inc=inc, per_obj=po[:n], per_tick=pt)


INCIDENT_TTCS = [4.0, 3.0, 2.0, 2.5, 4.0, None, 1.0, 4.0]          # no incident, opens, deepens, stays open, closes, no object, reopens, closes


# ---- 1. header against mirror -------------------------------------------------------------------------------------------------------------
def test_header_equals_the_mirror_bit_for_bit(shim, case_list):
    cs, groups, ref = case_list
    assert len(groups["random"]) == 40 and shim.safety_record_doubles() == sim.SAFETY_DOUBLES
    assert shim.safety_ring_doubles() == sim.SAFETY_INCIDENTS * sim.INCIDENT_DOUBLES
    r, i = np.zeros(31), np.zeros((8, 6))
    shim.safety_start_host(r.ctypes.data, i.ctypes.data)
    r0, i0 = sim.safety_start(1)
    assert np.array_equal(su.bits(r), su.bits(r0[0])) and np.all(np.isnan(i)) and np.all(np.isnan(i0))
    for k, (c, m) in enumerate(zip(cs, ref)):
        su.compare(header(shim, c), m, "case %d" % k)
    for ttcs in (INCIDENT_TTCS, [1.0, 4.0] * 9):
        seq = su.sequence(ttcs)
        for k, (a, b) in enumerate(zip(su.run_sequence(seq, lambda c, r, i: header(shim, c, r, i)), su.run_sequence(seq))):
            su.compare(a, b, "sequence tick %d" % k)
    # every field of the record moves somewhere in the list
    moved = np.zeros(31, bool)
    for c, m in zip(cs, ref):
        moved |= su.bits(m["rec"]) != su.bits(su.start_of(c)[0])
    print("case list: %d cases; record fields that never move: %s" % (len(cs), [sim.SAFETY_FIELDS[min(i, 23)][0] for i in np.nonzero(~moved)[0]]))
    assert np.all(moved[:23]) and np.sum(moved[23:]) >= 7


def test_every_boundary_group_shows_what_it_is_there_for(case_list):
    cs, groups, ref = case_list

    def of(name):
        return [(cs[i], ref[i]) for i in groups[name]]

    def fl(r, k=0):
        return int(r["per_obj"][k, FLAGS])
    assert [c["objs"].shape[0] for c, _ in of("objects")] == [0, 1, 64, 65, 96]
    (c, r) = of("objects")[0]
    assert r["per_tick"].tolist() == [np.inf, -1.0, np.inf, -1.0, 0.0, np.inf, 0.0, 0.0] and r["rec"][23 + 7] == 1 and r["rec"][1] == 1
    assert of("objects")[3][1]["per_tick"][1] >= 0
    at, above, below = [r for _, r in of("gap")]
    assert at["per_obj"][0, GAP] == 0.0 and fl(at) & sim.SAF_OVERLAP and at["per_obj"][0, TTC] == 0.0 and at["rec"][18] == 1
    assert 0.0 < above["per_obj"][0, GAP] < 1e-15 and not fl(above) & sim.SAF_OVERLAP and above["per_obj"][0, TTC] > 0.0 and above["rec"][18] == 0
    assert above["per_obj"][0, DRAC] > 1e15                      # a hair's gap at 5 m/s of closing speed
    assert below["per_obj"][0, GAP] < 0.0 and fl(below) & sim.SAF_OVERLAP
    flips = of("sign flip")
    assert len(flips) == 2, "the search found %d of the two roundings" % len(flips)
    (c, r), (c2, r2) = flips
    assert r["per_obj"][0, GAP] > 0.0 and not fl(r) & sim.SAF_OVERLAP and r["per_obj"][0, TTC] == 0.0        # c <= 0 by rounding: TTC 0, no overlap
    assert r["rec"][18] == 0                                     # ... and no overlap tick
    assert not r2["per_obj"][0, GAP] > 0.0 and fl(r2) & sim.SAF_OVERLAP and r2["per_obj"][0, TTC] == 0.0
    (c, r), = of("b == 0")
    assert r["per_obj"][0, TTC] == np.inf and r["per_obj"][0, CLOSING] == 0.0 and not fl(r) & sim.SAF_COURSE and r["per_obj"][0, DRAC] == 0.0
    (c, r), (c2, r2) = of("grazing")
    assert fl(r) & sim.SAF_COURSE and r["per_obj"][0, TTC] == 2.0 and r["per_obj"][0, DRAC] > 0.0                # disc == 0: they touch at t = 2
    assert not fl(r2) & sim.SAF_COURSE and r2["per_obj"][0, TTC] == np.inf and r2["per_obj"][0, DRAC] == 0.0    # disc < 0: a miss
    assert r2["per_obj"][0, CLOSING] > 0.0
    (c, r), = of("a == 0")
    assert r["per_obj"][0, TTC] == np.inf and r["per_obj"][0, CLOSING] == 0.0 and fl(r) & sim.SAF_CORRIDOR
    assert r["per_obj"][0, THW] == (10.0 - 2.5) / 5.0
    (c, r), = of("dist == 0")
    assert fl(r) & sim.SAF_OVERLAP and r["per_obj"][0, TTC] == 0.0 and r["per_obj"][0, CLOSING] > 0.0 and r["per_tick"][6] == r["per_obj"][0, CLOSING]
    assert r["rec"][19] == r["per_obj"][0, CLOSING]              # impact_max
    (c, r), = of("wn == 0")
    assert r["per_obj"][0, THW] == np.inf and not fl(r) & sim.SAF_CORRIDOR and np.isfinite(r["per_obj"][0, TTC]) and r["rec"][1] == 1
    on, out, neg = [r for _, r in of("corridor edge")]
    assert fl(on) & sim.SAF_CORRIDOR and on["per_obj"][0, THW] == 3.5 and fl(neg) & sim.SAF_CORRIDOR
    assert not fl(out) & sim.SAF_CORRIDOR and out["per_obj"][0, THW] == np.inf
    (c, r), = of("lon < rho")
    assert fl(r) & sim.SAF_CORRIDOR and r["per_obj"][0, THW] == 0.0 and r["rec"][17] == 1
    (c, r), (c2, r2) = of("equal ttc")
    assert r["per_obj"][1, TTC] == r["per_obj"][2, TTC] < r["per_obj"][0, TTC] and r["per_tick"][3] == 1.0 and r2["per_tick"][3] == 0.0
    (c, r), = of("all inf")
    assert np.all(r["per_obj"][:, TTC] == np.inf) and r["per_tick"][2] == np.inf and r["per_tick"][3] == 0.0 and r["rec"][30] == 1
    assert r["rec"][8] == np.inf and r["rec"][21] == 0
    (c, r), = of("not finite")
    assert [fl(r, k) & sim.SAF_SKIPPED for k in range(5)] == [0, 1, 1, 1, 0] and r["rec"][20] == 3
    assert r["per_tick"][1] == 4.0 and r["per_tick"][3] == 4.0 and np.isfinite(r["per_tick"][[0, 2, 4, 7]]).all()
    for j, (c, r) in enumerate(of("bin edges")):
        edge = (c["par"][1] * (j + 1)) / 7.0
        assert r["per_tick"][2] == edge == 0.5 * (j + 1)          # exactly on the edge: the bin above
        assert np.nonzero(r["rec"][23:31])[0].tolist() == [j + 1]
        assert (r["rec"][21], r["rec"][11]) == ((1, c["dt"]) if j < 6 else (0, 0.0))       # ttc_t == ttc_thr is not under the threshold
    (c, r), = of("no previous pose")
    assert r["rec"][0] == 1 and r["rec"][1] == 0 and r["rec"][4] == 1 and (r["rec"][2], r["rec"][3]) == c["pose"]
    assert r["rec"][5] == -0.5 and r["rec"][7] == 1 and r["rec"][18] == 1 and r["rec"][8] == np.inf and np.sum(r["rec"][23:31]) == 0
    assert np.all(np.isnan(r["inc"])) and r["rec"][21] == 0


def test_incidents_open_deepen_close_reopen_and_wrap():
    out = su.run_sequence(su.sequence(INCIDENT_TTCS))
    n_inc = [int(r["rec"][21]) for r in out]
    is_open = [int(r["rec"][22]) for r in out]
    assert n_inc == [0, 1, 1, 1, 1, 1, 2, 2] and is_open == [0, 1, 1, 1, 0, 0, 1, 0]
    ring = out[-1]["inc"]
    assert ring[0, :4].tolist() == [101.0, 103.0, 2.0, 0.0] and ring[1, :4].tolist() == [106.0, 106.0, 1.0, 0.0]
    assert ring[0, 4] == 2.0 and ring[0, 5] == 1.0 and np.all(np.isnan(ring[2:]))      # gap_min of the incident (D - rho = w ttc), closing_max
    assert out[-1]["rec"][8] == 1.0 and out[-1]["rec"][9] == 106.0
    assert len(sim.safety_incidents(ring, 2)) == 2 and sim.safety_incidents(ring, 2)[1]["tick_first"] == 106.0
    wrap = su.run_sequence(su.sequence([1.0, 4.0] * 9))
    assert wrap[-1]["rec"][21] == 9 and wrap[15]["inc"][0, 0] == 100.0 and wrap[-1]["inc"][0, 0] == 116.0 and wrap[-1]["inc"][1, 0] == 102.0
    assert [d["tick_first"] for d in sim.safety_incidents(wrap[-1]["inc"], 9)] == [102.0 + 2 * k for k in range(8)]


# ---- 2. properties ------------------------------------------------------------------------------------------------------------------------
def test_ttc_agrees_with_a_time_march_of_the_two_discs(case_list):
    cs, groups, ref = case_list
    n, grazes, far, worst = 0, 0, 0, 0.0
    for i in groups["random"] + groups["equal ttc"]:     # (not the exact graze: a tangent touch is ill-conditioned for a march)
        c, r = cs[i], ref[i]
        for k in range(c["objs"].shape[0]):
            t, slack = su.march_ttc(c, k)
            ttc = r["per_obj"][k, TTC]
            if abs(slack) < 1e-6 and (t == np.inf) != (ttc == np.inf):
                grazes += 1                   # a pass that grazes within the march's resolution
                continue
            if ttc > 40.0:
                assert t == np.inf, (i, k, ttc, t)
                far += 1                      # (no touch inside the march's 40 s: +inf, or a TTC beyond it)
            else:
                assert abs(ttc - t) <= 1e-9, (i, k, ttc, t)
                worst = max(worst, abs(ttc - t))
            n += 1
    print("time march: %d objects, %d of them without a touch inside 40 s, %d grazing passes left out, largest |ttc - march| %.3g s" % (
        n, far, grazes, worst))
    assert n - far >= 40, "only %d objects were compared to 1e-9" % (n - far)
    assert n >= 150 and grazes <= 2        # (the 40 seeded cases hold 0 .. 12 objects each)


def test_gap_min_equals_telemetrys_clearance_on_the_race4_recording(monteblanco, oracle_backend):
    tele = tu.recording_mirror("race4", monteblanco, oracle_backend)["fields"]
    cars = [pr.load_ticks("race4_car%d" % k) for k in range(4)]
    r_ego = 1.25
    m = sim.SafetyModel(4, r_ego=r_ego)
    under = np.zeros(4)
    for k in range(len(cars[0])):
        for p, c in enumerate(cars):
            pos = np.asarray(c[k]['obj_pos'], float).reshape(-1, 2)
            pred = np.asarray(c[k]['obj_pred'], float).reshape(pos.shape[0], -1)[:, :2]
            objs = np.concatenate((pos, pred, np.asarray(c[k]['obj_radius'], float).reshape(-1, 1)), axis=1)
            _, pt = m.step(p, c[k]['pos_est'], objs, tu.DT)
            under[p] += m.rec[p, 1] > 0 and pt[2] < m.par[p, 1] and k > 0
        m.advance()
    d = m.as_dict()
    assert np.array_equal(su.bits(d["gap_min"]), su.bits(tele["clear_min"] - r_ego)), (d["gap_min"], tele["clear_min"] - r_ego)
    assert np.array_equal(d["gap_tick"], tele["clear_tick"]) and np.array_equal(d["gap_slot"], tele["clear_slot"])
    assert np.all(d["ticks"] == 600) and np.all(d["ticks_eval"] == 599) and np.array_equal(d["hist"].sum(axis=1), d["ticks_eval"])
    # tet is dt added once per tick under the threshold: the same sum, in the same order
    for p in range(4):
        t = 0.0
        for _ in range(int(under[p])):
            t += tu.DT
        assert d["tet"][p] == t and abs(t - tu.DT * under[p]) < 1e-9
    print("race4: gap_min %s, ttc_min %s, tet %s s, incidents %s, overlap ticks %s" % (d["gap_min"], d["ttc_min"], d["tet"], d["n_incidents"],
                                                                                     d["overlap_ticks"]))
    assert np.any(d["n_incidents"] > 0)


# ---- 3. behaviour -------------------------------------------------------------------------------------------------------------------------
# a flying start at 20 m/s, 60 m behind an opponent that drives 0.2 of the race-line speed, `follow` first; 200 ticks of 0.05 s. Chosen on
# the CPU: the oracle's planner brakes early -- the smallest TTC of the run is 6.4 s in the first ticks, then the car settles 43 m behind --
# so the thresholds of this run sit where its measures are (ttc_thr 8 s: the approach is one incident, which closes once the car follows)
BEHAVIOUR = dict(gap=60.0, scale=0.2, ticks=200, vel=20.0, safety=dict(r_ego=1.5, ttc_thr=8.0, drac_thr=0.5, thw_thr=3.0, margin=1.0))


def run_behaviour(monteblanco, oracle_backend, tab, start, obj_pos, obj_vel):
    from oracle.planner_host import HostPlannerBackend
    s0 = float(tab.s_rl[int(np.argmin((tab.x - start['pos'][0]) ** 2 + (tab.y - start['pos'][1]) ** 2))])
    entry = dict(opponents=[(s0 + BEHAVIOUR["gap"], BEHAVIOUR["scale"], 5.0)], static=[], pref=("follow", "straight", "left", "right"),
                 pos_est=tuple(start['pos']), vel_est=BEHAVIOUR["vel"], zone_gids=[])
    loop = nu.NoisySimLoop(monteblanco, tab, [entry], [HostPlannerBackend(monteblanco).planner(1)], oracle=oracle_backend,
                           noise=sim.NoiseModel(1, 77, obj_pos=obj_pos, obj_vel=obj_vel))
    assert loop.set_start(0, start['pos'], start['heading'], BEHAVIOUR["vel"], start['max_heading_offset'])[0]
    loop.sim_vel(0, **sl.C2_VEL)
    m, truth = sim.SafetyModel(1, **BEHAVIOUR["safety"]), sim.SafetyModel(1, **BEHAVIOUR["safety"])
    ticks = []
    for k in range(BEHAVIOUR["ticks"]):
        r = loop.tick()[0]
        assert not r["failed"], (k, r.get("error"))
        # what the device's monitor is handed: TRUE positions, perceived displacements
        staged = [(v[2][0, 0], v[2][0, 1], v[2][1, 0], v[2][1, 1], v[0]) for v in r["veh"]]
        po, pt = m.step(0, r["pos"], sim.safety_objects(staged, r["true_xy"]), loop.dt)
        ticks.append(dict(per_obj=po, per_tick=pt, evaluated=k > 0))
        m.advance()
        # the drive itself: the same rule on the objects' TRUE velocities (the host loop knows them; the device's staging does not)
        kept = [o for o, keep in zip(r["true_objects"], r["keep"]) if keep]
        assert len(kept) == len(staged)
        truth.step(0, r["pos"], [(o[0], o[1], o[0] - 0.2 * o[3] * math.sin(o[2]), o[1] + 0.2 * o[3] * math.cos(o[2]), v[0])      # (heading 0 points along +y)
                                 for o, v in zip(kept, r["veh"])], loop.dt)
        truth.advance()
    return m, ticks, truth


def test_a_following_run_exercises_the_rule_and_a_worse_perception_scores_worse(monteblanco, oracle_backend):
    tab = sim.RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))
    start = pr.load_ticks("c2")[0]['start']
    m, ticks, truth = run_behaviour(monteblanco, oracle_backend, tab, start, 0.0, 0.0)
    d = m.as_dict()
    print("exact perception: %s" % {k: v[0].tolist() for k, v in d.items()})
    print("  incidents: %s" % sim.safety_incidents(m.inc[0], d["n_incidents"][0]))
    assert d["n_incidents"][0] >= 1 and (d["n_incidents"][0] >= 2 or d["inc_open"][0] == 0), "no closed incident"
    assert np.isfinite(d["ttc_min"][0]) and d["ticks_eval"][0] == BEHAVIOUR["ticks"] - 1
    assert any(t["evaluated"] and t["per_tick"][4] > 0.0 for t in ticks), "no tick with a positive required deceleration"
    assert any(t["evaluated"] and np.any(t["per_obj"][:, FLAGS].astype(int) & sim.SAF_CORRIDOR) for t in ticks), "never an object in the corridor"
    assert d["tet"][0] > 0.0 and d["hist"][0].sum() == d["ticks_eval"][0]
    # with exact perception the perceived velocity is the true one: the same incidents, the measures equal to rounding
    t = truth.as_dict()
    assert t["n_incidents"][0] == d["n_incidents"][0] and abs(t["ttc_min"][0] - d["ttc_min"][0]) < 1e-6 and t["gap_min"][0] == d["gap_min"][0]
    m2, _, truth2 = run_behaviour(monteblanco, oracle_backend, tab, start, 2.0, 8.0)
    d2, t2 = m2.as_dict(), truth2.as_dict()
    print("sigma obj_pos 2 m, obj_vel 8 m/s, as monitored: %s" % {k: v[0].tolist() for k, v in d2.items()})
    print("  on the objects' true velocities: %s" % {k: v[0].tolist() for k, v in t2.items()})
    assert d2["ttc_min"][0] < d["ttc_min"][0] or d2["tet"][0] > d["tet"][0], "the twin with the larger perception error did not score worse"
    # ... and not only because its monitor is fed noisier velocities: the drive itself was worse. On the TRUE object velocities the twin
    # still scores worse, and it came closer to the car ahead (the gap is measured on true positions in both records)
    assert t2["ttc_min"][0] < t["ttc_min"][0] or t2["tet"][0] > t["tet"][0], "on true velocities the twin did not score worse"
    assert t2["gap_min"][0] < t["gap_min"][0] and d2["gap_min"][0] == t2["gap_min"][0] and t2["thw_min"][0] < t["thw_min"][0]


# ---- 4. the entry points ------------------------------------------------------------------------------------------------------------------
def test_safety_entry_points_check_their_arguments_without_a_device():
    """The real library refuses a null fleet; tools/fakehip/sim_safety_args.py on the stand-in runtime (plain build): every bad argument is
    refused with a message that names it, without allocation or launch; a failing allocation keeps the previous monitor; a tick with the
    monitor on launches k_fleet_sim_safety once, a tick with it off never."""
    import sys
    lib = ctypes.CDLL(os.path.join(ROOT, "graphbasedlocaltrajectoryplanner_amd", "csrc", "libltpl_hip.so"))
    assert lib.ltpl_fleet_sim_safety(None, None) == 1 and lib.ltpl_fleet_sim_safety_read(None, None, 31, None, 6) == 1
    assert lib.ltpl_fleet_sim_safety_eval(None, 0, *([None] * 10)) == 1
    env = dict(os.environ, FAKEHIP_SAN="none", LTPL_NO_SELFTEST="1")
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "sim_safety_args.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and "sim safety args OK" in p.stdout, p.stdout[-3000:]
    assert "launches per tick" in p.stdout, p.stdout[-3000:]


# ---- 5. the field tables ------------------------------------------------------------------------------------------------------------------
def test_python_binding_and_header_declare_the_entry_points():
    from graphbasedlocaltrajectoryplanner_amd import fleet
    for name in ("sim_safety", "sim_safety_read", "sim_safety_eval"):
        assert callable(getattr(fleet.Fleet, name)), name
    with open(os.path.join(ROOT, "include", "ltpl_hip.h")) as fh:
        hdr = fh.read()
    for name in ("ltpl_fleet_sim_safety(", "ltpl_fleet_sim_safety_read(", "ltpl_fleet_sim_safety_eval(", "#define LTPL_ABI_VERSION 9",
                 "#define LTPL_FLEET_SIM_SAFETY_DOUBLES 31", "#define LTPL_FLEET_SIM_SAFETY_INCIDENTS 8", "#define LTPL_SIM_SAFETY_KEEP_STATE 1u"):
        assert name in hdr, name
    assert sim.SAFETY_DOUBLES == 31 == sim.SAFETY_FIELDS[-1][1] + sim.SAFETY_HIST and fleet.SAFETY_FIELDS is sim.SAFETY_FIELDS
    assert [f[1] for f in sim.SAFETY_FIELDS] == list(range(24)) and fleet.INCIDENT_FIELDS is sim.INCIDENT_FIELDS
    assert len(sim.INCIDENT_FIELDS) == sim.INCIDENT_DOUBLES == 6 and sim.SAFETY_INCIDENTS == 8
    assert set(sim.SAFETY_PARAMS) == set(sim.SAFETY_DEFAULTS) and len(sim.SAFETY_PARAMS) == 5
    assert [f[0] for f in fleet.SimSafetyIn._fields_] == ["on"] + list(sim.SAFETY_PARAMS) + ["tick0", "flags"]
    with pytest.raises(ValueError):
        sim.SafetyModel(1, bogus=1.0)
    assert math.isinf(sim.safety_start(2)[0][1, 8])
