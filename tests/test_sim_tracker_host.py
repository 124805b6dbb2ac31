"""
CPU: the object tracker of the fleet's simulation (ltpl_fleet_sim_tracker) off the device --

  1. csrc/fleet_track.hpp, compiled alone with the host compiler (-ffp-contract=off), equals the Python mirror sim.TrackerModel bit for bit
     on the case table of sim_tracker_util.cases: tables, lists handed on, assignments, counters and next_id;
  2. the rule on that table's sequences: the gate at equality and one ulp above (both outcomes occur), exact ties by track then
     detection, competition, w = 0 pass-through, n_confirm of 1, 2 and 3, n_coast of 0 and 3, a tentative track deleted on a miss,
     overflow at C_p, withholding at S_p, ids never reused, the counts 0, 1, 63, 64, 65, 96 with matches on both sides of slot 64;
  3. the header's own stand-alone program under -fsanitize=address,undefined (a plain executable) exits 0;
  4. closed loops on Monteblanco: behind a slow car with a dropout of 0.3 and n_coast = 3 the car is handed on through every gap of at
     most 3 ticks and the planner's actions differ from the run without a tracker; with n_confirm = 3 a car is handed on exactly two
     ticks later than without a tracker; the record's counters equal counts taken from the loop;
  5. the margins of the scenarios of the device differential: on the noisy one no pair lies within 1e-9 gate^2 of the gate and no two
     competing candidates differ by less than 1e-9 relative (the condition under which a noisy run may be compared); the others carry the
     same bits on both sides, exact ties included;
  6. the entry points check their arguments without a device.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import sim_tracker_util as tu
from graphbasedlocaltrajectoryplanner_amd import sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "sim_tracker_shim.cpp")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tracker") / "sim_tracker_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, SHIM], check=True)
    lib = ctypes.CDLL(so)
    D, P, I = ctypes.c_double, ctypes.c_void_p, ctypes.c_int
    lib.tracker_step_host.argtypes = [P, D, D, I, I, P, P, P, P, I, P, P, P, P]
    return lib


@pytest.fixture(scope="module")
def table_cases():
    cs, groups = tu.cases()
    return cs, groups, [tu.mirror(c) for c in cs]


def header(shim, c):
    """A case by the compiled header, in the form of sim_tracker_util.mirror."""
    cap, slots, T, K = c["cap"], c["slots"], c["tracks"].shape[0], c["dets"].shape[0]
    tab = np.full((sim.TRACK_CAP, sim.TRACK_DOUBLES), np.nan)
    tab[:T] = c["tracks"]
    par, dets = np.array(c["params"], float), np.ascontiguousarray(np.concatenate((c["dets"], np.zeros((1, 6)))))
    n, nid, n_out = ctypes.c_int(T), ctypes.c_double(c["next_id"]), ctypes.c_int(-1)
    out, assign, rec = np.zeros((slots + 1, 6)), np.zeros(K + 1, np.int32), np.zeros(sim.TRACKER_DOUBLES)
    shim.tracker_step_host(par.ctypes.data, c["adv"], float(c["tick"]), cap, slots, tab.ctypes.data, ctypes.addressof(n), ctypes.addressof(nid),
                           dets.ctypes.data, K, out.ctypes.data, ctypes.addressof(n_out), assign.ctypes.data, rec.ctypes.data)
    tab[n.value:] = np.nan
    return dict(table=tab, n_tracks=n.value, next_id=nid.value, out=out[:n_out.value].copy(), assign=assign[:K].tolist(), rec=rec)


# ---- 1. header against mirror -------------------------------------------------------------------------------------------------------------
def test_header_equals_the_mirror_bit_for_bit(shim, table_cases):
    cs, groups, ref = table_cases
    for i, (c, r) in enumerate(zip(cs, ref)):
        tu.compare(header(shim, c), r, "case %d" % i)
    # the counted scenes: every pair of counts, matches below and from slot 64 on, on the track's side and on the detection's
    seen, low_t, high_t, low_k, high_k = set(), 0, 0, 0, 0
    for i in groups["counts"]:
        c, r = cs[i], ref[i]
        seen.add((c["tracks"].shape[0], c["dets"].shape[0]))
        ids = c["tracks"][:, 6].astype(int).tolist()
        for k, a in enumerate(r["assign"]):
            if a >= 0:
                t = ids.index(a)
                low_t, high_t, low_k, high_k = low_t + (t < 64), high_t + (t >= 64), low_k + (k < 64), high_k + (k >= 64)
    edge = (0, 1, 63, 64, 65, 96)
    assert seen == {(t, k) for t in edge for k in edge}
    assert min(low_t, high_t, low_k, high_k) > 20, (low_t, high_t, low_k, high_k)
    total = np.sum([r["rec"] for r in ref], axis=0)
    print("case table: %d cases; counters %s" % (len(cs), dict(zip([f[0] for f in sim.TRACKER_FIELDS], total.astype(int).tolist()))))
    assert np.all(total[:11] > 0)                             # every counter moves somewhere on the table


# ---- 2. the rule --------------------------------------------------------------------------------------------------------------------------
def steps(table_cases, name):
    cs, groups, ref = table_cases
    return [(cs[i], ref[i]) for i in groups[name]]


def test_the_gate_at_equality_and_one_ulp_above(table_cases):
    eq, above, down = (steps(table_cases, "gate / " + n)[1] for n in ("equal", "one ulp above", "gate one ulp down"))
    g2 = 5.0 * 5.0
    assert 3.0 * 3.0 + 4.0 * 4.0 == g2 and 5.0 * 5.0 + 2.0 ** -24 * 2.0 ** -24 == np.nextafter(g2, np.inf)
    assert eq[1]["assign"] == [0] and eq[1]["rec"][2] == 1 and eq[1]["n_tracks"] == 1            # d2 == gate^2: accepted
    assert above[1]["assign"] == [sim.TRACK_UNMATCHED] and above[1]["rec"][2] == 0               # one ulp above: rejected, a new track
    assert above[1]["rec"][3] == 1 and above[1]["table"][0, 6] == 1.0                            # (n_coast = 0: the old one is gone)
    assert down[1]["assign"] == [sim.TRACK_UNMATCHED] and down[0]["params"][0] ** 2 < g2


def test_ties_and_competition(table_cases):
    _, (c, r) = steps(table_cases, "tie / tracks")
    assert r["assign"] == [0] and r["n_tracks"] == 1 and r["table"][0, 6] == 0.0                  # the lower track takes it, the other is gone
    _, (c, r) = steps(table_cases, "tie / detections")
    assert r["assign"] == [0, sim.TRACK_UNMATCHED] and r["table"][0, 0] == 1.0                    # the lower detection
    _, (c, r) = steps(table_cases, "tie / square")
    assert r["assign"] == [0, 1]                                                                   # (0, 0) first, then (1, 1) is what is left
    _, (c, r) = steps(table_cases, "compete / tracks")
    assert r["assign"] == [1] and r["rec"][2] == 1 and r["rec"][8] == 1 and r["n_tracks"] == 2    # the nearer track; the other coasts
    assert [o[0] for o in r["out"]] == [2.0, 0.0]                                                  # matched first, then the coasting one
    _, (c, r) = steps(table_cases, "compete / detections")
    assert r["assign"] == [sim.TRACK_UNMATCHED, 0] and r["n_tracks"] == 2
    _, (c, r) = steps(table_cases, "compete / greedy")
    assert r["assign"] == [1, 0]                                                                   # t1-d0 at 0.5 first, t0-d1 at 1.5 left


def test_w0_is_the_detection_and_the_filter_is_the_written_blend(table_cases):
    for c, r in steps(table_cases, "w0"):
        d = c["dets"][0]
        assert tu.equal_bits(r["out"][0], d)                                                       # x, y, px, py, r, v bitwise
        assert tu.equal_bits(r["table"][0, [0, 1, 4, 5]], d[[0, 1, 4, 5]])
    (c0, r0), (c1, r1), _ = steps(table_cases, "filter")
    d, old = c1["dets"][0], r0["table"][0]
    xp = old[0] + 0.5 * old[2]
    assert r1["table"][0, 0] == d[0] + 0.75 * (xp - d[0]) and r1["table"][0, 2] == (d[2] - d[0]) + 0.5 * (old[2] - (d[2] - d[0]))
    assert r1["table"][0, 5] == d[5] + 0.5 * (old[5] - d[5]) and r1["table"][0, 4] == d[4] and r1["table"][0, 7] == 2.0


def test_confirmation_coasting_and_tentative_tracks(table_cases):
    for nc in (1, 2, 3):
        outs = [len(r["out"]) for _, r in steps(table_cases, "confirm / %d" % nc)]
        assert outs == [0] * (nc - 1) + [1] * (4 - nc + 1) + [1, 0, 0], (nc, outs)                # from the nc-th tick; n_coast = 1 after the last
        assert sum(r["rec"][4] for _, r in steps(table_cases, "confirm / %d" % nc)) == 1
    for ncoast in (0, 3):
        st = steps(table_cases, "coast / %d" % ncoast)
        outs = [len(r["out"]) for _, r in st]
        assert outs == [1, 1] + [1] * ncoast + [0] * (6 - ncoast), (ncoast, outs)
        x_last = st[1][1]["out"][0][0]
        for j in range(1, ncoast + 1):                                                             # x + j adv ex, exactly (dyadic values)
            o = st[1 + j][1]["out"][0]
            assert o[0] == x_last + j * 0.5 * 1.0 and o[1] == 2.0 and o[2] == o[0] + 1.0 and st[1 + j][1]["rec"][8] == 1
        assert st[2 + ncoast][1]["rec"][6] == 1 and st[2 + ncoast][1]["n_tracks"] == 0
    st = steps(table_cases, "tentative")
    assert [len(r["out"]) for _, r in st] == [0, 0, 0, 0, 0, 1]
    assert st[2][1]["rec"][5] == 1 and st[2][1]["n_tracks"] == 0 and st[3][1]["table"][0, 6] == 1.0 and st[3][1]["table"][0, 9] == 3.0


def test_overflow_withholding_and_ids(table_cases):
    st = steps(table_cases, "overflow")
    assert st[0][0]["cap"] == 4 and st[0][0]["slots"] == 2
    assert st[1][1]["rec"][[3, 7, 8, 9, 10]].tolist() == [2, 2, 0, 2, 0] and st[1][1]["n_tracks"] == 4          # C, D born; A, B withheld
    assert st[2][1]["assign"] == [sim.TRACK_OVERFLOW] * 2 and st[2][1]["rec"][[3, 7, 8, 9, 10]].tolist() == [0, 2, 2, 2, 2]
    assert st[2][1]["next_id"] == 4.0                                                               # an overflow takes no id
    assert st[3][1]["assign"] == [sim.TRACK_OVERFLOW] and st[3][1]["rec"][8] == 2 and st[3][1]["rec"][9] == 2
    born = []
    for c, r in steps(table_cases, "ids"):
        before = set(c["tracks"][:, 6].astype(int).tolist())
        born += [i for i in r["table"][:r["n_tracks"], 6].astype(int).tolist() if i not in before]
    assert born == list(range(len(born))) and len(born) >= 5                                        # ascending, never reused


# ---- 3. sanitizers ------------------------------------------------------------------------------------------------------------------------
def test_the_stand_alone_program_runs_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sim_tracker_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DSIM_TRACKER_SHIM_MAIN", "-o", exe, SHIM], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert p.returncode == 0 and "tracker shim:" in p.stdout, p.stdout[-3000:]


# ---- 4. closed loops ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    return sim.RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


@pytest.fixture(scope="module")
def track():
    return np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz"))


@pytest.fixture(scope="module")
def c2_start():
    return pr.load_ticks("c2")[0]['start']


def slow_car_class(table, start, ahead=45.0):
    """The ego behind one slow car on the race line, ``ahead`` m in front of the start."""
    i0 = int(np.argmin((table.x - start['pos'][0]) ** 2 + (table.y - start['pos'][1]) ** 2))
    opp = [(float(table.s_rl[i0]) + ahead, 0.04, 5.0)]
    return dict(entry=dict(opponents=opp, static=[], pref=sl.DEFAULT_PREF, pos_est=tuple(start['pos']), vel_est=0.0, zone_gids=[]), vel=sl.C2_VEL)


def run_loop(lat, oracle, table, cls, start, ticks, sensor=None, tracker=None):
    from oracle.planner_host import HostPlannerBackend
    pl = [HostPlannerBackend(lat).planner(1)]
    loop = tu.TrackingSimLoop(lat, table, [cls["entry"]], pl, oracle=oracle, sensor=sensor, trackers=None if tracker is None else [tracker])
    assert loop.set_start(0, start['pos'], start['heading'], cls.get("start_vel", start['vel']), start['max_heading_offset'])[0]
    loop.sim_vel(**cls["vel"])
    return [loop.tick()[0] for _ in range(ticks)], loop


def test_closed_loop_behind_a_slow_car_with_dropouts(monteblanco, oracle_backend, table, c2_start):
    cls, ticks = slow_car_class(table, c2_start), 100

    def sensor():
        return sim.SensorModel(1, p_drop=0.3, seed=2025)
    bare, _ = run_loop(monteblanco, oracle_backend, table, cls, c2_start, ticks, sensor=sensor())
    trk = sim.TrackerModel(1, dt=0.05, gate=5.0, w_pos=0.5, w_vel=0.5, n_confirm=1, n_coast=3)
    recs, loop = run_loop(monteblanco, oracle_backend, table, cls, c2_start, ticks, sensor=sensor(), tracker=trk)
    assert not any(r["failed"] for r in recs) and not any(r["failed"] for r in bare)
    seen = [len(r["dets"]) for r in recs]
    assert all(len(r["veh_all"]) == 1 for r in recs) and 0 < sum(seen) < ticks
    gap, longest, expect = 0, 0, []
    for k, s in enumerate(seen):
        gap = 0 if s else gap + 1
        longest = max(longest, gap)
        expect.append(1 if (s or (gap <= 3 and any(seen[:k]))) else 0)
    assert [r["cnt"] for r in recs] == expect and longest > 3 and 0 in expect[5:], (seen, [r["cnt"] for r in recs])
    d = trk.as_dict()
    print({k: int(v[0]) for k, v in d.items()}, "longest gap", longest)
    print("without tracker:", [r["sel"] for r in bare][::5])
    print("with tracker:   ", [r["sel"] for r in recs][::5])
    assert [r["sel"] for r in recs] != [r["sel"] for r in bare]
    # the record against counts taken from the loop
    assert d["ticks"][0] == ticks and d["n_det"][0] == sum(seen) and d["n_out"][0] == sum(r["cnt"] for r in recs)
    assert d["n_out_coast"][0] == sum(r["cnt"] - r["out_live"] for r in recs) == sum(e and not s for e, s in zip(expect, seen))
    assert d["n_matched"][0] + d["n_born"][0] + d["n_overflow"][0] == d["n_det"][0] and d["n_born"][0] == d["n_confirmed"][0]
    assert d["n_matched"][0] == sum(a >= 0 for r in recs for a in r["assign"]) and d["n_withheld"][0] == 0 and d["tracks_max"][0] == 1
    assert d["n_born"][0] - d["n_del_coast"][0] - d["n_del_tentative"][0] == len(trk.tracks)


def test_a_car_entering_the_range_is_handed_on_two_ticks_later_with_n_confirm_3(monteblanco, oracle_backend, table, c2_start):
    cls, ticks = slow_car_class(table, c2_start, ahead=45.0), 100

    def sensor():
        return sim.SensorModel(1, range=44.0)
    bare, _ = run_loop(monteblanco, oracle_backend, table, cls, c2_start, ticks, sensor=sensor())
    trk = sim.TrackerModel(1, dt=0.05, gate=5.0, w_pos=0.0, w_vel=0.0, n_confirm=3, n_coast=0)
    recs, _ = run_loop(monteblanco, oracle_backend, table, cls, c2_start, ticks, sensor=sensor(), tracker=trk)
    first_bare, first = [r["cnt"] for r in bare].index(1), [r["cnt"] for r in recs].index(1)
    print("in range from tick %d; handed on from tick %d" % (first_bare, first))
    assert 0 < first_bare and first == first_bare + 2
    # (until then the two runs are the same run: the planner saw nothing in either)
    assert all(a["pos"] == b["pos"] and a["sel"] == b["sel"] for a, b in zip(bare[:first_bare + 1], recs[:first_bare + 1]))
    assert all(r["cnt"] == 1 for r in recs[first:first + 5]) and trk.as_dict()["n_confirmed"][0] >= 1


# ---- 5. margins of the device scenarios ---------------------------------------------------------------------------------------------------
def test_no_pair_of_the_device_scenarios_lies_on_the_gate_or_ties(monteblanco, oracle_backend, table, track, c2_start):
    import test_gpu_sim_differential as gd
    total = np.zeros(sim.TRACKER_DOUBLES)
    for name, units, skw, tkw, ticks, kind in tu.scenarios(table, track, c2_start):
        sc = gd.Scenario(monteblanco, table, units)
        loop = tu.host_loop(sc, oracle_backend, skw, tkw, kind)
        gate, comp = tu.INF, tu.INF
        for k in range(ticks):
            recs = loop.tick()
            assert not any(r["failed"] for r in recs), (name, k)
            g, c = tu.margins(recs)
            gate, comp = min(gate, g), min(comp, c)
        rec = np.sum([m.rec for m in loop.trackers], axis=0)
        print("%s: smallest |d2 - gate^2| / gate^2 = %.3g, smallest relative difference of competing candidates = %.3g; counters %s" % (
            name, gate, comp, rec.astype(int).tolist()))
        # without noise host and device see the same bits, and an exact tie (the crowd's opponents parked on one spot) is decided by the
        # rule's (t, k) order on both sides; with noise the inputs differ in the last bits, so no decision may hang on them
        if kind == "noise":
            assert gate > 1e-9 and comp > 1e-9, name
        else:
            assert gate > 0.0 and (comp == 0.0 or comp > 1e-9), name
        assert rec[2] > 0 and rec[3] > 0, name
        total += rec
    # over the scenarios: matches, births, confirmations, both deletions and coasting objects handed on
    assert np.all(total[[2, 3, 4, 5, 6, 8]] > 0), total


# ---- 6. the entry points ------------------------------------------------------------------------------------------------------------------
def test_tracker_entry_points_check_their_arguments_without_a_device():
    """The real library refuses a null fleet; tools/fakehip/sim_tracker_args.py on the stand-in runtime (plain build): every bad argument
    is refused with a message that names it, without allocation or launch; one more launch per tick while the tracker is set."""
    import sys
    lib = ctypes.CDLL(os.path.join(ROOT, "graphbasedlocaltrajectoryplanner_amd", "csrc", "libltpl_hip.so"))
    assert lib.ltpl_fleet_sim_tracker(None, None) == 1 and lib.ltpl_fleet_sim_tracker_read(None, None, 12, 0, None, None, None) == 1
    assert lib.ltpl_fleet_sim_tracker_eval(None, 0, *([None] * 16)) == 1
    env = dict(os.environ, FAKEHIP_SAN="none", LTPL_NO_SELFTEST="1")
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "sim_tracker_args.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and "sim tracker args OK" in p.stdout, p.stdout[-3000:]
    assert "launches per tick" in p.stdout, p.stdout[-3000:]


def test_python_binding_and_header_declare_the_entry_points():
    from graphbasedlocaltrajectoryplanner_amd import fleet
    for name in ("sim_tracker", "sim_tracker_read", "sim_tracker_eval"):
        assert callable(getattr(fleet.Fleet, name)), name
    with open(os.path.join(ROOT, "include", "ltpl_hip.h")) as fh:
        hdr = fh.read()
    for name in ("ltpl_fleet_sim_tracker(", "ltpl_fleet_sim_tracker_read(", "ltpl_fleet_sim_tracker_eval(", "#define LTPL_ABI_VERSION 9",
                 "#define LTPL_FLEET_SIM_TRACK_DOUBLES 10", "#define LTPL_FLEET_SIM_TRACKER_DOUBLES 12"):
        assert name in hdr, name
    assert sim.TRACKER_DOUBLES == 12 == len(sim.TRACKER_FIELDS) and sim.TRACK_DOUBLES == 10 == len(sim.TRACK_FIELDS)
    assert fleet.TRACKER_FIELDS is sim.TRACKER_FIELDS and set(sim.TRACKER_DEFAULTS) == set(sim.TRACKER_PARAMS)
    assert sim.tracker_capacity(8) == 16 and sim.tracker_capacity(48) == 96 and sim.tracker_capacity(96) == 96
