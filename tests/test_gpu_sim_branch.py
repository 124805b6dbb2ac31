"""
GPU: snapshot and branch of the fleet simulation's planner state on the device (ltpl_fleet_sim_snapshot / _snapshot_info / _snapshot_drop /
ltpl_fleet_sim_branch, include/ltpl_hip.h; csrc/fleet_branch.hpp: k_fleet_sim_branch) -- held to BIT EQUALITY against the simulation itself
(a planner that took another's state runs like it; a restored fleet runs its ticks again), against the reference's recordings
(tests/test_gpu_fleet_sim.check_trace) and against the host loop of tests/sim_loop.py over the oracle's planner.

"Bitwise" is ``tobytes()`` equality of all 52 trace doubles of every tick (digest included), of ``sim_state()``, ``sim_heading()`` and
``digest()``, and of the telemetry records where telemetry is on. Every test calls an entry point the parent commit does not have.
"""
import os

import numpy as np
import pytest

import friction_replay as fr
import planner_replay as pr
import sim_loop as sl
import test_gpu_fleet_sim as gs
import test_gpu_friction as gf
import test_gpu_sim_differential as gd
from fleet_differential import same_paths, same_trajectories

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip(monteblanco):
    from graphbasedlocaltrajectoryplanner_amd import _capi
    return _capi.HipBackend(monteblanco)


@pytest.fixture(scope="module")
def table():
    from graphbasedlocaltrajectoryplanner_amd.sim import RaceLineTable
    return RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


@pytest.fixture(scope="module")
def c2():
    return pr.load_ticks("c2")


@pytest.fixture(scope="module")
def classes(table, c2):
    return sl.monteblanco_classes(table, np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")), tuple(c2[0]['start']['pos']))


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def same(a, b):
    """Bitwise equality of two values of ``paths()`` / ``trajectories()`` / ``sim_state()``: arrays by their bytes, containers element-wise."""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, (np.ndarray, float, np.floating)):
        x, y = np.asarray(a), np.asarray(b)
        return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
    return a == b


def opp_offsets(entries):
    return np.concatenate(([0], np.cumsum([len(e.get("opponents", ())) for e in entries]))).astype(int)


def state_of(fleet, off, p):
    """Everything ``sim_state`` / ``sim_heading`` / ``digest`` hold of planner ``p`` (``off``: opponent offsets of the fleet)."""
    st, a, b = fleet.sim_state(), off[p], off[p + 1]
    return dict(pos=st['pos_est'][p].copy(), vel=st['vel_est'][p:p + 1].copy(), sel=st['sel_action'][p:p + 1].copy(), now=st['now'][p:p + 1].copy(),
                opp_s=st['opp_s'][a:b].copy(), opp_tic=st['opp_tic'][a:b].copy(), heading=fleet.sim_heading()[p:p + 1].copy(),
                digest=fleet.digest()[p].copy())


def same_rows(trace, p, other, q, what):
    """Trace of planner ``p`` bitwise that of planner ``q`` of ``other`` on every tick."""
    a, b = np.ascontiguousarray(trace[:, p]), np.ascontiguousarray(other[:, q])
    if a.tobytes() != b.tobytes():
        bad = np.argwhere((a != b) & ~(np.isnan(a) & np.isnan(b)))
        raise AssertionError("%s: planner %d differs from planner %d first at (tick, field) %s: %r vs %r" % (
            what, p, q, bad[0] if len(bad) else "(sign / NaN payload)", a[tuple(bad[0])] if len(bad) else None, b[tuple(bad[0])] if len(bad) else None))


def build(hip, table, entries, starts, vels, races=None):
    """A fleet of ``entries`` (Fleet.sim_setup) started at ``starts`` [(pos, heading, vel, max_heading_offset)] with the velocity arguments
    ``vels`` (one dict per planner, grouped as test_gpu_sim_differential.Scenario.fleet does)."""
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    fleet = Fleet(hip, len(entries))
    for p, (pos, heading, vel, mho) in enumerate(starts):
        assert fleet.set_start(p, pos, heading, vel, mho)[0], p
    fleet.sim_setup(table, entries)
    if races:
        fleet.sim_race(races, length=5.0)
    set_vels(fleet, vels)
    return fleet


def set_vels(fleet, vels):
    uniq, idx = [], []
    for p, v in enumerate(vels):
        for u, q in zip(uniq, idx):
            if u is v or gs.same_vel(u, v):
                q.append(p)
                break
        else:
            uniq.append(v)
            idx.append([p])
    gs.set_vel(fleet, [[{'vel_args': v}] for v in uniq], idx, 0)


def recorded_start(ticks):
    st = ticks[0]['start']
    return (st['pos'], st['heading'], st['vel'], st['max_heading_offset'])


def elsewhere(table, s):
    pos, heading = sl.race_line_pose(table, s)
    return (pos, heading, 0.0, np.pi / 4)


def healthy(fleet):
    return bool(np.all(fleet.digest()[:, 0] == 0))


# ---- 1. branch against the recording ----------------------------------------------------------------------------------------------------
def test_a_branched_planner_follows_the_recording_of_its_source(hip, monteblanco, table, c2, classes):
    """p = 0 drives the c2 recording; q = 3 has p's configuration and was started elsewhere. Between them a planner without opponents and
    one with a single opponent (q's opponents lie at offset 9, p's at 0); planner 4 is a third c2 planner. q's opponents were started
    5 m ahead of p's (same speeds and lengths: the configuration), so their positions differ from p's when the branch comes and a copy
    to a wrong offset would show. After 40 ticks q takes p's state: from then on q is p, bit for bit, and so follows the recording; the
    others never notice."""
    e = gs.planner_entry(monteblanco, "c2", c2)
    far = elsewhere(table, 900.0)
    ahead = [(s0 + 5.0, scale, length) for s0, scale, length in e["opponents"]]
    entries = [e, classes["empty"]["entry"], classes["one"]["entry"], dict(e, pos_est=far[0], opponents=ahead),
               dict(e, pos_est=elsewhere(table, 1500.0)[0])]
    starts = [recorded_start(c2), recorded_start(c2), recorded_start(c2), far, elsewhere(table, 1500.0)]
    vels = [gs.vel_of(c2[0])] * 5
    off = opp_offsets(entries)
    assert off[3] != off[0] and off[2] - off[1] == 0 and off[3] - off[2] == 1 and off[4] - off[3] == off[1] - off[0] == 8
    p, q, others = 0, 3, [1, 2, 4]
    fleet, control = build(hip, table, entries, starts, vels), build(hip, table, entries, starts, vels)
    t1, c1 = gd.run_one(fleet, 40), gd.run_one(control, 40)
    assert healthy(fleet) and not same(state_of(fleet, off, p), state_of(fleet, off, q))
    assert np.all(state_of(fleet, off, p)["opp_s"] != state_of(fleet, off, q)["opp_s"])              # every opponent of q stands elsewhere
    assert fleet.sim_branch(p, q) >= 0.0
    assert same(fleet.paths(q), fleet.paths(p)) and same(fleet.trajectories(q), fleet.trajectories(p))
    assert same(state_of(fleet, off, q), state_of(fleet, off, p))
    for o in others + [p]:
        assert same(state_of(fleet, off, o), state_of(control, off, o)), o
    t2, c2t = gd.run_one(fleet, 40), gd.run_one(control, 40)
    same_rows(t2, q, t2, p, "after the branch")
    assert same(state_of(fleet, off, q), state_of(fleet, off, p)) and healthy(fleet)
    gs.check_trace(t2, c2[40:80], [p, q], "branched c2")
    for o in others + [p]:
        same_rows(t1, o, c1, o, "before the branch")
        same_rows(t2, o, c2t, o, "bystander after the branch")
    assert np.ascontiguousarray(c2t[:, q]).tobytes() != np.ascontiguousarray(c2t[:, p]).tobytes()      # (without the branch q drives its own way)
    fleet.close(); control.close()


# ---- 2. shapes of the pair list -----------------------------------------------------------------------------------------------------------
def one_opponent_fleet(hip, table, classes, c2, poses):
    """Planner i at arc length poses[i] with one opponent far behind it, started at 50 + 2 i m: every planner's opponent stands elsewhere."""
    starts = [elsewhere(table, s) for s in poses]
    entries = [dict(classes["one"]["entry"], opponents=[(50.0 + 2.0 * i, 0.35, 5.0)], pos_est=st[0]) for i, st in enumerate(starts)]
    return build(hip, table, entries, starts, [sl.C2_VEL] * len(entries)), opp_offsets(entries)


def branch_pairs(fleet, off, pairs):
    """``sim_branch`` of ``pairs`` [(src, dst)] in one call; before it the opponents of every dst stand elsewhere than its source's."""
    for s, d in pairs:
        a, b = state_of(fleet, off, s), state_of(fleet, off, d)
        assert a["opp_s"].size and np.all(a["opp_s"] != b["opp_s"]) and not same(a["pos"], b["pos"]), (s, d)
    fleet.sim_branch([s for s, _ in pairs], [d for _, d in pairs])


def check_pairs(fleet, off, pairs, n_ticks, what):
    """After ``sim_branch`` of ``pairs`` [(src, dst)]: every dst holds its source's state and runs like it for ``n_ticks``."""
    for s, d in pairs:
        assert same(state_of(fleet, off, d), state_of(fleet, off, s)), "%s: state of %d after taking %d's" % (what, d, s)
    tr = gd.run_one(fleet, n_ticks)
    for s, d in pairs:
        same_rows(tr, d, tr, s, what)
        assert same(state_of(fleet, off, d), state_of(fleet, off, s)), "%s: state of %d, %d ticks after taking %d's" % (what, d, n_ticks, s)
    assert healthy(fleet)
    return tr


def test_shapes_of_the_pair_list(hip, table, classes, c2):
    """One pair; then in ONE call a fan-out of one source into 9 destinations, a pair with src > dst and one with src < dst, the fleet's
    first and last planner among the destinations; then 65 pairs (more than 64) in a fleet of 70."""
    fleet, off = one_opponent_fleet(hip, table, classes, c2, [300.0 + 100.0 * i for i in range(16)])
    gd.run_one(fleet, 15)
    digests = fleet.digest()
    assert healthy(fleet) and len(set(digests[p].tobytes() for p in range(16))) == 16                # sixteen different states
    branch_pairs(fleet, off, [(5, 6)])
    check_pairs(fleet, off, [(5, 6)], 10, "one pair")
    fan = [0, 1, 2, 3, 4, 11, 12, 13, 15]
    pairs = [(7, d) for d in fan] + [(10, 8), (9, 14)]
    branch_pairs(fleet, off, pairs)
    tr = check_pairs(fleet, off, pairs, 10, "fan-out and single pairs")
    assert np.ascontiguousarray(tr[:, 7]).tobytes() != np.ascontiguousarray(tr[:, 9]).tobytes()
    assert fleet.sim_branch(7, fan) >= 0.0                                                            # (a scalar source is broadcast)
    fleet.close()
    fleet, off = one_opponent_fleet(hip, table, classes, c2, [300.0 + 300.0 * i for i in range(5)] + [2000.0] * 65)
    gd.run_one(fleet, 10)
    pairs = [(d % 5, d) for d in range(5, 70)]
    assert len(pairs) == 65
    branch_pairs(fleet, off, pairs)
    check_pairs(fleet, off, pairs, 10, "65 pairs")
    fleet.close()


# ---- 3. more than 64 opponents ------------------------------------------------------------------------------------------------------------
def test_a_pair_with_70_opponents(hip, table, classes, c2):
    """The opponents' positions and clocks are copied one lane per opponent: 70 of them cross lane 64. The destination's opponents were
    started 3 m behind the source's, and the first branch comes from a snapshot five ticks old, so that every opponent's tic and every moving
    opponent's s of the destination differ from what it is handed -- beyond lane 64 as well; then the same from the live fleet."""
    c = classes["crowded70"]
    assert len(c["entry"]["opponents"]) == 70
    far = elsewhere(table, 100.0)
    behind = [(s0 - 3.0, scale, length) for s0, scale, length in c["entry"]["opponents"]]
    entries = [c["entry"], classes["one"]["entry"], dict(c["entry"], pos_est=far[0], opponents=behind)]
    starts = [recorded_start(c2), recorded_start(c2), far]
    off = opp_offsets(entries)
    fleet = build(hip, table, entries, starts, [c["vel"], classes["one"]["vel"], c["vel"]])
    gd.run_one(fleet, 5)
    fleet.sim_snapshot(0, [0])
    at5 = state_of(fleet, off, 0)
    tr_a = gd.run_one(fleet, 5)                                                 # ticks 5 .. 9
    bystander, dst = state_of(fleet, off, 1), state_of(fleet, off, 2)
    # (the class parks some opponents with speed factor 0 beyond the end of the lap: those wrap to s = 0 on both sides and stay there)
    moving = np.array([scale > 0.0 for _, scale, _ in behind])
    assert dst["opp_s"].size == 70 and moving[64:].sum() >= 4 and moving[:64].sum() >= 40
    assert np.all(dst["opp_tic"][64:] != at5["opp_tic"][64:]) and np.all(dst["opp_tic"][:64] != at5["opp_tic"][:64])
    assert np.all((dst["opp_s"] != at5["opp_s"])[moving])
    fleet.sim_branch(0, 2, snapshot=0)
    got = state_of(fleet, off, 2)
    assert same(got["opp_s"], at5["opp_s"]) and same(got["opp_tic"], at5["opp_tic"]) and same(got, at5)
    assert same(state_of(fleet, off, 1), bystander)
    tr_b = gd.run_one(fleet, 5)                                                 # planner 2 lives planner 0's ticks 5 .. 9
    same_rows(tr_b, 2, tr_a, 0, "70 opponents from a snapshot")
    # ... and from the live fleet: planner 0 is at its tick 15, planner 2 at tick 10 of the same course
    src, dst = state_of(fleet, off, 0), state_of(fleet, off, 2)
    assert np.any(dst["opp_s"][64:] != src["opp_s"][64:]) and np.all(dst["opp_tic"][64:] != src["opp_tic"][64:])     # (parked ones stand still)
    fleet.sim_branch(0, 2)
    assert same(fleet.paths(2), fleet.paths(0)) and same(fleet.trajectories(2), fleet.trajectories(0))
    check_pairs(fleet, off, [(0, 2)], 5, "70 opponents")
    fleet.close()


# ---- 4. snapshot round trip -----------------------------------------------------------------------------------------------------------------
def mixed_fleet(hip, monteblanco, table, c2):
    """c2 planners around the recorded race 'race3_mixed', the last planner on the friction grid; telemetry on."""
    race = gd.recorded_race("race3_mixed")
    e = gs.planner_entry(monteblanco, "c2", c2)
    entries = [e] + race["entries"] + [e, e]
    starts = [recorded_start(c2)] + race["starts"] + [recorded_start(c2), elsewhere(table, 900.0)]
    entries[-1] = dict(e, pos_est=starts[-1][0])
    vels = [gs.vel_of(c2[0])] + race["vels"] + [gs.vel_of(c2[0])] * 2
    fleet = build(hip, table, entries, starts, vels, races=[1, len(race["entries"]), 1, 1])
    n = len(entries)
    fleet.friction(fr.load_grid(), map_idx=[-1] * (n - 1) + [0])
    fleet.sim_telemetry(radius=2.5)
    return fleet, n, opp_offsets(entries)


def whole_state(fleet, off, n):
    return [state_of(fleet, off, p) for p in range(n)]


def test_snapshot_round_trip(hip, monteblanco, table, c2):
    """60 ticks, snapshot, 40 ticks (A), restore, the same 40 ticks again (B): A == B bitwise, telemetry included -- only clear_tick, where
    it was set inside the window, names the tick that was executed: 40 later. A second slot taken next to the first is left alone."""
    fleet, n, off = mixed_fleet(hip, monteblanco, table, c2)
    gd.run_one(fleet, 60)
    assert healthy(fleet)
    fleet.sim_snapshot(0)
    info0 = fleet.sim_snapshot_info(0)
    assert info0["planners"].tolist() == list(range(n)) and info0["bytes"] > 0 and fleet.sim_snapshot_info(1) is None
    at60, tele60 = whole_state(fleet, off, n), fleet.sim_telemetry_read()
    A = gd.run_one(fleet, 40)
    stA, teleA = whole_state(fleet, off, n), fleet.sim_telemetry_read()
    assert not same(stA, at60)
    fleet.sim_snapshot(1)
    info1 = fleet.sim_snapshot_info(1)
    assert info1["bytes"] == info0["bytes"] and info1["planners"].tolist() == list(range(n))
    assert fleet.sim_restore(0) >= 0.0
    assert same(whole_state(fleet, off, n), at60) and same(fleet.sim_telemetry_read(), tele60)
    assert same(fleet.sim_snapshot_info(1), info1) and same(fleet.sim_snapshot_info(0), info0)
    B = gd.run_one(fleet, 40)
    assert A.tobytes() == B.tobytes(), np.argwhere((A != B) & ~(np.isnan(A) & np.isnan(B)))[:4]
    assert same(whole_state(fleet, off, n), stA)
    teleB = fleet.sim_telemetry_read()
    moved = 0
    for key in teleA:
        if key == "clear_tick":
            inside = teleA[key] >= 60                                           # set in fleet ticks 60 .. 99; the second time in 100 .. 139
            assert np.all(teleA[key][inside] < 100) and np.array_equal(teleB[key], np.where(inside, teleA[key] + 40, teleA[key])), (teleA[key], teleB[key])
            moved = int(inside.sum())
        else:
            assert same(teleB[key], teleA[key]), key
    assert moved > 0                                                            # (the rule above was put to the test)
    print("\nsnapshot round trip: %d planners, %d bytes per slot, clear_tick moved for %d planners" % (n, info0["bytes"], moved))
    # slot 1 holds tick 100: the fleet can go there as well
    fleet.sim_restore(1)
    assert same(whole_state(fleet, off, n), stA)
    fleet.sim_snapshot_drop(0)
    assert fleet.sim_snapshot_info(0) is None and same(fleet.sim_snapshot_info(1), info1)
    fleet.close()


# ---- 5. subset snapshot, branch from a snapshot ---------------------------------------------------------------------------------------------
def test_subset_snapshot_and_branch_from_a_snapshot(hip, table, classes, c2):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    poses = [300.0 + 200.0 * i for i in range(8)]
    fleet, off = one_opponent_fleet(hip, table, classes, c2, poses)
    control, _ = one_opponent_fleet(hip, table, classes, c2, poses)
    slot, rest = 6, [0, 2, 3, 5, 7]
    gd.run_one(fleet, 30)
    fleet.sim_snapshot(slot, [4, 1])
    assert fleet.sim_snapshot_info(slot)["planners"].tolist() == [4, 1]
    at30 = {p: state_of(fleet, off, p) for p in (1, 4)}
    orig = gd.run_one(fleet, 40)                                                # ticks 30 .. 69
    ctl = np.concatenate([gd.run_one(control, 30), gd.run_one(control, 40)])
    same_rows(orig, 6, ctl[30:], 6, "before the restore")
    fleet.sim_restore(slot)
    for p in (1, 4):
        assert same(state_of(fleet, off, p), at30[p]), p
    for p in rest + [6]:
        assert same(state_of(fleet, off, p), state_of(control, off, p)), p        # only planners 1 and 4 changed
    with pytest.raises(BackendError, match="pair 0 .src 2, dst 6.: the source is not a planner of snapshot 6"):
        fleet.sim_branch(2, 6, snapshot=slot)
    fleet.sim_branch(1, 6, snapshot=slot)
    assert same(state_of(fleet, off, 6), at30[1])
    again, ctl2 = gd.run_one(fleet, 20), gd.run_one(control, 20)                 # fleet ticks 70 .. 89; planners 1, 4 and 6 live their ticks 30 .. 49
    for p, src in ((1, 1), (4, 4), (6, 1)):
        same_rows(again, p, orig[:20], src, "ticks 31 .. again")                  # (the clock is per planner and travels with the state)
    for p in rest:
        same_rows(again, p, ctl2, p, "bystander")
    assert healthy(fleet)
    fleet.close(); control.close()


# ---- 6. row windows and a backup plan -----------------------------------------------------------------------------------------------------
def test_branch_inside_the_loss_of_grip_of_gridmapdrop(hip, monteblanco, table):
    """'gridmapdrop' in the simulation (set-up of test_gpu_friction.test_sim_run_reproduces_the_grid_recordings): the grid's scale drops to 0.3
    at tick 280; at tick 300 the backup branch is active (test_gpu_friction.test_emergency_profile_on_a_backup_tick_of_a_map_planner) and
    the planner's memory holds friction rows of its own in its row window. q = 2 (started elsewhere, a planner with an opponent between)
    takes p's state there and follows the recording through ticks 300 .. 339. (The recording fixes the 300 ticks in front.)"""
    ticks = pr.load_ticks("gridmapdrop")
    K, T = 300, 340
    assert ticks[279]['grid_scale'] == 1.0 and ticks[K]['grid_scale'] == 0.3
    e = fr.planner_entry(monteblanco, "gridmapdrop", ticks)
    far = elsewhere(table, 900.0)
    entries = [e, dict(e, opponents=[(1500.0, 0.35, 5.0)]), dict(e, pos_est=far[0])]
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    fleet = Fleet(hip, 3)
    for p, st in enumerate([recorded_start(ticks), recorded_start(ticks), far]):
        assert fleet.set_start(p, *st)[0]
    fleet.sim_setup(table, entries)
    fleet.friction(fr.load_grid())
    off = opp_offsets(entries)
    cuts = sorted(set([a for a, _ in gf.cuts_of([ticks], T)] + [K, T]))
    traces = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a == K:
            assert not same(state_of(fleet, off, 2), state_of(fleet, off, 0))
            fleet.sim_branch(0, 2)
            assert same(fleet.paths(2), fleet.paths(0)) and same(fleet.trajectories(2), fleet.trajectories(0))
        gf.set_vel(fleet, [ticks], [range(3)], a)
        fleet.friction_scale(ticks[a]['grid_scale'])
        traces.append(gd.run_one(fleet, b - a))
    trace = np.concatenate(traces)
    assert trace.shape[0] == T and healthy(fleet)
    same_rows(trace[K:], 2, trace[K:], 0, "inside the loss of grip")
    assert np.ascontiguousarray(trace[:K, 2]).tobytes() != np.ascontiguousarray(trace[:K, 0]).tobytes()
    gs.check_trace(trace[K:], ticks[K:T], [0, 2], "gridmapdrop from tick %d" % K)
    gs.check_trace(trace[:K], ticks[:K], [0], "gridmapdrop")
    assert same(state_of(fleet, off, 2), state_of(fleet, off, 0))
    fleet.close()


# ---- 7. revival ---------------------------------------------------------------------------------------------------------------------------
def test_a_failed_planner_is_revived(hip, table, classes, c2):
    """Planner 1 accepts 'straight' only and has an opponent right in front: its second tick offers 'follow' and 'right', and it stops
    with E_SIM_ACTION -- the simulation's own outcome. Its state from before the run, restored for it alone, clears its error word: it
    lives its first tick again (and stops again, its preference list being what it is). With the state of its neighbour 0, whose
    opponent is far away, 'straight' stays on offer: it keeps running, bitwise like the neighbour; the fleet's status is clean."""
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    base = classes["one"]["entry"]
    entries = [dict(base, opponents=[(1500.0, 0.35, 5.0)], pref=("straight", "follow")), dict(base, opponents=[(250.0, 0.35, 5.0)], pref=("straight",)),
               dict(base, opponents=[(1500.0, 0.35, 5.0)], pref=("straight", "follow"))]
    off = opp_offsets(entries)
    fleet = build(hip, table, entries, [recorded_start(c2)] * 3, [sl.C2_VEL] * 3)
    fleet.sim_snapshot(0, [1])
    with pytest.raises(BackendError, match="planner 1: closed-loop simulation"):
        fleet.sim_run(6)
    first = fleet.last_trace
    assert first[0, 1, 8] == 0 and np.all(first[1:, 1, 8] != 0) and fleet.digest()[1, 0] != 0 and np.all(first[:, [0, 2], 8] == 0)
    fleet.sim_restore(0)
    assert fleet.digest()[1, 0] == 0 and healthy(fleet)
    with pytest.raises(BackendError, match="planner 1: closed-loop simulation"):
        fleet.sim_run(2)
    again = fleet.last_trace
    same_rows(again, 1, first[:2], 1, "the first ticks again")
    assert again[0, 1, 8] == 0 and again[1, 1, 8] != 0
    same_rows(again, 0, again, 2, "the healthy neighbours")
    fleet.sim_branch(0, 1)
    assert healthy(fleet) and same(state_of(fleet, off, 1), state_of(fleet, off, 0))
    tr, ms = fleet.sim_run(30)                                                   # raises nothing: the fleet's status is clean again
    assert np.all(tr[:, :, 8] == 0) and healthy(fleet)
    same_rows(tr, 1, tr, 0, "revived")
    # ... and a failed source fails its destination
    fleet.sim_snapshot(1, [1])
    fleet.sim_restore(0)
    with pytest.raises(BackendError, match="planner 1: closed-loop simulation"):
        fleet.sim_run(2)
    fleet.sim_branch(1, 2)
    assert fleet.digest()[2, 0] != 0 and fleet.digest()[2, 0] == fleet.digest()[1, 0]
    fleet.sim_branch(1, 2, snapshot=1)
    assert fleet.digest()[2, 0] == 0
    fleet.close()


# ---- 8. the copied state is complete: lockstep against the host loop ---------------------------------------------------------------------------
def lockstep_ticks(fleet, loop, hmap, off, n_ticks, prev_traj, what):
    """``n_ticks`` ticks of the lockstep differential of tests/test_gpu_sim_differential.py (its bounds: discrete results exact, floats
    within 1e-12) with host planner h seated on device planner hmap[h]. Returns the device's trace."""
    from graphbasedlocaltrajectoryplanner_amd.planner import KEY_IDS, KEY_NAMES
    traces = []
    for k in range(n_ticks):
        st, th = fleet.sim_state(), fleet.sim_heading()
        for h, p in enumerate(hmap):
            a, b = off[p], off[p + 1]
            loop.seat(h, st['now'][p], st['pos_est'][p], st['vel_est'][p], th[p], st['opp_s'][a:b], st['opp_tic'][a:b], prev_traj[h])
        tr = gd.run_one(fleet, 1)[0]
        traces.append(tr.copy())
        st2, th2 = fleet.sim_state(), fleet.sim_heading()
        recs = loop.step_sim()
        post = {}
        for h, p in enumerate(hmap):
            w, r = "%s tick %d planner %d" % (what, k, p), recs[h]
            assert not r["failed"] and tr[p, 8] == 0, "%s: failed (host %s, device error word %s)" % (w, r["failed"], tr[p, 8])
            assert tr[p, 0] == KEY_IDS[r["sel"]] and st2['sel_action'][p] == KEY_IDS[r["sel"]], "%s: action %s vs %s" % (w, tr[p, 0], r["sel"])
            assert tr[p, 1] == r["now"] == st2['now'][p], "%s: clock" % w
            a, b = off[p], off[p + 1]
            d = dict(pos=float(np.max(np.abs(st2['pos_est'][p] - r["pos"]))), vel=abs(st2['vel_est'][p] - r["vel"]) / max(abs(r["vel"]), 1.0),
                     heading=float(gd.wrapped(th2[p] - r["theta"])), opp_s=float(np.max(np.abs(st2['opp_s'][a:b] - r["opp_s"]))),
                     opp_tic=float(np.max(np.abs(st2['opp_tic'][a:b] - r["opp_tic"]))))
            for q, v in d.items():
                assert v <= gd.TOL, "%s: %s differs by %g" % (w, q, v)
            assert np.array_equal(tr[p, 2:5], [st2['pos_est'][p, 0], st2['pos_est'][p, 1], st2['vel_est'][p]]), "%s: trace vs state" % w
            post[h] = dict(sel=KEY_NAMES.get(int(st2['sel_action'][p])), now=st2['now'][p], pos=st2['pos_est'][p], vel=st2['vel_est'][p], theta=th2[p])
        recs = loop.step_plan(post=post, want_paths=True)
        for h, p in enumerate(hmap):
            w, r = "%s tick %d planner %d" % (what, k, p), recs[h]
            assert not r["failed"], "%s: error on the host only (%s)" % (w, r.get("error"))
            assert tr[p, 5] == r["cnt"], "%s: on-track objects %s vs %d" % (w, tr[p, 5], r["cnt"])
            if r["cnt"]:
                assert float(np.max(np.abs(tr[p, 6:8] - r["first"]))) <= gd.TOL, "%s: first vehicle %s vs %s" % (w, tr[p, 6:8], r["first"])
            else:
                assert np.all(np.isnan(tr[p, 6:8])), w
            same_paths(fleet.paths(p), r["paths"], exact=False, what=w)
            dev_traj = fleet.trajectories(p)
            same_trajectories(dev_traj, r["traj"], exact=False, what=w)
            prev_traj[h] = dev_traj[0]
    return np.array(traces)


def test_branched_planners_with_other_arguments_against_the_host_loop(hip, monteblanco, oracle_backend, table, classes, c2):
    """p = 0 runs 40 ticks; q1 = 2 and q2 = 3 (started elsewhere) take its state and get another vel_max / gg_scale / machine table through
    sim_vel. Two host planners (the oracle's) lived p's 40 ticks in lockstep with p; from the branch on they are seated on q1 and q2 with
    the new arguments, for 30 ticks and without a tick skipped. A state copied incompletely would part from the host, which holds p's
    planner memory by its own arithmetic. q1 and q2 must leave p's course."""
    from oracle.planner_host import HostPlannerBackend
    c = classes["one"]
    far = elsewhere(table, 900.0)
    entries = [c["entry"], classes["empty"]["entry"], dict(c["entry"], pos_est=far[0]), dict(c["entry"], pos_est=elsewhere(table, 1400.0)[0])]
    starts = [recorded_start(c2), recorded_start(c2), far, elsewhere(table, 1400.0)]
    off = opp_offsets(entries)
    fleet = build(hip, table, entries, starts, [c["vel"]] * 4)
    backend = HostPlannerBackend(monteblanco)
    loop = sl.HostSimLoop(monteblanco, table, [c["entry"]] * 2, [backend.planner(1) for _ in range(2)], oracle=oracle_backend)
    for h in range(2):
        assert loop.set_start(h, *recorded_start(c2))[0]
        loop.sim_vel(h, **c["vel"])
    prev = [None, None]
    lockstep_ticks(fleet, loop, [0, 0], off, 40, prev, "before the branch")
    fleet.sim_branch(0, [2, 3])
    new = [sl.VEL_VARIANTS[0], sl.VEL_VARIANTS[3]]                              # vel_max 60 and gg_scale 0.8; a machine table of three rows and gg_scale 0.9
    set_vels(fleet, [c["vel"], c["vel"]] + new)
    for h in range(2):
        loop.sim_vel(h, **new[h])
    tr = lockstep_ticks(fleet, loop, [2, 3], off, 30, prev, "after the branch")
    for q in (2, 3):
        assert np.ascontiguousarray(tr[:, q, 2:5]).tobytes() != np.ascontiguousarray(tr[:, 0, 2:5]).tobytes(), "planner %d drives like its source" % q
    assert np.ascontiguousarray(tr[:, 2]).tobytes() != np.ascontiguousarray(tr[:, 3]).tobytes() and healthy(fleet)
    fleet.close()


# ---- 9. two fleets on one handle ----------------------------------------------------------------------------------------------------------
def test_snapshots_belong_to_their_fleet(hip, table, classes, c2):
    a, off = one_opponent_fleet(hip, table, classes, c2, [300.0, 600.0, 900.0])
    b, _ = one_opponent_fleet(hip, table, classes, c2, [300.0, 600.0, 900.0])
    gd.run_one(a, 5)
    a.sim_snapshot(0, [2, 0])
    a.sim_snapshot(3)
    assert b.sim_snapshot_info(0) is None and b.sim_snapshot_info(3) is None
    b.sim_snapshot(0, [1])
    assert a.sim_snapshot_info(0)["planners"].tolist() == [2, 0] and b.sim_snapshot_info(0)["planners"].tolist() == [1]
    tr_b, tr_a = gd.run_one(b, 5), gd.run_one(a, 5)
    b.sim_restore(0)
    a.sim_restore(3)
    again_a, again_b = gd.run_one(a, 5), gd.run_one(b, 5)
    for p in range(3):
        same_rows(again_a, p, tr_a, p, "fleet a again")
    same_rows(again_b, 1, tr_b, 1, "fleet b again")
    assert np.ascontiguousarray(again_b[:, 0]).tobytes() != np.ascontiguousarray(tr_b[:, 0]).tobytes()       # (planner 0 of b went on)
    b.sim_snapshot_drop(0)
    assert b.sim_snapshot_info(0) is None and a.sim_snapshot_info(0)["planners"].tolist() == [2, 0]
    a.close()
    assert b.sim_snapshot_info(0) is None
    b.close()


# ---- 10. every part in one call -------------------------------------------------------------------------------------------------------------
def parts_of(fleet, off, p):
    """What the models hold of planner ``p`` and a branch carries: telemetry, vehicle, safety and react records, the incident ring, the
    effective scales and the tracker's rows -- and the selector's ordered list, which the next tick computes from the carried list."""
    tele = fleet.sim_telemetry_read()
    _, tabs, cnt = fleet.sim_tracker_read(planners=[p], raw=True)
    (saf, ring), (rct, eff) = fleet.sim_safety_read(raw=True), fleet.sim_react_read(raw=True)
    return dict(tele={k: np.array(v[p]) for k, v in tele.items() if k != "track_length"}, veh=fleet.sim_vehicle_read(raw=True)[p].copy(),
                n_tracks=int(cnt[0]), tracks=tabs[0, :cnt[0]].copy(), order=fleet.sim_selector_read()[1][p].copy(), safety=saf[p].copy(),
                ring=ring[p].copy(), react=rct[p].copy(), eff=eff[off[p]:off[p + 1]].copy())


def test_every_part_in_one_call(hip, table, classes):
    """Telemetry, vehicle model, tracker, selector, safety monitor and reactive opponents set together: one ``sim_branch`` moves all of it.
    Planners (0, 1) and (2, 3) are twins by configuration -- one and three opponents, so offsets and bases of source and destination differ
    -- and not by state: the second of a pair starts elsewhere, its opponents further ahead. Leg 1: behind the branch a twin IS its source,
    in the trace, in ``sim_state`` and in every model's records, tick by tick. Leg 2: a snapshot taken with selector, monitor and reactive
    model off leaves their start states behind a restore, whatever the three had written since."""
    from graphbasedlocaltrajectoryplanner_amd import sim
    poses, further = [300.0, 700.0, 1100.0, 1500.0], [0.0, 9.0, 0.0, 7.0]
    # (opponents that have someone to react to, so that scales and reactive records are state: the lone one comes up behind the ego, within
    #  the model's sight; of the three the faster one closes in on the slower)
    ahead = [[(-120.0, 0.35, 5.0)]] * 2 + [[(45.0, 0.40, 5.0), (60.0, 0.30, 5.0), (110.0, 0.35, 5.0)]] * 2
    starts = [elsewhere(table, s) for s in poses]
    entries = [dict(classes["one"]["entry"], pos_est=starts[p][0], opponents=[(poses[p] + d + further[p], scale, length) for d, scale, length in ahead[p]])
               for p in range(4)]
    scales = np.array([q[1] for e in entries for q in e["opponents"]])
    off = opp_offsets(entries)
    fleet = build(hip, table, entries, starts, [sl.C2_VEL] * 4)

    def set_three():
        fleet.sim_selector()
        fleet.sim_safety()
        fleet.sim_react()
    fleet.sim_telemetry()
    fleet.sim_vehicle()
    fleet.sim_tracker()
    set_three()
    gd.run_one(fleet, 20)
    assert healthy(fleet)
    pairs = [(0, 1), (2, 3)]
    for s, d in pairs:
        a, b = parts_of(fleet, off, s), parts_of(fleet, off, d)
        assert a["n_tracks"] > 0 and not same(state_of(fleet, off, s), state_of(fleet, off, d))
        for key in ("tele", "veh", "tracks", "safety", "react"):
            assert not same(a[key], b[key]), (s, d, key)
    assert np.any(fleet.sim_react_read()[1][off[2]:off[3]] != scales[off[2]:off[3]])              # (effective scales that are state)
    assert fleet.sim_branch([0, 2], [1, 3]) >= 0.0
    for k in range(11):                                                                           # behind the branch, then behind each of 10 ticks
        for s, d in pairs:
            a, b = parts_of(fleet, off, s), parts_of(fleet, off, d)
            for key in a:
                assert key == "order" and k == 0 or same(a[key], b[key]), "%d ticks behind the branch: %s of planner %d is not planner %d's" % (k, key, d, s)
            assert same(state_of(fleet, off, d), state_of(fleet, off, s)), (k, s, d)
        if k < 10:
            tr = gd.run_one(fleet, 1)
            for s, d in pairs:
                same_rows(tr, d, tr, s, "tick %d behind the branch" % k)
    assert healthy(fleet)

    # leg 2: a source without state
    fleet.sim_selector(None)
    fleet.sim_safety(None)
    fleet.sim_react(None)
    fleet.sim_snapshot(0)
    set_three()
    gd.run_one(fleet, 2)
    fleet.sim_selector()                                                                          # (fresh statistics: the list stays)
    gd.run_one(fleet, 1)
    assert np.all(fleet.sim_selector_read()[0]["clear_min"] < np.inf)                             # objects were scored behind a fresh selector
    assert not same(fleet.sim_safety_read(raw=True)[0], sim.safety_start(4)[0]) and not same(fleet.sim_react_read(raw=True)[0], sim.react_start(4))
    fleet.sim_restore(0)
    (saf, ring), (rct, eff) = fleet.sim_safety_read(raw=True), fleet.sim_react_read(raw=True)
    assert same(saf, sim.safety_start(4)[0]) and same(ring, sim.safety_start(4)[1]) and same(rct, sim.react_start(4))
    assert same(eff, scales)
    fleet.sim_selector()
    gd.run_one(fleet, 1)
    d = fleet.sim_selector_read()[0]
    assert np.all(d["ticks"] == 1) and np.all(d["clear_min"] == np.inf)                           # the restored lists are empty
    assert healthy(fleet)
    fleet.close()
