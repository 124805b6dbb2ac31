"""
GPU: the race telemetry of the fleet's closed-loop simulation (ltpl_fleet_sim_telemetry / _read; csrc/fleet_sim.hpp k_fleet_sim_tele,
k_fleet_sim_rank) against its host mirror (sim.Telemetry over the oracle's get_s_coord) --

  1. the recorded races (race4, race3_mixed, set up as tests/test_gpu_fleet_race.py does) against the mirror ON THE RECORDINGS: counts,
     ranks and passes exactly, s / dist / clear_min / gap_ahead to 1e-5 m (the device follows the recorded poses to 1e-6 m);
  2. a race of 70 (the second block of both kernels' mate and object loops) next to a planner with 70 opponents and 26 statics, the
     mirror fed from the device's trace and objects rebuilt on the host: integers exactly, floats to 1e-9;
  3. laps: four free planners started before the line with four vel_max, until every one has crossed the line twice;
  4. telemetry only reads: trace, state, heading and digest of a fleet with telemetry equal the same fleet's without, bit for bit;
  5. one call against runs of 25 ticks with a read after each; a reset mid-way; a read while off;
  6. a car that fails stays ranked by its mate; a single planner next to a race.
"""
import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import telemetry_util as tu
import test_gpu_fleet_race as gr
import test_gpu_fleet_sim as gs
import test_gpu_sim_differential as gd
from test_gpu_fleet_race import cars, hip, race        # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu


def run_cuts(fleet, recs, n_ticks, every, after=None):
    """``test_gpu_fleet_race.run`` without its heading checks: runs split where the recordings' velocity arguments change and every
    ``every`` ticks, ``after(ticks done)`` behind each run. Returns the trace."""
    uniq, idx = [], []
    for p, r in enumerate(recs):
        for u, q in zip(uniq, idx):
            if u is r:
                q.append(p)
                break
        else:
            uniq.append(r)
            idx.append([p])
    cuts = sorted(set([a for a, _ in gs.segments(uniq, n_ticks)] + list(range(0, n_ticks, every)) + [n_ticks]))
    traces = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        gs.set_vel(fleet, uniq, idx, a)
        traces.append(fleet.sim_run(b - a)[0])
        if after:
            after(b)
    return np.concatenate(traces)


def recorded(hip, monteblanco, race, cars, name, telemetry, every=25, after=None):
    """The recorded race ``name`` on a fresh fleet: dict(trace, state, heading, digest, tele (None without telemetry), fleet)."""
    fleet, recs, sizes, entries, plan = gr.race_fleet(hip, race, cars, [(name, 1)])
    gr.setup(fleet, race, monteblanco, recs, sizes, entries)
    if telemetry:
        fleet.sim_telemetry(radius=tu.RADIUS)
    T = gr.SCEN[name]["n_ticks"]
    trace = run_cuts(fleet, recs, T, every, (lambda b: after(fleet, b)) if after else None)
    return dict(trace=trace, state=fleet.sim_state(), heading=fleet.sim_heading(), digest=fleet.digest(),
                tele=fleet.sim_telemetry_read() if telemetry else None, fleet=fleet, recs=recs)


@pytest.fixture(scope="module")
def race4_on(hip, monteblanco, race, cars):
    """race4 with telemetry, in runs of 25 ticks with a read after each (shared by tests 1, 4 and 5)."""
    reads = []
    out = recorded(hip, monteblanco, race, cars, "race4", True, after=lambda fleet, b: reads.append((b, fleet.sim_telemetry_read())))
    out["fleet"].close()
    out["reads"] = reads
    return out


# ---- 1. the recorded races -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["race4", "race3_mixed"])
def test_recorded_races_against_the_mirror_on_the_recordings(hip, monteblanco, oracle_backend, race, cars, race4_on, name):
    if name == "race4":
        dev = race4_on["tele"]
    else:
        out = recorded(hip, monteblanco, race, cars, name, True)
        out["fleet"].close()
        dev = out["tele"]
    mirrors = {nm: tu.recording_mirror(nm, monteblanco, oracle_backend) for nm in tu.RECORDINGS}
    m = mirrors[name]
    for f in ("ticks", "rank", "passes", "passed", "contact_ticks", "clear_min", "dist", "s", "gap_ahead", "act"):
        print(name, f, dev[f].tolist(), "mirror", m["fields"][f].tolist())
    # clear_tick / clear_slot: only where the recorded runner-up tick lies more than 1e-4 m above the minimum (the device follows the
    # recorded poses to 1e-6 m); that leaves out at most one of the seven cars
    close = {nm: [c for c in range(n) if tu.runner_up_margin(mirrors[nm]["clear"][c]) <= 1e-4] for nm, n in tu.RECORDINGS.items()}
    assert sum(len(v) for v in close.values()) <= 1, close
    tu.compare(dev, m["fields"], 1e-5, name, skip_clear_at=close[name],
               fields=("ticks", "s", "dist", "laps", "t_cross", "lap_last", "lap_best", "act", "clear_min", "clear_tick", "clear_slot",
                       "contact_ticks", "rank", "passes", "passed", "gap_ahead"))
    # vel_est follows the recording to 1e-5 relative per tick (tests/test_gpu_fleet_race.py): the bound of the sum is the sum of the bounds
    T = m["n_ticks"]
    v = np.array([[t['vel_args']['vel_est'] for t in c] for c in cars[name]])
    assert np.all(np.abs(dev["vel_sum"] - m["fields"]["vel_sum"]) <= 1e-5 * np.sum(np.maximum(np.abs(v), 1.0), axis=1))
    assert np.all(np.abs(dev["vel_max"] - m["fields"]["vel_max"]) <= 1e-5 * np.maximum(np.max(np.abs(v), axis=1), 1.0))
    assert dev["track_length"] == tu.track_length(monteblanco) and np.all(dev["ticks"] == T)


# ---- 2. a race larger than a wave -------------------------------------------------------------------------------------------------------
def test_race_of_70_and_a_crowded_planner_against_the_mirror_fed_from_the_trace(hip, monteblanco, oracle_backend, race):
    track = np.load(gr.os.path.join(gr.ROOT, "tests", "golden", "monteblanco_track.npz"))
    start = pr.load_ticks("c2")[0]['start']
    classes = sl.monteblanco_classes(race, track, tuple(start['pos']))
    units = [gd.single("crowded70", classes["crowded70"], start), gd.race_unit("race70", *sl.big_race(race, 70))]
    sc = gd.Scenario(monteblanco, race, units)
    fleet = sc.fleet(hip)
    fleet.sim_telemetry()                                       # radius 2.5
    feed = tu.TraceFeed(oracle_backend, race, sc.entries, sc.sizes)
    mir = sim_mirror(sc.n, sc.sizes, 2.5, monteblanco, oracle_backend)
    k, per_tick_cnt = 0, []
    for _ in range(4):
        trace = fleet.sim_run(sl.BIG_RACE_TICKS // 4)[0]
        assert np.all(trace[:, :, 8] == 0)
        for tr in trace:
            recs = feed.recs(tr)
            mir.update(k, recs)
            per_tick_cnt.append([len(r["objects"]) for r in recs])
            k += 1
        dev = fleet.sim_telemetry_read()
        assert sorted(dev["rank"][1:]) == list(range(1, 71)) and dev["rank"][0] == 1, dev["rank"]
        tu.compare(dev, mir.as_dict(), 1e-9, "70 + crowded70 after %d ticks" % k)
    cnt = np.array(per_tick_cnt)
    # the crowded planner's and the cars' object lists go past lane 64 (the second block of the clearance loop), and a closest object lies there
    assert cnt[:, 0].max() > 64 and cnt[:, 1:].max() > 64 and np.all(dev["ticks"] == sl.BIG_RACE_TICKS)
    assert np.isfinite(dev["clear_min"][0]) and dev["clear_slot"].max() >= 64
    print("objects per tick: crowded %d .. %d, race %d .. %d; clear_slot %s" % (cnt[:, 0].min(), cnt[:, 0].max(), cnt[:, 1:].min(),
                                                                              cnt[:, 1:].max(), dev["clear_slot"].tolist()))
    fleet.close()


def sim_mirror(n, sizes, radius, lat, oracle, dt=0.05):
    from graphbasedlocaltrajectoryplanner_amd import sim
    return sim.Telemetry(n, sizes, radius, tu.track_length(lat), oracle.raceline_s, dt)


# ---- 3. laps --------------------------------------------------------------------------------------------------------------------------
def test_lap_times_of_four_free_planners(hip, monteblanco, oracle_backend, race):
    vel_max = (100.0, 50.0, 40.0, 30.0)
    pos, heading = sl.race_line_pose(race, float(race.s_rl[-1]) - 30.0)
    entry = dict(opponents=[], static=[], pref=sl.DEFAULT_PREF, pos_est=pos, vel_est=0.0, zone_gids=[])
    units = [dict(cls="free%d" % i, entries=[entry], vels=[dict(sl.C2_VEL, vel_max=v)], starts=[(pos, heading, 0.0, np.pi / 4)])
             for i, v in enumerate(vel_max)]
    sc = gd.Scenario(monteblanco, race, units)
    fleet = sc.fleet(hip)
    fleet.sim_telemetry()
    feed = tu.TraceFeed(oracle_backend, race, sc.entries, sc.sizes)
    mir = sim_mirror(4, sc.sizes, 2.5, monteblanco, oracle_backend)
    k = 0
    while k < 3000 and not np.all(mir.as_dict()["laps"] >= 2):
        trace = fleet.sim_run(200)[0]
        assert np.all(trace[:, :, 8] == 0)
        for tr in trace:
            mir.update(k, feed.recs(tr))
            k += 1
    dev, m = fleet.sim_telemetry_read(), mir.as_dict()
    print("ticks %d laps %s lap_last %s t_cross %s" % (k, dev["laps"].tolist(), dev["lap_last"].tolist(), dev["t_cross"].tolist()))
    assert np.all(m["laps"] >= 2), "no two crossings within %d ticks: laps %s" % (k, m["laps"])
    tu.compare(dev, m, 1e-9, "laps")
    assert np.all(np.isfinite(dev["lap_last"])) and np.all(dev["lap_best"] <= dev["lap_last"])
    assert np.all(np.diff(dev["lap_last"]) > 0.0), dev["lap_last"]          # a smaller vel_max, a longer lap
    assert np.all(dev["rank"] == 1) and np.all(np.isnan(dev["gap_ahead"]))
    fleet.close()


# ---- 4. telemetry only reads ----------------------------------------------------------------------------------------------------------
def test_telemetry_changes_nothing_else(hip, monteblanco, race, cars, race4_on):
    off = recorded(hip, monteblanco, race, cars, "race4", False)
    off["fleet"].close()
    assert np.array_equal(off["trace"], race4_on["trace"], equal_nan=True)
    for key, v in off["state"].items():
        assert np.array_equal(v, race4_on["state"][key]), key
    assert np.array_equal(off["heading"], race4_on["heading"]) and np.array_equal(off["digest"], race4_on["digest"])


# ---- 5. chunks and reads ----------------------------------------------------------------------------------------------------------------
def test_one_call_equals_runs_with_reads_and_a_reset_restarts(hip, monteblanco, race, cars, race4_on):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.sim import TELEMETRY_FIELDS
    assert len(race4_on["reads"]) >= 24 and [b for b, _ in race4_on["reads"]][-1] == 600
    ticks = np.array([d["ticks"] for _, d in race4_on["reads"]])
    assert np.all(ticks == np.array([b for b, _ in race4_on["reads"]])[:, None])          # every read sees the ticks run so far
    one = recorded(hip, monteblanco, race, cars, "race4", True, every=10 ** 9)              # (split only where the velocity arguments change)
    for name, _, _, _ in TELEMETRY_FIELDS:
        assert np.array_equal(one["tele"][name], race4_on["tele"][name], equal_nan=True), name
    fleet = one["fleet"]
    fleet.sim_telemetry(radius=tu.RADIUS)                      # set again: the records and the tick index start over
    d = fleet.sim_telemetry_read()
    assert np.all(d["ticks"] == 0) and np.all(np.isnan(d["s"])) and np.all(d["rank"] == 0) and np.all(d["clear_tick"] == -1)
    assert np.all(np.isinf(d["clear_min"])) and np.all(d["dist"] == 0.0) and np.all(d["vel_max"] == -np.inf)
    fleet.sim_run(10)
    d = fleet.sim_telemetry_read()
    assert np.all(d["ticks"] == 10) and sorted(d["rank"]) == [1, 2, 3, 4]
    assert np.all(d["clear_tick"] >= 0) and np.all(d["clear_tick"] <= 9)
    fleet.sim_telemetry(radius=None)
    with pytest.raises(BackendError, match="telemetry is off"):
        fleet.sim_telemetry_read()
    fleet.sim_run(5)                                           # and the simulation runs on without it
    fleet.close()


# ---- 6. a failed car; a single planner next to a race ---------------------------------------------------------------------------------------
def test_a_failed_car_keeps_its_record_and_its_place(hip, monteblanco, oracle_backend, race, cars):
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    r4 = cars["race4"]
    # the scenario of test_a_failed_car_stays_in_its_mates_list (car 0 finds no action in the first tick: it never lives) ...
    fleet = Fleet(hip, 2)
    gs.start(fleet, [(r4[0], [0]), (r4[1], [1])])
    fleet.sim_setup(race, [gr.car_entry("race4", 0, pref=("right", "left", "follow")), gr.car_entry("race4", 1)])
    fleet.sim_race([2])
    fleet.sim_telemetry(radius=tu.RADIUS)
    gs.set_vel(fleet, [r4[0], r4[1]], [[0], [1]], 0)
    with pytest.raises(BackendError, match="planner 0: closed-loop simulation"):
        fleet.sim_run(80)
    d = fleet.sim_telemetry_read()
    assert list(d["ticks"]) == [0, 80] and list(d["rank"]) == [0, 1] and np.isnan(d["gap_ahead"][1]) and np.isnan(d["s"][0])
    assert d["passes"][1] == 0 and d["passed"][1] == 0 and np.isfinite(d["clear_min"][1]) and np.isinf(d["clear_min"][0])
    fleet.close()
    # ... and a car that only drives straight: it lives until the key is gone, then its record stops and its mate still ranks it
    fleet = Fleet(hip, 2)
    gs.start(fleet, [(r4[0], [0]), (r4[1], [1])])
    entries = [gr.car_entry("race4", 0, pref=("straight",)), gr.car_entry("race4", 1)]
    fleet.sim_setup(race, entries)
    fleet.sim_race([2])
    fleet.sim_telemetry(radius=tu.RADIUS)
    gs.set_vel(fleet, [r4[0], r4[1]], [[0], [1]], 0)
    T = 400
    with pytest.raises(BackendError, match="planner 0: closed-loop simulation"):
        fleet.sim_run(T)
    trace, d = fleet.last_trace, fleet.sim_telemetry_read()
    n_live = int(np.sum(trace[:, 0, 8] == 0))
    print("car 0 lives %d ticks; ranks %s gap %s" % (n_live, d["rank"].tolist(), d["gap_ahead"].tolist()))
    assert 0 < n_live < T and np.all(trace[:n_live, 0, 8] == 0) and np.all(trace[:, 1, 8] == 0)
    # the stopped car keeps the rank of its last live tick; its mate goes on being ranked against where it stopped
    assert list(d["ticks"]) == [n_live, T] and d["rank"][0] in (1, 2) and d["rank"][1] in (1, 2)
    assert np.isnan(d["gap_ahead"][1]) == (d["rank"][1] == 1)
    feed = tu.TraceFeed(oracle_backend, race, entries, [2])
    mir = sim_mirror(2, [2], tu.RADIUS, monteblanco, oracle_backend)
    for k, tr in enumerate(trace):
        mir.update(k, feed.recs(tr))
    tu.compare(d, mir.as_dict(), 1e-9, "failed car")
    fleet.close()


def test_a_single_planner_next_to_a_race(hip, monteblanco, race, cars):
    cars = dict(cars, c2=pr.load_ticks("c2"))
    fleet, recs, sizes, entries, plan = gr.race_fleet(hip, race, cars, [("race3_mixed", 1), ("c2", 1)])
    gr.setup(fleet, race, monteblanco, recs, sizes, entries)
    fleet.sim_telemetry(radius=tu.RADIUS)
    run_cuts(fleet, recs, 100, 50)
    d = fleet.sim_telemetry_read()
    assert np.all(d["ticks"] == 100) and sorted(d["rank"][:3]) == [1, 2, 3]
    assert d["rank"][3] == 1 and d["passes"][3] == 0 and d["passed"][3] == 0 and np.isnan(d["gap_ahead"][3])
    assert np.sum(np.isnan(d["gap_ahead"][:3])) == 1
    fleet.close()
