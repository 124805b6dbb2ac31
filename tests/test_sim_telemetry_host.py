"""
CPU: the race telemetry of the fleet simulation (ltpl_fleet_sim_telemetry, include/ltpl_hip.h) on the host --

  1. the mirror (sim.Telemetry) on the reference's own race recordings (race4, race3_mixed: pose, clock, action, speed and object list of
     every car and tick), projected by the oracle's get_s_coord: ranks, passes, contacts, distances, clearances and action counts against
     numbers taken from a numpy restatement of get_s_coord on the same recordings, and the margins that keep them stable under the
     device's 1e-6 m pose agreement;
  2. the lap logic on made-up inputs: forward and backward crossings, the interpolated crossing time, lap times, a first tick on a
     polyline point, a planner that is not live for some ticks, and a race larger than a wave with two equal progress values;
  3. the argument checks of the two entry points on the stand-in runtime (tools/fakehip/sim_telemetry_args.py, plain build).
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import telemetry_util as tu
from graphbasedlocaltrajectoryplanner_amd import fleet, sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = {
    "race4": dict(n_ticks=600, first=[1, 2, 3, 4], last=[3, 1, 2, 4], passes=[0, 1, 1, 0], passed=[2, 0, 0, 0], contact=[18, 18, 0, 0],
                  dist=[249.8747, 490.4214, 461.5155, 371.9936], clear={0: (1.535628, 294, 0), 1: (1.535628, 294, 0), 2: (3.660794, None, None)}),
    "race3_mixed": dict(n_ticks=400, first=[1, 2, 3], last=[2, 1, 3], passes=[0, 1, 0], passed=[1, 0, 0], contact=[14, 14, 0],
                        dist=[269.4954, 367.8840, 333.4396], clear={0: (1.378777, 344, 4), 1: (1.378777, 344, 4)}),
}


def test_track_length_of_monteblanco(monteblanco):
    L = tu.track_length(monteblanco)
    assert abs(monteblanco.s_raceline[-1] - 2367.3048672) < 1e-6 and abs(L - 2382.2979975) < 1e-6
    assert fleet.TELEMETRY_FIELDS is sim.TELEMETRY_FIELDS and sum(c for _, _, c, _ in sim.TELEMETRY_FIELDS) == sim.TELEMETRY_DOUBLES == 22
    assert [i for _, i, _, _ in sim.TELEMETRY_FIELDS] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 14, 15, 16, 17, 18, 19, 20, 21]


@pytest.mark.parametrize("name", ["race4", "race3_mixed"])
def test_mirror_on_the_recordings(monteblanco, oracle_backend, name):
    m, e = tu.recording_mirror(name, monteblanco, oracle_backend), EXPECTED[name]
    f = m["fields"]
    assert m["n_ticks"] == e["n_ticks"] and np.all(f["ticks"] == e["n_ticks"])
    assert list(m["first_rank"]) == e["first"] and list(f["rank"]) == e["last"]
    assert list(f["passes"]) == e["passes"] and list(f["passed"]) == e["passed"]
    assert list(f["contact_ticks"]) == e["contact"]
    assert np.all(np.abs(f["dist"] - e["dist"]) <= 1e-3), f["dist"]
    for car, (c, tick, slot) in e["clear"].items():
        assert abs(f["clear_min"][car] - c) <= 1e-5, (car, f["clear_min"][car])
        if tick is not None:
            assert (f["clear_tick"][car], f["clear_slot"][car]) == (tick, slot), (car, f["clear_tick"][car], f["clear_slot"][car])
    if name == "race4":
        assert list(f["act"][1]) == [291, 147, 13, 149, 0]
    assert np.all(f["laps"] == 0) and np.all(np.isnan(f["t_cross"])) and np.all(np.isnan(f["lap_best"]))
    assert np.all(f["act"].sum(axis=1) == e["n_ticks"])
    # the leader has no gap; every other gap is the progress difference to the car one rank ahead
    lead = int(np.argmin(f["rank"]))
    assert np.isnan(f["gap_ahead"][lead]) and np.all(f["gap_ahead"][np.arange(len(e["last"])) != lead] > 0.0)
    assert f["track_length"] == tu.track_length(monteblanco)
    # what keeps ranks and contacts stable under a pose agreement of 1e-6 m (a changed fixture says so here)
    assert m["prog_margin"] > 1e-3 and m["clear_margin"] > 1e-3, (m["prog_margin"], m["clear_margin"])
    assert abs(m["prog_margin"] - (0.100 if name == "race4" else 0.204)) < 1e-3
    assert abs(m["clear_margin"] - (0.127 if name == "race4" else 0.0186)) < 1e-3


def on_line(lat, i, frac=0.25):
    """A point on segment (i, i + 1) of the closed race-line polyline."""
    a, b = lat.raceline[i % lat.raceline.shape[0]], lat.raceline[(i + 1) % lat.raceline.shape[0]]
    return (float(a[0] + frac * (b[0] - a[0])), float(a[1] + frac * (b[1] - a[1])))


def rec(pos, now, live=True, sel="straight", vel=10.0, objects=()):
    return dict(live=live, sel=sel, now=now, pos=pos, vel=vel, objects=list(objects))


def test_laps_and_crossing_times(monteblanco, oracle_backend):
    lat, n, L, dt = monteblanco, monteblanco.raceline.shape[0], tu.track_length(monteblanco), 0.7
    tm = sim.Telemetry(1, [1], 2.5, L, oracle_backend.raceline_s, dt)
    idx = list(range(n - 3, 3 * n + 2))                   # three times over the line
    s_prev, crossings, now = None, [], 100.0
    for k, i in enumerate(idx):
        now += dt if i < 2 * n else 2 * dt                # a slower third lap on the made-up clock
        pos = on_line(lat, i)
        tm.update(k, [rec(pos, now)])
        s = oracle_backend.raceline_s(pos)
        if s_prev is not None and s - s_prev < -L / 2:
            d = (s - s_prev) + L
            assert d > 0.0
            crossings.append(now - dt * (s / d))
        s_prev = s
    f = tm.as_dict()
    assert len(crossings) == 3 and f["laps"][0] == 3 and f["ticks"][0] == len(idx)
    assert f["t_cross"][0] == crossings[2] and f["lap_last"][0] == crossings[2] - crossings[1]
    assert f["lap_best"][0] == crossings[1] - crossings[0] < f["lap_last"][0]
    # every step runs forward: the distance is the arc length covered, three times the closed length less the start's lead
    assert abs(f["dist"][0] - (2 * L + (oracle_backend.raceline_s(on_line(lat, 1)) + L - oracle_backend.raceline_s(on_line(lat, n - 3))))) < 1e-6
    assert list(f["act"][0]) == [len(idx), 0, 0, 0, 0] and f["vel_sum"][0] == 10.0 * len(idx) and f["vel_max"][0] == 10.0
    assert f["rank"][0] == 1 and f["passes"][0] == f["passed"][0] == 0 and np.isnan(f["gap_ahead"][0])
    assert np.isinf(f["clear_min"][0]) and f["clear_tick"][0] == f["clear_slot"][0] == -1 and f["contact_ticks"][0] == 0


def test_a_backward_crossing_takes_a_lap_back_and_no_time(monteblanco, oracle_backend):
    lat, n, L = monteblanco, monteblanco.raceline.shape[0], tu.track_length(monteblanco)
    tm = sim.Telemetry(1, [1], 2.5, L, oracle_backend.raceline_s, 0.05)
    tm.update(0, [rec(on_line(lat, 1), 1.0)])
    tm.update(1, [rec(on_line(lat, n - 2), 1.05)])
    f = tm.as_dict()
    assert f["laps"][0] == -1 and np.isnan(f["t_cross"][0]) and np.isnan(f["lap_last"][0]) and f["dist"][0] < 0.0
    tm.update(2, [rec(on_line(lat, 1), 1.1)])
    f = tm.as_dict()
    assert f["laps"][0] == 0 and abs(f["dist"][0]) < 1e-9 and 1.05 < f["t_cross"][0] <= 1.1
    assert np.isnan(f["lap_last"][0]) and np.isnan(f["lap_best"][0])         # one forward crossing: no lap time yet


def test_first_tick_on_a_polyline_point(monteblanco, oracle_backend):
    lat = monteblanco
    pos = (float(lat.raceline[17, 0]), float(lat.raceline[17, 1]))
    tm = sim.Telemetry(1, [1], 2.0, tu.track_length(lat), oracle_backend.raceline_s, 0.05)
    tm.update(0, [rec(pos, 1.0, sel="follow", vel=3.0, objects=[(pos[0] + 3.0, pos[1] + 4.0, 2.5), (pos[0] + 3.0, pos[1] + 4.0, 2.5)])])
    f = tm.as_dict()
    assert f["ticks"][0] == 1 and f["dist"][0] == 0.0 and f["s"][0] == oracle_backend.raceline_s(pos) and math.isfinite(f["s"][0])
    assert abs(f["s"][0] - lat.s_raceline[17]) < 0.5 and tm.grid[0] == f["s"][0]
    assert abs(f["clear_min"][0] - 2.5) < 1e-9 and (f["clear_tick"][0], f["clear_slot"][0]) == (0, 0)     # two equal clearances: the first counts
    assert f["contact_ticks"][0] == 0 and list(f["act"][0]) == [0, 1, 0, 0, 0]              # (2.5 is not below the radius 2.0)
    tm.update(7, [rec(pos, 1.05, objects=[(pos[0] + 3.0, pos[1] + 4.0, 2.5)])])
    f = tm.as_dict()
    assert (f["clear_tick"][0], f["clear_slot"][0]) == (0, 0) and f["dist"][0] == 0.0         # replaced only on strictly smaller
    tm.update(8, [rec(pos, 1.1, objects=[(pos[0] + 50.0, pos[1], 2.5), (pos[0], pos[1] + 4.0, 2.5)])])
    f = tm.as_dict()
    assert abs(f["clear_min"][0] - 1.5) < 1e-9 and (f["clear_tick"][0], f["clear_slot"][0]) == (8, 1) and f["contact_ticks"][0] == 1


def line_telemetry(n, races, grid_s=None, L=1000.0):
    """A made-up straight 'track': s = x."""
    return sim.Telemetry(n, races, 2.5, L, lambda pos: float(pos[0]), 0.05, grid_s=grid_s)


def test_a_planner_that_is_not_live_keeps_its_record_and_its_place():
    tm = line_telemetry(3, [3])
    x = [[30.0, 20.0, 10.0], [31.0, 21.0, 11.0]]
    for k in range(2):
        tm.update(k, [rec((x[k][p], 0.0), 1.0 + k) for p in range(3)])
    assert list(tm.as_dict()["rank"]) == [1, 2, 3]
    frozen = tm.rows()[1].copy()
    # planner 1 is not live for four ticks; planner 2 drives past where it stopped
    for k, x2 in enumerate((15.0, 20.5, 21.0, 25.0), start=2):
        tm.update(k, [rec((32.0 + k, 0.0), 1.0 + k), dict(live=False), rec((x2, 0.0), 1.0 + k)])
        assert np.array_equal(tm.rows()[1], frozen, equal_nan=True)
    f = tm.as_dict()
    # 21.0 == 21.0: the lower index (the stopped planner) is still ahead at equal progress; 25.0 is past it
    assert list(f["rank"]) == [1, 2, 2] and f["passes"][2] == 1 and f["ticks"][1] == 2 and f["gap_ahead"][2] == 37.0 - 25.0
    tm.update(6, [rec((40.0, 0.0), 7.0), rec((22.0, 0.0), 7.0), rec((26.0, 0.0), 7.0)])
    f = tm.as_dict()
    assert list(f["rank"]) == [1, 3, 2] and f["passed"][1] == 1 and f["ticks"][1] == 3 and f["dist"][1] == 2.0
    # a mate that has not lived a tick is behind everybody
    tm = line_telemetry(3, [3])
    tm.update(0, [dict(live=False), rec((5.0, 0.0), 1.0), rec((-400.0, 0.0), 1.0)])
    f = tm.as_dict()
    assert list(f["rank"]) == [0, 1, 2] and f["ticks"][0] == 0 and np.isnan(f["s"][0])


def test_a_race_of_70_with_two_equal_progress_values():
    n = 72                                                   # a single planner, a race of 70, a single planner
    grid = [5.0] + [700.0 - 10.0 * k for k in range(70)] + [900.0]
    grid[1 + 40] = grid[1 + 12]
    tm = line_telemetry(n, [1, 70, 1], grid_s=grid)
    tm.update(0, [rec((100.0, 0.0), 1.0) for _ in range(n)])
    f = tm.as_dict()
    rk = f["rank"][1:71]
    assert sorted(rk) == list(range(1, 71)) and rk[12] == 13 and rk[40] == 14 and f["gap_ahead"][1 + 40] == 0.0
    assert f["gap_ahead"][1 + 12] == 10.0 and np.isnan(f["gap_ahead"][1]) and f["gap_ahead"][1 + 69] == 10.0
    assert f["rank"][0] == f["rank"][71] == 1 and np.isnan(f["gap_ahead"][0]) and np.all(f["passes"] == 0) and np.all(f["passed"] == 0)


def test_telemetry_entry_points_check_their_arguments_without_a_device():
    env = dict(os.environ, FAKEHIP_SAN="none", LTPL_NO_SELFTEST="1")
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "sim_telemetry_args.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and "sim telemetry args OK" in p.stdout, p.stdout[-3000:]
    assert "launches per tick" in p.stdout and "previous telemetry kept" in p.stdout, p.stdout[-3000:]
