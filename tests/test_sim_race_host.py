"""
CPU: races of the fleet simulation (ltpl_fleet_sim_race: planners of one fleet that see one another) -- the host mirrors of
graphbasedlocaltrajectoryplanner_amd/sim.py against the race recordings of the unmodified reference (tools/gen_golden_race.py: several
Graph_LTPL instances in lockstep, every car's object list holding the other cars at their tracked pose):
  - the heading of the tracked pose (sim.vdc_track + sim.peer_heading) bit for bit from every tick whose recording holds the full trajectory
    the next tick tracks (the recording's headings come from the generator's own statement of the rule), and against np.interp on the
    unwrapped psi column there; on EVERY tick the recorded heading against the direction in which the car moved;
  - the mates' objects (sim.race_objects) bit for bit against the object lists handed to the reference, and the reference's on-track
    survivors as the list-order subset of them;
and the argument checks of ltpl_fleet_sim_race / ltpl_fleet_sim_heading on the stand-in runtime (tools/fakehip/sim_race_args.py).
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import planner_replay as pr
from graphbasedlocaltrajectoryplanner_amd import sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRED_DT = 0.2
N_EXPORT = 115
with open(os.path.join(ROOT, "tests", "golden", "race_scenarios.json")) as fh:
    SCEN = json.load(fh)


def cars_of(name):
    return [pr.load_ticks("%s_car%d" % (name, k)) for k in range(len(SCEN[name]["cars"]))]


@pytest.fixture(scope="module", params=sorted(SCEN))
def race(request):
    return request.param, cars_of(request.param)


def test_heading_of_the_tracked_pose_reproduces_the_recording_bit_for_bit(race):
    name, cars = race
    n = 0
    for k, ticks in enumerate(cars):
        spec = SCEN[name]["cars"][k]
        assert ticks[0]['start']['heading'] == spec["heading"] and list(ticks[0]['start']['pos']) == spec["pos"]
        for i in range(len(ticks) - 1):
            full, sel = ticks[i]['full'], ticks[i + 1]['action_id_sel']
            if full is None or sel not in full.get('traj', {}):
                continue
            traj = full['traj'][sel][:N_EXPORT]
            pos, vel, s, j = sim.vdc_track(ticks[i]['pos_est'], traj, 0.05)
            assert (pos, vel) == sim.vdc_step(ticks[i]['pos_est'], traj, 0.05)
            theta = ticks[i]['theta_est'] if s is None else sim.peer_heading(s, j, traj[:, 0], traj[:, 3])
            nxt = ticks[i + 1]
            w = "%s car %d tick %d -> %d" % (name, k, i, i + 1)
            assert pos == list(nxt['pos_est']) and vel == nxt['vel_args']['vel_est'], w
            assert theta == nxt['theta_est'], "%s: heading %r vs %r" % (w, theta, nxt['theta_est'])
            if s is not None:                                  # the same rule stated differently: interp on the unwrapped column
                alt = float(np.interp(s, traj[:, 0], np.unwrap(traj[:, 3])))
                assert wrapped(theta - alt) <= 1e-9, "%s: heading %r vs unwrapped interp %r" % (w, theta, alt)
            n += 1
    assert n >= 20, n


def wrapped(d):
    return abs((d + math.pi) % (2 * math.pi) - math.pi)


def test_heading_follows_the_direction_of_motion_on_every_tick(race):
    name, cars = race
    n = crossed = 0
    for k, ticks in enumerate(cars):
        for i in range(len(ticks) - 1):
            (x0, y0), (x1, y1) = ticks[i]['pos_est'], ticks[i + 1]['pos_est']
            a, b = ticks[i]['theta_est'], ticks[i + 1]['theta_est']
            assert -math.pi < b <= math.pi
            crossed += abs(b - a) > math.pi
            if math.hypot(x1 - x0, y1 - y0) < 0.2:
                continue
            motion = math.atan2(y1 - y0, x1 - x0) - math.pi / 2       # the reference's heading convention (psi = 0: north)
            assert wrapped(b - motion) <= 0.1, "%s car %d tick %d: heading %r, moved towards %r" % (name, k, i + 1, b, motion)
            n += 1
    assert n >= 0.9 * sum(len(t) - 1 for t in cars), n
    if name == "race4":
        assert crossed > 0                                    # race4 drives through the +-pi wrap of the race line's heading


def test_mates_reproduce_the_recorded_objects_and_their_on_track_subset(race):
    name, cars = race
    N, nd = len(cars), len(SCEN[name]["dummies"])
    length = [SCEN[name]["length"]] * N
    mates_kept = 0
    for i in range(len(cars[0])):
        pos = [cars[q][i]['pos_est'] for q in range(N)]
        vel = [cars[q][i]['vel_args']['vel_est'] for q in range(N)]
        theta = [cars[q][i]['theta_est'] for q in range(N)]
        if i == 0:
            assert theta == [c["heading"] for c in SCEN[name]["cars"]]                 # heading0 before the first trajectory
        for k in range(N):
            t = cars[k][i]
            w = "%s car %d tick %d" % (name, k, i)
            objs = sim.race_objects(k, range(N), pos, vel, theta, length)
            rows = np.array([[o['X'], o['Y'], o['theta'], o['v'], o['length']] for o in objs]).reshape(-1, 5)
            assert np.array_equal(rows, t['obj_in'][nd:]), w
            assert [o['id'] for o in objs] == [100 + q for q in range(N) if q != k]
            # the survivors are a list-order subset of the objects handed in; the mates' ones follow the dummies'
            src = []
            m = 0
            for x, y in np.asarray(t['obj_pos'], float).reshape(-1, 2):
                while m < len(t['obj_in']) and tuple(t['obj_in'][m, :2]) != (x, y):
                    m += 1
                assert m < len(t['obj_in']), "%s: survivor (%r, %r) is not in the object list" % (w, x, y)
                src.append(m)
                m += 1
            assert src == sorted(src)
            for v, m in enumerate(src):
                X, Y, th, vv, ln = t['obj_in'][m]
                assert t['obj_vel'][v] == vv and t['obj_radius'][v] == ln / 2.0, w
                pred = (X - np.sin(th) * vv * PRED_DT, Y + np.cos(th) * vv * PRED_DT)
                assert pred == tuple(np.asarray(t['obj_pred'][v]).reshape(-1)), "%s: prediction of object %d" % (w, m)
            mates_kept += sum(1 for m in src if m >= nd)
    assert mates_kept > 0


def test_peer_heading_across_the_wrap():
    ts, psi = [0.0, 1.0, 2.0, 3.0], [3.0, -3.1, -2.9, 0.5]
    assert sim.peer_heading(-1.0, -1, ts, psi) == 3.0 and sim.peer_heading(9.0, 4, ts, psi) == 0.5 and sim.peer_heading(3.0, 3, ts, psi) == 0.5
    d = -3.1 - 3.0 + 2 * math.pi                                         # the short way: through +-pi
    th = 3.0 + d * 0.9
    assert sim.peer_heading(0.9, 0, ts, psi) == th - 2 * math.pi and -math.pi < th - 2 * math.pi < -3.1   # past pi: wrapped
    assert sim.peer_heading(0.5, 0, ts, psi) == 3.0 + d * 0.5 < math.pi                                # still below pi
    assert sim.peer_heading(1.5, 1, ts, psi) == -3.1 + (-2.9 - -3.1) * 0.5
    assert sim.peer_heading(1.0, 1, [0.0, 1.0, 1.0, 3.0], psi) == -3.1                   # a repeated knot
    d = 3.0 - -3.0 - 2 * math.pi
    assert sim.peer_heading(0.25, 0, [0.0, 1.0], [-3.0, 3.0]) == -3.0 + d * 0.25
    assert -3.0 + d * 0.5 <= -math.pi and sim.peer_heading(0.5, 0, [0.0, 1.0], [-3.0, 3.0]) == -3.0 + d * 0.5 + 2 * math.pi   # (-pi, pi]
    assert sim.vdc_track([4.0, 5.0], np.array([[0.0, 1.0, 2.0, 0.0, 0.0, 7.5, 0.0]] * 2), 0.05) == ([4.0, 5.0], 7.5, None, None)


def test_race_objects_list_order():
    objs = sim.race_objects(2, [4, 1, 2, 3], {q: (q, -q) for q in range(5)}, [10.0 * q for q in range(5)], [0.1 * q for q in range(5)],
                            [4.0 + q for q in range(5)])
    assert [o['id'] for o in objs] == [101, 103, 104]
    assert objs[0] == {'X': 1.0, 'Y': -1.0, 'theta': 0.1, 'type': 'physical', 'id': 101, 'length': 5.0, 'v': 10.0}


def test_race_entry_points_check_their_arguments_without_a_device():
    env = dict(os.environ, FAKEHIP_SAN="none", LTPL_NO_SELFTEST="1")
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "sim_race_args.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and "sim race args OK" in p.stdout, p.stdout[-3000:]
    assert "above 96" in p.stdout and "launches per tick" in p.stdout, p.stdout[-3000:]
