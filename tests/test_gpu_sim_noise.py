"""
GPU: the seeded sensor noise of the fleet's closed-loop simulation (ltpl_fleet_sim_noise / _estimate / _noise_draws; csrc/fleet_noise.hpp,
k_fleet_sim_step_noise / k_fleet_sim_mates_noise in csrc/fleet_sim.hpp) against its host mirror (sim.noise_gauss, sim.NoiseModel) and the
noisy host loop of tests/sim_noise_util.py --

  1. draws: g and the generator's words bit-equal to the mirror on the tuples of sim_noise_util.draw_tuples;
  2. seated differential in the manner of tests/test_gpu_sim_differential.py: per tick the estimate bit-equal to the mirror applied to the
     device's own state, the recorder's objects (perceived x, y, v, prediction) within 1e-12 of the mirror, action / clock / counts / first
     vehicle / paths / trajectories by that file's rules, and one call of K ticks bitwise equal to the K single ticks (digest included);
  3. identity: all sigmas 0, and noise set then cleared, leave the trace bit-identical to a fleet that never called sim_noise;
  4. layout independence: a planner alone and the same planner at index 5 of 70 give identical trace rows; another seed another estimate;
  5. tick0: 20 ticks in one run = 10 + sim_noise(tick0=10) + 10; a restored snapshot with tick0 reproduces the second half bit for bit;
  6. telemetry measures clearance and contacts against the TRUE object positions;
  7. refused calls leave the previous noise in force.
"""
import os

import numpy as np
import pytest

import planner_replay as pr
import sim_loop as sl
import sim_noise_util as nu
import telemetry_util as tu
import test_gpu_sim_differential as gd
from fleet_differential import same_paths, same_trajectories

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12                     # tests/test_gpu_sim_differential.py: the bound of an opponent's position


@pytest.fixture(scope="module")
def hip(monteblanco):
    from graphbasedlocaltrajectoryplanner_amd import _capi
    return _capi.HipBackend(monteblanco)


@pytest.fixture(scope="module")
def table():
    from graphbasedlocaltrajectoryplanner_amd.sim import RaceLineTable
    return RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))


@pytest.fixture(scope="module")
def track():
    return np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz"))


@pytest.fixture(scope="module")
def c2_start():
    return pr.load_ticks("c2")[0]['start']


# ---- 1. draws ---------------------------------------------------------------------------------------------------------------------------
def test_draws_equal_the_mirror_bit_for_bit(hip):
    from graphbasedlocaltrajectoryplanner_amd import sim
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    fleet = Fleet(hip, 1)
    seed, tick, obj, comp = nu.draw_tuples()
    g, words = fleet.sim_noise_draws(seed, tick, obj, comp, words=True)
    assert g.shape == seed.shape and words.shape == (seed.size, 12)
    assert np.array_equal(words, sim.noise_words(seed, tick, obj, comp))
    assert np.array_equal(g.view(np.uint64), sim.noise_gauss(seed, tick, obj, comp).view(np.uint64))
    assert np.array_equal(fleet.sim_noise_draws(seed[:300], tick[:300], obj[:300], comp[:300]), g[:300])          # (without the words; two blocks)
    assert fleet.sim_noise_draws(np.zeros(0, np.uint64), 0, 0, 0).shape == (0,)
    fleet.close()


# ---- scenarios ----------------------------------------------------------------------------------------------------------------------------
def singles(table, track, start):
    """Three single planners, each with 2 opponents and 1 static of its own (classes of their own: each is compared in full)."""
    lap = float(table.s_rl[-1])
    opp = [[(250.0, 0.35, 5.0), (lap - 1.0, 0.5, 5.0)], [(140.0, 0.4, 5.0), (300.0, 0.2, 5.0)], [(200.0, 0.3, 5.0), (420.0, 0.1, 4.0)]]
    out = []
    for k in range(3):
        e = dict(opponents=opp[k], static=sl.crowded_statics(track, 1, 21 + k, first_row=260 + 30 * k, off_every=5, off_phase=4),
                 pref=sl.DEFAULT_PREF, pos_est=tuple(start['pos']), vel_est=0.0, zone_gids=[])
        out.append(gd.single("n%d" % k, dict(entry=e, vel=sl.C2_VEL), start))
    return out


def race3(table):
    return gd.race_unit("race3", *sl.big_race(table, 3, gap=25.0))


def seventy(table, track, start):
    """One planner with 70 objects: 40 opponents, then 30 statics of which every third lies 40 m off the track -- list indices 40, 43, ..
    69: dropped objects on both sides of lane 64."""
    lap = float(table.s_rl[-1])
    opp = [(250.0, 0.35, 5.0), (lap - 1.0, 0.5, 5.0)] + [(600.0 + 40.0 * k, (0.0, 0.02, 0.05)[k % 3], 5.0) for k in range(38)]
    e = dict(opponents=opp, static=sl.crowded_statics(track, 30, 11), pref=sl.DEFAULT_PREF, pos_est=tuple(start['pos']), vel_est=0.0, zone_gids=[])
    return gd.single("seventy", dict(entry=e, vel=sl.C2_VEL), start)


def noise_args(n, seed0=1000):
    """Seeds and sigmas of ``n`` planners: the sigmas of sim_noise_util.SIGMAS, scaled per planner; every fourth planner with obj_theta and
    vel switched off (a component that draws nothing next to ones that do)."""
    p = np.arange(n)
    kw = {k: v * (1.0 + 0.25 * (p % 3)) for k, v in nu.SIGMAS.items()}
    kw["obj_theta"] = np.where(p % 4 == 3, 0.0, kw["obj_theta"])
    kw["vel"] = np.where(p % 4 == 3, 0.0, kw["vel"])
    kw["seed"] = (np.uint64(seed0) + p.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
    return kw


def noisy_host(sc, oracle, kw, tick0=0):
    """``Scenario.host`` with the noisy loop over the scenario's host planners."""
    from graphbasedlocaltrajectoryplanner_amd import sim
    from oracle.planner_host import HostPlannerBackend
    backend = HostPlannerBackend(sc.lat)
    sub = {k: np.broadcast_to(np.asarray(v), (sc.n,))[sc.hmap] for k, v in kw.items()}
    model = sim.NoiseModel(len(sc.hmap), races=[sc.sizes[i] for i in sc.host_units], **sub)
    loop = nu.NoisySimLoop(sc.lat, sc.tab, [sc.entries[p] for p in sc.hmap], [backend.planner(1, **sc.config) for _ in sc.hmap],
                           oracle=oracle, dt=sc.dt, n_export=sc.n_export, noise=model, tick0=tick0)
    for h, p in enumerate(sc.hmap):
        pos, heading, vel, mho = sc.starts[p]
        assert loop.set_start(h, pos, heading, vel, mho)[0], p
        loop.sim_vel(h, **sc.vels[p])
    if max(sc.sizes) > 1:
        loop.sim_race([sc.sizes[i] for i in sc.host_units], length=5.0)
    return loop


def noisy_fleet(sc, hip, kw, tick0=0):
    fleet = sc.fleet(hip)
    fleet.sim_noise(tick0=tick0, **kw)
    return fleet


def lockstep(sc, hip, oracle, n_ticks, kw, what):
    """Per tick: the host loop seated on the device's own (true) state of the tick before computes the tick; see the module docstring."""
    from graphbasedlocaltrajectoryplanner_amd.planner import KEY_IDS, KEY_NAMES
    assert sc.hmap == list(range(sc.n))                       # every planner is compared in full
    fleet, loop = noisy_fleet(sc, hip, kw), noisy_host(sc, oracle, kw)
    fleet.sim_record(list(range(sc.n)), depth=1)
    prev_traj = [None] * sc.n
    traces, worst, stats = [], dict(obj=0.0, first=0.0, state=0.0), dict(max_cnt=0, keys=set(), drops=set(), est_moved=0)
    for k in range(n_ticks):
        st, th = fleet.sim_state(), fleet.sim_heading()
        for p in range(sc.n):
            a, b = sc.opp_off[p], sc.opp_off[p + 1]
            loop.seat(p, st['now'][p], st['pos_est'][p], st['vel_est'][p], th[p], st['opp_s'][a:b], st['opp_tic'][a:b], prev_traj[p])
        tr = fleet.sim_run(1)[0][0]
        traces.append(tr.copy())
        st2, th2, est = fleet.sim_state(), fleet.sim_heading(), fleet.sim_estimate()
        rec_dev = fleet.sim_record_read()[-1]
        recs = loop.step_sim()
        post = {}
        for p in range(sc.n):
            w, r = "%s tick %d planner %d" % (what, k, p), recs[p]
            assert tr[p, 8] == 0 and not r["failed"], w
            assert tr[p, 0] == KEY_IDS[r["sel"]] and tr[p, 1] == r["now"] == st2['now'][p], "%s: action / clock" % w
            a, b = sc.opp_off[p], sc.opp_off[p + 1]
            d = max(float(np.max(np.abs(st2['pos_est'][p] - r["pos"]))), abs(st2['vel_est'][p] - r["vel"]) / max(abs(r["vel"]), 1.0),
                    float(gd.wrapped(th2[p] - r["theta"])), float(np.max(np.abs(st2['opp_s'][a:b] - r["opp_s"]))) if b > a else 0.0)
            assert d <= TOL, "%s: true state differs by %g" % (w, d)
            worst['state'] = max(worst['state'], d)
            # the trace and the recorder's head hold the TRUE pose
            assert np.array_equal(tr[p, 2:5], [st2['pos_est'][p, 0], st2['pos_est'][p, 1], st2['vel_est'][p]]), "%s: trace vs state" % w
            assert rec_dev[p]["pos_est"] == list(st2['pos_est'][p]) and rec_dev[p]["vel_est"] == st2['vel_est'][p], "%s: recorder head" % w
            post[p] = dict(sel=KEY_NAMES.get(int(st2['sel_action'][p])), now=st2['now'][p], pos=st2['pos_est'][p], vel=st2['vel_est'][p], theta=th2[p])
        recs = loop.step_plan(post=post, want_paths=True)
        for p in range(sc.n):
            w, r = "%s tick %d planner %d" % (what, k, p), recs[p]
            assert not r["failed"], "%s: %s" % (w, r.get("error"))
            # the estimate: the mirror applied to the device's own state, bit for bit
            assert list(est['pos_est'][p]) == r["est_pos"] and est['vel_est'][p] == r["est_vel"], \
                "%s: estimate %s %s vs %s %s" % (w, est['pos_est'][p], est['vel_est'][p], r["est_pos"], r["est_vel"])
            stats['est_moved'] += r["est_pos"] != list(st2['pos_est'][p])
            assert tr[p, 5] == r["cnt"] == len(rec_dev[p]["vehicles"]), "%s: on-track objects %s vs %d" % (w, tr[p, 5], r["cnt"])
            for i, ((rad, v, xy), (hrad, hv, hxy)) in enumerate(zip(rec_dev[p]["vehicles"], r["veh"])):
                d = max(abs(rad - hrad), abs(v - hv), float(np.max(np.abs(xy - hxy))))
                assert d <= TOL, "%s: object %d differs by %g: %s %s vs %s %s" % (w, i, d, v, xy, hv, hxy)
                worst['obj'] = max(worst['obj'], d)
            if r["cnt"]:
                d = float(np.max(np.abs(tr[p, 6:8] - r["first"])))
                assert d <= TOL, "%s: first vehicle %s vs %s" % (w, tr[p, 6:8], r["first"])
                worst['first'] = max(worst['first'], d)
            else:
                assert np.all(np.isnan(tr[p, 6:8])), w
            same_paths(fleet.paths(p), r["paths"], exact=False, what=w)
            dev_traj = fleet.trajectories(p)
            same_trajectories(dev_traj, r["traj"], exact=False, what=w)
            prev_traj[p] = dev_traj[0]
            stats['keys'].add(r["sel"])
            stats['max_cnt'] = max(stats['max_cnt'], r["cnt"])
            stats['drops'] |= set(np.nonzero(~np.asarray(r["keep"], bool))[0].tolist())
    final = (fleet.sim_state(), fleet.sim_heading(), fleet.digest(), fleet.sim_estimate())
    fleet.close()
    # the same scenario in one call: bitwise the single ticks, digest included
    fleet = noisy_fleet(sc, hip, kw)
    one = fleet.sim_run(n_ticks)[0]
    assert np.array_equal(one, np.array(traces), equal_nan=True), "%s: one call differs from the single ticks" % what
    st = fleet.sim_state()
    assert all(np.array_equal(st[key], final[0][key]) for key in st) and np.array_equal(fleet.sim_heading(), final[1])
    assert np.array_equal(fleet.digest(), final[2]) and all(np.array_equal(fleet.sim_estimate()[key], final[3][key]) for key in final[3])
    fleet.close()
    print("\n%s: %d ticks x %d planners against the noisy host loop; actions %s, up to %d objects, largest differences %s" %
          (what, n_ticks, sc.n, sorted(stats['keys']), stats['max_cnt'], worst))
    return stats


# ---- 2. seated differential ---------------------------------------------------------------------------------------------------------------
def test_three_single_planners_against_the_noisy_host_loop(hip, monteblanco, oracle_backend, table, track, c2_start):
    sc = gd.Scenario(monteblanco, table, singles(table, track, c2_start))
    stats = lockstep(sc, hip, oracle_backend, 40, noise_args(3), "three singles")
    assert stats['max_cnt'] >= 2 and stats['est_moved'] == 3 * 40, stats


def test_a_race_of_three_against_the_noisy_host_loop(hip, monteblanco, oracle_backend, table):
    sc = gd.Scenario(monteblanco, table, [race3(table)])
    stats = lockstep(sc, hip, oracle_backend, 40, noise_args(3, seed0=7), "race of 3")
    assert stats['max_cnt'] == 2, stats                      # both mates on the track


def test_seventy_objects_against_the_noisy_host_loop(hip, monteblanco, oracle_backend, table, track, c2_start):
    sc = gd.Scenario(monteblanco, table, [seventy(table, track, c2_start)])
    stats = lockstep(sc, hip, oracle_backend, 10, noise_args(1, seed0=2 ** 63 + 5), "70 objects")
    # the object index passes lane 64, with dropped objects on both sides of it
    assert stats['max_cnt'] > 40 and any(i < 64 for i in stats['drops']) and any(i >= 64 for i in stats['drops']), stats


# ---- 3. identity ------------------------------------------------------------------------------------------------------------------------
def mixed(table, track, start):
    s = singles(table, track, start)
    return [s[0], race3(table), s[1]]


def test_zero_sigmas_and_cleared_noise_leave_the_trace_untouched(hip, monteblanco, table, track, c2_start):
    sc = gd.Scenario(monteblanco, table, mixed(table, track, c2_start))
    plain = sc.fleet(hip)
    ref = plain.sim_run(30)[0]
    ref_state, ref_digest = plain.sim_state(), plain.digest()
    assert np.array_equal(plain.sim_estimate()['pos_est'], ref_state['pos_est']) and np.array_equal(plain.sim_estimate()['vel_est'], ref_state['vel_est'])
    plain.close()
    zero = sc.fleet(hip)
    zero.sim_noise(seed=noise_args(sc.n)["seed"])             # every sigma 0
    cleared = noisy_fleet(sc, hip, noise_args(sc.n))
    cleared.sim_noise(None)
    for what, fleet in (("all sigmas 0", zero), ("set, then cleared", cleared)):
        tr = fleet.sim_run(30)[0]
        assert np.array_equal(tr, ref, equal_nan=True), what
        st = fleet.sim_state()
        assert all(np.array_equal(st[k], ref_state[k]) for k in st) and np.array_equal(fleet.digest(), ref_digest), what
        est = fleet.sim_estimate()
        assert np.array_equal(est['pos_est'], st['pos_est']) and np.array_equal(est['vel_est'], st['vel_est']), what
        fleet.close()
    # and the noise is not a no-op on this scenario
    noisy = noisy_fleet(sc, hip, noise_args(sc.n))
    assert not np.array_equal(noisy.sim_run(30)[0], ref, equal_nan=True)
    noisy.close()


# ---- 4. layout independence ------------------------------------------------------------------------------------------------------------
def test_a_planner_computes_the_same_alone_and_at_index_5_of_70(hip, monteblanco, table, track, c2_start):
    s = singles(table, track, c2_start)
    S = 0xC0FFEE0123456789
    kw1 = dict(nu.SIGMAS, seed=S)
    alone = noisy_fleet(gd.Scenario(monteblanco, table, [s[0]]), hip, kw1)
    ref = alone.sim_run(30)[0]
    alone.close()
    units = [s[k % 3] for k in (1, 2, 1, 2, 1)] + [s[0]] + [s[k % 3] for k in range(64)]          # s[0] at 5, again at 6, 9, ..
    sc = gd.Scenario(monteblanco, table, units)
    assert sc.n == 70 and units[6] is s[0]
    seeds = np.arange(70, dtype=np.uint64) + np.uint64(99)
    seeds[5] = S
    fleet = noisy_fleet(sc, hip, dict(nu.SIGMAS, seed=seeds))
    first = fleet.sim_run(1)[0]
    est = fleet.sim_estimate()
    rest = fleet.sim_run(29)[0]
    fleet.close()
    tr = np.concatenate((first, rest))
    assert np.array_equal(tr[:, 5], ref[:, 0], equal_nan=True)
    # the same planner under another seed: the same true pose on the first tick, another estimate
    assert np.array_equal(first[0, 5, 2:5], first[0, 6, 2:5])
    assert np.all(est['pos_est'][5] != est['pos_est'][6]) and not np.array_equal(tr[:, 6], tr[:, 5], equal_nan=True)


# ---- 5. tick0 ---------------------------------------------------------------------------------------------------------------------------
def test_tick0_continues_a_run_and_reproduces_a_restored_snapshot(hip, monteblanco, table, track, c2_start):
    sc = gd.Scenario(monteblanco, table, mixed(table, track, c2_start))
    kw = noise_args(sc.n, seed0=31)
    whole = noisy_fleet(sc, hip, kw)
    ref = whole.sim_run(20)[0]
    ref_est = whole.sim_estimate()
    whole.close()
    fleet = noisy_fleet(sc, hip, kw)
    a = fleet.sim_run(10)[0]
    fleet.sim_snapshot(0)
    fleet.sim_noise(tick0=10, **kw)
    b = fleet.sim_run(10)[0]
    assert np.array_equal(np.concatenate((a, b)), ref, equal_nan=True)
    assert all(np.array_equal(fleet.sim_estimate()[k], ref_est[k]) for k in ref_est)
    fleet.sim_restore(0)
    fleet.sim_noise(tick0=10, **kw)
    c = fleet.sim_run(10)[0]
    assert np.array_equal(c, ref[10:], equal_nan=True)
    # without tick0 the second half is another one
    fleet.sim_restore(0)
    fleet.sim_noise(**kw)
    assert not np.array_equal(fleet.sim_run(10)[0], ref[10:], equal_nan=True)
    fleet.close()


# ---- 6. telemetry ---------------------------------------------------------------------------------------------------------------------------
TELE_RADIUS = 12.92                # inside the true clearances of the 30 ticks (12.99 .. 12.85 m): contact from the middle of the run on
TELE_AHEAD = 14.0


def tele_unit(table, start):
    """One planner, one static object standing on the race line ahead of it."""
    i0 = int(np.argmin((table.x - start['pos'][0]) ** 2 + (table.y - start['pos'][1]) ** 2))
    pos, heading = sl.race_line_pose(table, float(table.s_rl[i0]) + TELE_AHEAD)
    e = dict(opponents=[], static=[(pos[0], pos[1], heading, 0.0, 4.0)], pref=sl.DEFAULT_PREF, pos_est=tuple(start['pos']), vel_est=0.0, zone_gids=[])
    return gd.single("tele", dict(entry=e, vel=sl.C2_VEL), start)


def tele_feeds(oracle, table, sc, trace, kw):
    """sim.Telemetry fed from the device's trace, once with the TRUE position of the object the planner was handed and once with the
    PERCEIVED one (radius and on-track decision of the perceived object in both)."""
    from graphbasedlocaltrajectoryplanner_amd import sim
    model = sim.NoiseModel(1, **kw)
    feed = tu.TraceFeed(oracle, table, sc.entries, sc.sizes)
    out = {}
    for which in ("true", "perceived"):
        mir = sim.Telemetry(1, [1], TELE_RADIUS, tu.track_length(sc.lat), oracle.raceline_s, sc.dt)
        for k, tr in enumerate(trace):
            row = tuple(float(v) for v in sc.entries[0]["static"][0])
            seen = model.objects(0, k, [row])
            kept = feed.on_track(seen)[0]
            assert (kept is not None) == (tr[0, 5] == 1), k
            objs = [] if kept is None else [(row[0], row[1], kept[2]) if which == "true" else kept]
            mir.update(k, [dict(live=True, sel=int(tr[0, 0]), now=float(tr[0, 1]), pos=(float(tr[0, 2]), float(tr[0, 3])), vel=float(tr[0, 4]), objects=objs)])
        out[which] = mir.as_dict()
    return out


def test_telemetry_measures_against_the_true_positions(hip, monteblanco, oracle_backend, table, c2_start):
    sc = gd.Scenario(monteblanco, table, [tele_unit(table, c2_start)])
    kw = dict(seed=12, obj_pos=1.0)
    fleet = noisy_fleet(sc, hip, kw)
    fleet.sim_telemetry(radius=TELE_RADIUS)
    trace = fleet.sim_run(30)[0]
    dev = fleet.sim_telemetry_read()
    fleet.close()
    assert np.all(trace[:, 0, 8] == 0) and np.sum(trace[:, 0, 5]) >= 25
    m = tele_feeds(oracle_backend, table, sc, trace, kw)
    print("device clear_min %r contacts %d; mirror on truth %r %d; on the perceived positions %r %d" % (
        dev["clear_min"][0], dev["contact_ticks"][0], m["true"]["clear_min"][0], m["true"]["contact_ticks"][0],
        m["perceived"]["clear_min"][0], m["perceived"]["contact_ticks"][0]))
    tu.compare(dev, m["true"], 1e-9, "telemetry against truth")
    assert 0 < dev["contact_ticks"][0] < 30
    assert dev["clear_min"][0] != m["perceived"]["clear_min"][0] and dev["contact_ticks"][0] != m["perceived"]["contact_ticks"][0]


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_keep_the_previous_noise(hip, monteblanco, table, track, c2_start):
    from graphbasedlocaltrajectoryplanner_amd import sim
    from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
    from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet
    sc = gd.Scenario(monteblanco, table, singles(table, track, c2_start)[:2])
    bare = Fleet(hip, 2)
    with pytest.raises(BackendError, match="sim_setup first"):
        bare.sim_noise(seed=1, pos=0.1)
    with pytest.raises(BackendError, match="sim_setup first"):
        bare.sim_estimate()
    bare.close()
    kw = noise_args(2, seed0=5)
    fleet = noisy_fleet(sc, hip, kw)
    model = sim.NoiseModel(2, **kw)
    tick = 0

    def still_in_force():
        nonlocal tick
        fleet.sim_run(1)
        st, est = fleet.sim_state(), fleet.sim_estimate()
        for p in range(2):
            pos, vel = model.ego(p, tick, st['pos_est'][p], st['vel_est'][p])
            assert list(est['pos_est'][p]) == pos and est['vel_est'][p] == vel and pos != list(st['pos_est'][p]), (tick, p)
        tick += 1
    still_in_force()
    for bad, msg in ((dict(pos=[0.1, -0.1]), "sigma"), (dict(obj_vel=[np.nan, 0.0]), "sigma"), (dict(vel=np.inf), "sigma"), (dict(tick0=-1), "tick0")):
        with pytest.raises(BackendError, match=msg):
            fleet.sim_noise(seed=99, **bad)
        still_in_force()
    fleet.close()
