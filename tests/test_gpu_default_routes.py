"""GPU: the tick routes a user gets by default, against the oracle.

tests/conftest.py pins LTPL_PIPELINE_MIN_SCEN=64 and LTPL_FOLLOW_EMIT_MIN_SCEN=256 for the suite, so that its batches exercise the
headline's pipeline. Every handle here is created WITHOUT those pins (the environment is read at ltpl_create), so ltpl_tick_batch picks
its routes by the product thresholds (include/ltpl_hip.h):
  four-wave -> one-wave path teams at 64 scenarios; fused k_tick -> batch pipeline above 2 (or 1) workgroups per compute unit (513 or
  257 on an MI355X); generic vx / ax written by the lane kernel from 256; follow jobs finished by the lane kernel from 8 192; scenarios
  planned in start-layer order from 2 048; the pipeline at every size in the long-horizon mode and on lattices whose fused tick does
  not fit in LDS (C5 with a 120 .. 190 m horizon).
Every result is compared with OracleBackend.tick_batch on the same packed inputs (test_gpu_vel.compare_tick: integers and node lists
bit-exact, vx / ax element-wise to 1e-5, coefficients and path_param under the suite's tolerances). Where the scenarios of a smaller
batch are a prefix of a larger one, the oracle's result for the larger batch is reused (the oracle plans every scenario on its own)."""
import numpy as np
import pytest

from test_gpu_vel import compare_tick, make_tick_inputs
from test_gpu_configs import c5_follow_scenarios, vel_inputs
from test_gpu_persistent_tick import assert_same_tick, copy_of, device_synchronize
from graphbasedlocaltrajectoryplanner_amd import _capi
from graphbasedlocaltrajectoryplanner_amd.scenario_gen import c2_scenarios, random_scenarios
from graphbasedlocaltrajectoryplanner_amd.synthetic_lattice import (c3_lattice, c5_lattice, make_oval_lattice,
                                                                    scattered_obstacle_scenarios)

pytestmark = pytest.mark.gpu

W_LAST = [0.0, 0.5, 0.8]
PINS = ("LTPL_PIPELINE_MIN_SCEN", "LTPL_FOLLOW_EMIT_MIN_SCEN")


def default_backend(lat, **kw):
    """A handle on the product's route thresholds."""
    with pytest.MonkeyPatch.context() as mp:
        for name in PINS:
            mp.delenv(name, raising=False)
        return _capi.HipBackend(lat, **kw)


def sub_batch(scen, vels, vel, lo, hi):
    """Scenarios lo .. hi-1 of a batch (scenarios, vehicle speeds, TickVelBatch) as a batch of their own."""
    veh = [x for x in vels[lo:hi] if len(x)]
    t = vel.struct
    v = _capi.TickVelBatch(vel.params, hi - lo, vel.vel_plan[lo:hi], vel.vel_est[lo:hi],
                           np.column_stack((vel.pos_x[lo:hi], vel.pos_y[lo:hi])), np.concatenate(veh) if veh else np.zeros(0),
                           gg=(t.gg_ax, t.gg_ay), gg_brake_scale=t.gg_brake_scale, safety_d=t.safety_d, v_max_offset=t.v_max_offset)
    return _capi.PathsBatch(scen[lo:hi], w_last_edges=W_LAST), v


class Rows(object):
    """The first n scenarios of results for consecutive parts of one batch (every per-scenario array joined and cut to n rows)."""

    def __init__(self, parts, rows, n):
        self.n_scen = n
        for name, val in vars(parts[0]).items():
            if isinstance(val, np.ndarray) and val.ndim >= 1 and val.shape[0] == rows[0]:
                setattr(self, name, np.concatenate([getattr(p, name) for p in parts])[:n])


def oracle_tick(orc, scen, vels, vel, parts=8):
    """OracleBackend.tick_batch of the whole batch, in parts planned on threads (the oracle plans every scenario on its own, and its
    C entry point holds no state between calls: the outputs are those of one call). Returns a function n -> (paths, vel) of the first
    n scenarios."""
    from concurrent.futures import ThreadPoolExecutor
    bounds = np.linspace(0, len(scen), parts + 1).astype(int)
    with ThreadPoolExecutor(parts) as ex:
        outs = list(ex.map(lambda b: orc.tick_batch(*sub_batch(scen, vels, vel, b[0], b[1])), zip(bounds[:-1], bounds[1:])))
    rows = list(np.diff(bounds))
    return lambda n: (Rows([o[0] for o in outs], rows, n), Rows([o[1] for o in outs], rows, n))


def counts(res, vel):
    valid = res.valid == 1
    return {"follow": int((valid & (res.action_id == _capi.ACT_FOLLOW)).sum()),
            "reduced": int((valid & (res.reduced != 0)).sum()),
            "vplan0": int((np.asarray(vel.vel_plan) == 0.0).sum()),
            "paths": int(valid.sum())}


# ---------------------------------------------------------------- (a) Monteblanco at every size threshold of the route table

SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 8191, 8192)
N_ALL = 8192


@pytest.fixture(scope="module")
def mb_random(monteblanco, oracle_backend):
    """make_tick_inputs' batch of 8 192 scenarios with 6 vehicles each (every 17th starts at vel_plan = 0) and the oracle's result."""
    _, vel = make_tick_inputs(monteblanco, N_ALL, seed=71, n_veh=6)
    scen, vels = random_scenarios(monteblanco, N_ALL, seed=71, n_veh=6)             # (the scenarios make_tick_inputs packed)
    return scen, vels, vel, oracle_tick(oracle_backend, scen, vels, vel)


@pytest.fixture(scope="module")
def mb_c2(monteblanco, oracle_backend):
    """C2 scenarios with an opponent 20 .. 80 m ahead in every one: follow jobs on both sides of 8 192."""
    scen, vels = c2_scenarios(monteblanco, N_ALL, seed=72, lead_gap=(20.0, 80.0))
    rng = np.random.default_rng(72)
    vplan = rng.uniform(5.0, 60.0, N_ALL)
    vplan[::17] = 0.0
    pos = np.array([monteblanco.node_pos[monteblanco.layer_off[s['start_node'][0]] + s['start_node'][1]] for s in scen])
    vel = _capi.TickVelBatch(_capi.VelParamSet(len_veh=monteblanco.veh_length), N_ALL, vplan, vplan + rng.uniform(-1, 1, N_ALL), pos,
                             np.concatenate(vels))
    return scen, vels, vel, oracle_tick(oracle_backend, scen, vels, vel)


@pytest.fixture(scope="module")
def mb_default(monteblanco):
    hip = default_backend(monteblanco)
    yield hip
    hip.close()


@pytest.mark.parametrize("n", SIZES)
def test_monteblanco_default_routes_match_oracle_at_every_threshold(monteblanco, mb_default, mb_random, n):
    scen, vels, vel, ref = mb_random
    batch, v = sub_batch(scen, vels, vel, 0, n)
    res, vres = mb_default.tick_batch(batch, v)
    compare_tick(res, vres, *ref(n))
    c = counts(res, v)
    assert c["paths"] >= n, c
    assert c["vplan0"] >= n // 17, c                                   # (scenario 0 is one of them)
    if n >= 255:
        assert c["follow"] >= n // 2 and c["reduced"] >= n // 200, c


@pytest.mark.parametrize("n", (2047, 2048, 8191, 8192))
def test_monteblanco_default_routes_with_an_opponent_ahead_match_oracle(monteblanco, mb_default, mb_c2, n):
    scen, vels, vel, ref = mb_c2
    batch, v = sub_batch(scen, vels, vel, 0, n)
    res, vres = mb_default.tick_batch(batch, v)
    compare_tick(res, vres, *ref(n))
    c = counts(res, v)
    assert c["follow"] >= n // 2 and c["vplan0"] >= n // 17, c


# ---------------------------------------------------------------- (b) one lattice per plan class and sweep form

def c3_case():
    lat = c3_lattice()
    scen, vels = scattered_obstacle_scenarios(lat, 600, n_obj=32, seed=81)
    return lat, scen, vels


def c5_case(horizon):
    def make():
        lat = c5_lattice(horizon=horizon)
        scen, vels = c5_follow_scenarios(lat, 600, seed=82)
        return lat, scen, vels
    return make


def wide_case():
    lat = make_oval_lattice(num_layers=60, nodes_per_layer=70, layer_spacing=10.0, lat_resolution=0.25, lat_steps=3,
                            radius=60.0, horizon=100.0, v_straight=40.0)
    scen, vels = scattered_obstacle_scenarios(lat, 600, n_obj=6, seed=83)
    return lat, scen, vels


def open_case(lat):
    scen, vels = random_scenarios(lat, 600, seed=84, n_veh=6)
    for sc in scen:                                                    # the last layers of an open track have no planning range
        sl = min(sc['start_node'][0], lat.num_layers - 8)
        sc['start_node'] = (sl, int(lat.raceline_index[sl]))
        sc['last_nodes'] = None
    return lat, scen, vels


CASES = {"c3": c3_case, "c5_100m": c5_case(100.0), "c5_150m_band": c5_case(150.0), "c5_300m_long_horizon": c5_case(300.0),
         "wide_70_nodes": wide_case, "open_track": open_case}


@pytest.mark.parametrize("name", sorted(CASES))
def test_lattice_classes_default_routes_match_oracle(request, name):
    from oracle.oracle_lib import OracleBackend
    lat, scen, vels = CASES[name](request.getfixturevalue("open_lattice")) if name == "open_track" else CASES[name]()
    vel = vel_inputs(lat, scen, vels, 85)
    ref = oracle_tick(OracleBackend(lat), scen, vels, vel)
    hip = default_backend(lat)
    try:
        for n in (1, 64, 300, 600):
            batch, v = sub_batch(scen, vels, vel, 0, n)
            res, vres = hip.tick_batch(batch, v)
            compare_tick(res, vres, *ref(n))
            assert counts(res, v)["paths"] >= n, (n, counts(res, v))
        if name.startswith("c5"):
            assert counts(res, v)["follow"] >= 300, counts(res, v)        # the follow-mode profile really ran
    finally:
        hip.close()


# ---------------------------------------------------------------- (c) persistent single tick on inputs that move every tick

N_VEH_CYCLE = (96, 0, 1, 96, 5, 0, 48, 2)          # (the first tick is the largest: the staging buffers never grow, the kernel stays resident)


def moving_ticks(lat, n_ticks, seed):
    """Single ticks whose vehicle count (0, 1, 96 = 192 obstacle positions), zone set (on / off), previous solution and velocity inputs
    change every tick: every input offset of the tick's argument block moves."""
    params = _capi.VelParamSet(len_veh=lat.veh_length)
    rng = np.random.default_rng(seed)
    ticks, n_pos, zones = [], [], []
    for i in range(n_ticks):
        n_veh = N_VEH_CYCLE[i % len(N_VEH_CYCLE)]
        scen, vels = random_scenarios(lat, 1, seed=seed * 1000 + i, n_veh=n_veh, zone_prob=float(i % 2 == 0), last_prob=0.5)
        sl, sn = scen[0]['start_node']
        pos = lat.node_pos[lat.layer_off[sl] + sn][None, :]
        vp = 0.0 if i % 5 == 3 else float(rng.uniform(1.0, 55.0))
        ticks.append((_capi.PathsBatch(scen, w_last_edges=W_LAST),
                      _capi.TickVelBatch(params, 1, np.full(1, vp), np.full(1, vp + 0.3), pos, vels[0] if n_veh else np.zeros(0))))
        n_pos.append(sum(len(pts) for _, pts in scen[0]["vehicles"]))
        zones.append(len(scen[0]["zone_gids"]))
    assert min(n_pos) == 0 and max(n_pos) == 192 and len(set(n_pos)) >= 5, n_pos
    assert min(zones) == 0 and max(zones) > 0, zones
    return ticks


def run_moving_ticks(lat, n_ticks, seed, monkeypatch):
    """Every tick through the persistent handle against the oracle, then every tick through a launched handle against the persistent
    handle's outputs, bit for bit. Returns the persistent stats. (The launched handle runs after the persistent sequence: a kernel it
    launched on a stream that shares a hardware queue with the resident kernel would wait for the idle limit, and the next persistent
    tick would start the resident kernel again.)"""
    from oracle.oracle_lib import OracleBackend
    monkeypatch.setenv("LTPL_PERSIST_IDLE_MS", "100")
    ticks = moving_ticks(lat, n_ticks, seed)
    orc = OracleBackend(lat)
    pers = default_backend(lat, persistent_tick=True)
    try:
        got, n_follow = [], 0
        for b, v in ticks:
            res = pers.tick_batch(b, v)
            compare_tick(*res, *orc.tick_batch(b, v))
            got.append(copy_of(res))
            n_follow += int(((res[0].action_id == _capi.ACT_FOLLOW) & (res[0].valid == 1)).sum())
        st = pers.persistent_stats()
    finally:
        pers.close()                                               # (a resident kernel: ltpl_destroy makes it leave first)
        device_synchronize()                                       # nothing of it is left on the device
    launched = default_backend(lat)
    try:
        for i, (b, v) in enumerate(ticks):
            assert_same_tick(got[i], launched.tick_batch(b, v), "tick %d" % i)
    finally:
        launched.close()
    return st, n_follow


def test_persistent_tick_on_moving_inputs_matches_launched_tick_and_oracle(monteblanco, monkeypatch):
    st, n_follow = run_moving_ticks(monteblanco, 32, seed=91, monkeypatch=monkeypatch)
    assert st["enabled"] == 1 and st["ticks"] == 32 and st["launches"] == 1, st
    assert n_follow >= 3, n_follow


def test_persistent_tick_on_a_lattice_whose_fused_tick_does_not_fit_runs_the_pipeline(monkeypatch):
    """C5 with a 150 m horizon: the fused tick does not fit in LDS, so a persistent handle serves single ticks with the launched pipeline
    (four-wave path team) -- no resident kernel is ever started."""
    st, _ = run_moving_ticks(c5_lattice(horizon=150.0), 24, seed=92, monkeypatch=monkeypatch)
    assert st["launches"] == 0 and st["resident"] == 0, st
