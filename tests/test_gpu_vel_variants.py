"""GPU: every velocity-kernel variant on every tick route, against the oracle.

vel_variant() (csrc/ltpl_hip.hip) compiles the velocity stage six times: exponent 1 / 2 / general pow x one-row / interpolated machine
table. k_vel_lanes, k_tick (compile-time and runtime plan class), k_tick_persistent and k_vel_profile exist once per variant, and only
(exponent 1, one row) is the affine fast path: the other five go through branches of their own in every sweep. The rest of the suite
runs its tick-level comparisons at VelParamSet()'s defaults, i.e. on that one variant. Here: one parameter set per variant (SETS), each
of which also moves tick-level fields off their defaults (controller type, a non-square gg, safety_d, v_max_offset, a v_max low enough
for the solver's "> v_max" break), on every route ltpl_tick_batch can take, each result compared with OracleBackend.tick_batch on the
same packed inputs through test_gpu_vel.compare_tick (integers, node lists, too_close, vel_bound exact; vx / ax element-wise under the
project's 1e-5 with its floors).

A comparison on inputs that never reach the forked code proves nothing, so every case first asserts ON THE ORACLE'S RESULT that the
batch is worth comparing (worth_comparing), and test_every_set_moves_the_profiles_and_both_flag_values_occur checks that a set's
profiles differ from the control set's.

The C2 batches place the leading opponent 8 .. 80 m ahead (not 20 .. 80 m as elsewhere in the suite): too_close is obj_dist < safety_d +
vehicle length, and with safety_d = 10 or 15 a gap of at least 20 m puts every follow slot of those two sets on one side of it.

What the oracle counted and what the comparison saw is in the comment block below (every case prints a line "variants: ..."; run
with `pytest -s`).
"""
# One run on an MI355X. Per (parameter set, route): the worst element-wise relative error of vx (|vx| >= 1 m/s) and ax (|ax| >= 0.5 m/s^2)
# over the route's cases -- recorded, not asserted: the bound is the project's 1e-5 -- and per case "generator n: valid follow slots /
# reduced-horizon slots / follow slots with too_close / valid slots with vel_bound == 0" as counted on the ORACLE's result (the
# quantities worth_comparing asserts).
#
# Exponent 2 stands apart by four orders of magnitude (ax up to 4.4e-6). It is the conditioning of the model, not the kernels: at the
# friction limit the tire share is ax_max * sqrt(1 - q^2) with 1 - q^2 next to zero, and the square root turns a last-bit difference of
# q (the kernels carry w = v^2 and multiply by |kappa| / ay_max, the oracle squares vx and divides by radius and ay_max) into ~1e-8. The oracle's own result for the exp2_row batch of 600
# random scenarios moves by vx 3.5e-8 / ax 1.6e-6 when both gg values are raised by one ulp (exp1p5_row: 3.9e-12 / 3.5e-10, exp1_row:
# 2.7e-13 / 1.1e-12).
#
#   exp1_row     k_tick PlanA4          vx 4.1e-13 ax 2.0e-12   random 1: 1/0/1/1; random 5: 5/0/4/3; random 48: 43/4/18/13; c2 48: 46/0/21/7
#   exp1_table   k_tick PlanA4          vx 5.8e-13 ax 2.0e-12   random 1: 1/0/0/0; random 5: 5/0/2/2; random 48: 43/4/10/14; c2 48: 46/0/10/7
#   exp1p5_row   k_tick PlanA4          vx 2.1e-12 ax 2.7e-10   random 1: 1/0/1/1; random 5: 5/0/4/3; random 48: 43/4/18/14; c2 48: 46/0/21/7
#   exp1p5_table k_tick PlanA4          vx 5.5e-12 ax 7.2e-10   random 1: 1/0/0/0; random 5: 5/0/0/2; random 48: 43/4/3/13; c2 48: 46/0/6/8
#   exp2_row     k_tick PlanA4          vx 5.1e-08 ax 1.2e-06   random 1: 1/0/1/1; random 5: 5/0/4/3; random 48: 43/4/18/14; c2 48: 46/0/21/8
#   exp2_table   k_tick PlanA4          vx 3.0e-09 ax 2.2e-07   random 1: 1/0/1/0; random 5: 5/0/4/2; random 48: 43/4/19/13; c2 48: 46/0/32/7
#   exp1_row     pipeline k_vel_final   vx 4.1e-13 ax 2.0e-12   random 96: 85/4/32/27; c2 96: 93/0/37/23
#   exp1_table   pipeline k_vel_final   vx 6.0e-13 ax 3.1e-12   random 96: 85/4/18/27; c2 96: 93/0/16/21
#   exp1p5_row   pipeline k_vel_final   vx 2.4e-12 ax 2.7e-10   random 96: 85/4/32/27; c2 96: 93/0/37/21
#   exp1p5_table pipeline k_vel_final   vx 6.5e-12 ax 7.2e-10   random 96: 85/4/6/29; c2 96: 93/0/10/22
#   exp2_row     pipeline k_vel_final   vx 3.5e-08 ax 1.6e-06   random 96: 85/4/32/30; c2 96: 93/0/37/23
#   exp2_table   pipeline k_vel_final   vx 4.3e-09 ax 2.2e-07   random 96: 85/4/38/27; c2 96: 93/0/59/19
#   exp1_row     pipeline lanes emit    vx 1.6e-12 ax 1.4e-11   c2 600: 596/0/230/147; random 600: 542/7/143/137
#   exp1_table   pipeline lanes emit    vx 1.5e-12 ax 3.1e-12   c2 600: 596/0/107/142; random 600: 542/7/50/126
#   exp1p5_row   pipeline lanes emit    vx 4.7e-12 ax 8.5e-10   c2 600: 596/0/230/138; random 600: 542/7/143/122
#   exp1p5_table pipeline lanes emit    vx 1.2e-11 ax 2.3e-09   c2 600: 596/0/61/131; random 600: 542/7/14/150
#   exp2_row     pipeline lanes emit    vx 1.0e-07 ax 4.4e-06   c2 600: 596/0/230/148; random 600: 542/7/143/152
#   exp2_table   pipeline lanes emit    vx 8.1e-09 ax 3.5e-07   c2 600: 596/0/329/123; random 600: 542/7/186/125
#   exp1_row     pipeline two-wave      vx 1.6e-12 ax 1.4e-11   c2 600: 596/0/230/147; random 600: 542/7/143/137
#   exp1_table   pipeline two-wave      vx 1.5e-12 ax 3.1e-12   c2 600: 596/0/107/142; random 600: 542/7/50/126
#   exp1p5_row   pipeline two-wave      vx 4.7e-12 ax 8.5e-10   c2 600: 596/0/230/138; random 600: 542/7/143/122
#   exp1p5_table pipeline two-wave      vx 1.2e-11 ax 2.3e-09   c2 600: 596/0/61/131; random 600: 542/7/14/150
#   exp2_row     pipeline two-wave      vx 1.0e-07 ax 4.4e-06   c2 600: 596/0/230/148; random 600: 542/7/143/152
#   exp2_table   pipeline two-wave      vx 8.1e-09 ax 3.5e-07   c2 600: 596/0/329/123; random 600: 542/7/186/125
#   exp1_row     k_tick grid (default)  vx 5.9e-13 ax 3.4e-12   c2 300: 297/0/115/69; random 300: 264/6/82/73
#   exp1_table   k_tick grid (default)  vx 7.7e-13 ax 3.1e-12   c2 300: 297/0/55/66; random 300: 264/6/32/67
#   exp1p5_row   k_tick grid (default)  vx 2.4e-12 ax 2.7e-10   c2 300: 297/0/115/62; random 300: 264/6/82/65
#   exp1p5_table k_tick grid (default)  vx 6.3e-12 ax 7.2e-10   c2 300: 297/0/33/60; random 300: 264/6/8/76
#   exp2_row     k_tick grid (default)  vx 1.0e-07 ax 4.4e-06   c2 300: 297/0/115/69; random 300: 264/6/82/80
#   exp2_table   k_tick grid (default)  vx 4.4e-09 ax 2.2e-07   c2 300: 297/0/174/54; random 300: 264/6/104/65
#   exp1_row     k_tick PlanRt (berlin) vx 9.0e-14 ax 2.3e-13   random 5: 5/0/2/1
#   exp1_table   k_tick PlanRt (berlin) vx 1.3e-13 ax 2.7e-13   random 5: 5/0/0/0
#   exp1p5_row   k_tick PlanRt (berlin) vx 1.6e-12 ax 2.2e-11   random 5: 5/0/2/1
#   exp1p5_table k_tick PlanRt (berlin) vx 2.5e-12 ax 2.3e-10   random 5: 5/0/0/0
#   exp2_row     k_tick PlanRt (berlin) vx 1.4e-09 ax 3.0e-07   random 5: 5/0/2/1
#   exp2_table   k_tick PlanRt (berlin) vx 1.1e-09 ax 7.1e-08   random 5: 5/0/3/0
#   exp1_table   k_tick_persistent      vx 1.0e-15 ax 9.4e-14   6 ticks (0 / 3 / 8 vehicles)
#   exp2_row     k_tick_persistent      vx 3.3e-09 ax 8.2e-08   6 ticks (0 / 3 / 8 vehicles)
#   exp2_table   k_tick_persistent      vx 1.5e-09 ax 1.4e-07   6 ticks (0 / 3 / 8 vehicles)
#   exp1p5_row   k_tick_persistent      vx 2.1e-12 ax 1.9e-10   6 ticks (0 / 3 / 8 vehicles)
#   exp1p5_table k_tick_persistent      vx 2.3e-12 ax 1.6e-10   6 ticks (0 / 3 / 8 vehicles)
#   exp1_row     k_tick_persistent      vx 1.1e-14 ax 6.2e-14   6 ticks (0 / 3 / 8 vehicles)
# worst over everything: vx 1.0e-07, ax 4.4e-06
import numpy as np
import pytest

from test_gpu_vel import compare_tick
from test_gpu_default_routes import default_backend, sub_batch, oracle_tick, W_LAST
from test_gpu_persistent_tick import device_synchronize
from helpers import ELEM_FLOOR_VX, ELEM_FLOOR_AX
from graphbasedlocaltrajectoryplanner_amd import _capi
from graphbasedlocaltrajectoryplanner_amd.scenario_gen import c2_scenarios, random_scenarios

pytestmark = pytest.mark.gpu

CTRL_PARAMS = {"c_p": 1.15, "k_d": 0.025, "k_p": 0.2, "tan_w": 15.0}

# name: (dyn_model_exp, ax_max_machines, controller, gg, safety_d, v_max_offset, v_max). One set per kernel variant; the first is the
# set the rest of the suite tests (the control). Every tick-level field is off its default in one set or more.
SETS = {
    "exp1_row": (1.0, [[100.0, 5.0]], "PD", (5.0, 5.0), 30.0, 0.1, 100.0),
    "exp1_table": (1.0, [[0.0, 6.0], [36.0, 6.0], [48.0, 4.8], [60.0, 3.9], [72.0, 2.5]], "PD", (4.0, 7.0), 15.0, 0.1, 65.0),
    "exp2_row": (2.0, [[100.0, 5.0]], "PDtan", (6.5, 3.5), 30.0, 0.5, 100.0),
    "exp2_table": (2.0, [[0.0, 6.0], [36.0, 6.0], [72.0, 2.5]], "PD", (5.0, 5.0), 40.0, 0.1, 45.0),
    "exp1p5_row": (1.5, [[100.0, 4.0]], "PD", (3.0, 8.0), 30.0, 0.1, 100.0),
    "exp1p5_table": (1.5, [[0.0, 6.0], [72.0, 2.5]], "PDtan", (8.0, 8.0), 10.0, 0.02, 70.0),
}
CONTROL = "exp1_row"
NAMES = sorted(SETS)
N_BIG = 600
SEED = 5


def test_one_set_per_variant_and_every_tick_level_field_moves():
    variants = {(1 if s[0] == 1.0 else 2 if s[0] == 2.0 else 0, len(s[1]) == 1) for s in SETS.values()}
    assert len(variants) == 6 == len(SETS)
    ctl = SETS[CONTROL]
    assert ctl[2:] == ("PD", (5.0, 5.0), 30.0, 0.1, 100.0) and ctl[:2] == (1.0, [[100.0, 5.0]])       # TickVelBatch's / VelParamSet's defaults
    for field in range(2, 7):
        assert any(s[field] != ctl[field] for s in SETS.values()), field
    assert any(s[3][0] != s[3][1] for s in SETS.values())                                              # a non-square gg


def params_of(lat, name):
    e, axm, ctrl = SETS[name][:3]
    return _capi.VelParamSet(dyn_model_exp=e, drag_coeff=0.85, m_veh=1000.0, len_veh=lat.veh_length, v_max=SETS[name][6],
                             ax_max_machines=axm, follow_control_type=ctrl, follow_control_params=dict(CTRL_PARAMS))


def vel_batch(lat, name, scen, vels, seed):
    """Velocity inputs of a batch at parameter set ``name``. The same seed gives every set the same draws (vel_plan scaled to the set's
    range: the entry point refuses vel_plan > v_max + 0.1), every 17th scenario starts at vel_plan = 0 as in make_tick_inputs."""
    _, _, _, gg, safety_d, v_max_offset, v_max = SETS[name]
    n = len(scen)
    rng = np.random.default_rng(seed)
    vplan = rng.uniform(0.0, 1.0, n) * min(60.0, v_max)
    vplan[::17] = 0.0
    pos = np.array([lat.node_pos[lat.layer_off[s['start_node'][0]] + s['start_node'][1]] for s in scen])
    pos = pos + rng.uniform(-0.3, 0.3, pos.shape)
    veh = [x for x in vels if len(x)]
    return _capi.TickVelBatch(params_of(lat, name), n, vplan, vplan + rng.uniform(-1, 1, n), pos,
                              np.concatenate(veh) if veh else np.zeros(0), gg=gg, safety_d=safety_d, v_max_offset=v_max_offset)


def scenarios_of(lat, gen, n):
    if gen == "c2":
        return c2_scenarios(lat, n, seed=SEED, lead_gap=(8.0, 80.0))
    return random_scenarios(lat, n, seed=SEED, n_veh=8)


class Cases(object):
    """(parameter set, generator) -> scenarios, velocity inputs and the oracle's result for N_BIG scenarios; made on first use, kept for
    the module. A case of n scenarios is the first n of them (the oracle plans every scenario on its own)."""

    def __init__(self, lat, orc, n_big=N_BIG):
        self.lat, self.orc, self.n_big, self.scen, self.made = lat, orc, n_big, {}, {}

    def get(self, name, gen):
        if gen not in self.scen:
            self.scen[gen] = scenarios_of(self.lat, gen, self.n_big)
        if (name, gen) not in self.made:
            scen, vels = self.scen[gen]
            vel = vel_batch(self.lat, name, scen, vels, SEED + 1)
            self.made[name, gen] = (scen, vels, vel, oracle_tick(self.orc, scen, vels, vel))
        return self.made[name, gen]


@pytest.fixture(scope="module")
def cases(monteblanco, oracle_backend):
    return Cases(monteblanco, oracle_backend)


def activity(ref, vref, v):
    """What the ORACLE's result of a case holds."""
    valid = ref.valid == 1
    follow = valid & (ref.action_id == _capi.ACT_FOLLOW)
    return {"paths": int(valid.sum()), "follow": int(follow.sum()), "reduced": int((valid & (ref.reduced != 0)).sum()),
            "too_close": int((vref.too_close[follow] != 0).sum()), "vel_bound0": int((vref.vel_bound[valid] == 0).sum()),
            "vplan0": int((np.asarray(v.vel_plan) == 0.0).sum())}


def worth_comparing(act, n, gen):
    assert act["paths"] >= n and act["vplan0"] >= 1, act
    if n >= 96:
        assert 4 * act["follow"] >= n, act                               # a valid follow slot per four scenarios or more
        assert 0 < act["too_close"] < act["follow"], act                 # both values of too_close
        assert 0 < act["vel_bound0"] < act["paths"], act                 # both values of vel_bound
        if gen == "random":
            assert act["reduced"] >= 1, act                              # a reduced-horizon slot


def worst_errors(res, vres, vref):
    """Largest element-wise relative error of vx (where |vx| >= 1 m/s) and ax (where |ax| >= 0.5 m/s^2) over the valid slots: the
    quantities compare_tick bounds by 1e-5. Reported, not asserted."""
    evx = eax = 0.0
    for s, a in zip(*np.nonzero(res.valid == 1)):
        n = int(res.n_pts[s, a])
        for got, ref, floor, which in ((vres.vx, vref.vx, ELEM_FLOOR_VX, 0), (vres.ax, vref.ax, ELEM_FLOOR_AX, 1)):
            g, r = got[s, a, :n], ref[s, a, :n]
            m = np.abs(r) >= floor
            if m.any():
                e = float(np.max(np.abs(g[m] - r[m]) / np.abs(r[m])))
                evx, eax = (max(evx, e), eax) if which == 0 else (evx, max(eax, e))
    return evx, eax


def run_case(hip, cases, name, route, gen, n):
    scen, vels, vel, ref = cases.get(name, gen)
    batch, v = sub_batch(scen, vels, vel, 0, n)
    r, vr = ref(n)
    act = activity(r, vr, v)
    worth_comparing(act, n, gen)
    res, vres = hip.tick_batch(batch, v)
    evx, eax = worst_errors(res, vres, vr) if np.array_equal(res.valid, r.valid) and np.array_equal(res.n_pts, r.n_pts) else (-1.0, -1.0)
    print("variants: %-12s %-22s %-6s n %3d  paths %3d follow %3d reduced %d too_close %3d vel_bound0 %3d  vx %.1e ax %.1e"
          % (name, route, gen, n, act["paths"], act["follow"], act["reduced"], act["too_close"], act["vel_bound0"], evx, eax))
    compare_tick(res, vres, r, vr)


# ---------------------------------------------------------------- the launched routes on Monteblanco

@pytest.mark.parametrize("name", NAMES)
def test_fused_tick_with_the_compile_time_plan(hip_backend, cases, name):
    """Below the suite's pipeline threshold (64 scenarios): k_tick<EM, AXM1, PlanA4>, one workgroup per scenario."""
    for gen, n in (("random", 1), ("random", 5), ("random", 48), ("c2", 48)):
        run_case(hip_backend, cases, name, "k_tick PlanA4", gen, n)


@pytest.mark.parametrize("name", NAMES)
def test_pipeline_with_generic_jobs_finished_by_the_final_kernel(hip_backend, cases, name):
    """96 scenarios: k_follow_prep + k_vel_lanes + k_vel_final (fewer than LTPL_EMIT_MIN_SCEN = 256)."""
    for gen in ("random", "c2"):
        run_case(hip_backend, cases, name, "pipeline k_vel_final", gen, 96)


@pytest.mark.parametrize("name", NAMES)
def test_pipeline_with_every_job_finished_by_the_lane_kernel(hip_backend, cases, name):
    """600 scenarios on the suite's handle (LTPL_FOLLOW_EMIT_MIN_SCEN = 256): generic and follow jobs written by k_vel_lanes."""
    for gen in ("c2", "random"):
        run_case(hip_backend, cases, name, "pipeline lanes emit", gen, N_BIG)


@pytest.fixture(scope="module")
def two_wave_backend(monteblanco):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("LTPL_FOLLOW_EMIT_MIN_SCEN", "1000000")
        hip = _capi.HipBackend(monteblanco)
    yield hip
    hip.close()


@pytest.mark.parametrize("name", NAMES)
def test_pipeline_with_two_wave_follow_jobs(two_wave_backend, cases, name):
    """The same 600 scenarios on a handle that never lets the lane kernel finish a follow job: two waves + k_vel_final."""
    for gen in ("c2", "random"):
        run_case(two_wave_backend, cases, name, "pipeline two-wave", gen, N_BIG)


@pytest.fixture(scope="module")
def product_backend(monteblanco):
    hip = default_backend(monteblanco)
    yield hip
    hip.close()


@pytest.mark.parametrize("name", NAMES)
def test_fused_tick_as_a_grid_on_the_product_thresholds(product_backend, cases, name):
    """300 scenarios on a handle without the suite's pins: the fused kernel as a grid of 300 workgroups."""
    for gen in ("c2", "random"):
        run_case(product_backend, cases, name, "k_tick grid (default)", gen, 300)


# ---------------------------------------------------------------- the runtime plan class

@pytest.fixture(scope="module")
def berlin():
    """A lattice without a compile-time plan for the four-wave kernel: ltpl_tick_batch takes k_tick<.., PlanRt>."""
    from oracle.oracle_lib import OracleBackend
    from test_other_tracks import lattice_of
    lat = lattice_of("berlin")
    hip = _capi.HipBackend(lat)
    yield Cases(lat, OracleBackend(lat), n_big=48), hip
    hip.close()


@pytest.mark.parametrize("name", NAMES)
def test_fused_tick_with_the_runtime_plan(berlin, name):
    cases, hip = berlin
    run_case(hip, cases, name, "k_tick PlanRt (berlin)", "random", 5)


# ---------------------------------------------------------------- the resident kernel

N_VEH_CYCLE = (8, 0, 3)


def alternating_ticks(lat, pair, n_ticks, seed):
    """Single ticks in blocks of two per parameter set (A A B B A A ...) whose vehicle count changes with every tick (8, 0, 3, ...): a
    change of set replaces the resident kernel, the second tick of a block is served by the SAME resident kernel with every input offset
    behind the vehicle arrays moved."""
    ticks = []
    for i in range(n_ticks):
        name, n_veh = pair[(i // 2) % 2], N_VEH_CYCLE[i % 3]
        scen, vels = random_scenarios(lat, 1, seed=seed * 1000 + i, n_veh=n_veh, zone_prob=float(i % 2 == 0), last_prob=0.5)
        vel = vel_batch(lat, name, scen, vels, seed * 1000 + i)
        if i % 5 != 0:
            vel.vel_plan[0] = vel.vel_est[0] = 3.0 + 2.0 * i                     # (vel_batch starts scenario 0 at vel_plan = 0)
        ticks.append((name, n_veh, _capi.PathsBatch(scen, w_last_edges=W_LAST), vel))
    return ticks


@pytest.mark.parametrize("pair", [("exp1_table", "exp2_row"), ("exp2_table", "exp1p5_row"), ("exp1p5_table", "exp1_row")],
                         ids=lambda p: "+".join(p))
def test_resident_kernel_alternating_between_sets_and_vehicle_counts_matches_oracle(monteblanco, oracle_backend, monkeypatch, pair):
    """k_tick_persistent: two pairs of non-default sets, and the sixth variant next to the control set so that every instantiation of the
    resident kernel is compared with the oracle (not only with the launched k_tick of the same variant)."""
    n_ticks = 12
    monkeypatch.setenv("LTPL_PERSIST_IDLE_MS", "1000")      # (a stall of the host between the two ticks of a block would cost a launch)
    ticks = alternating_ticks(monteblanco, pair, n_ticks, seed=17)
    assert {t[1] for t in ticks} == {0, 3, 8} and {t[0] for t in ticks} == set(pair)
    assert all(ticks[i][0] == ticks[i + 1][0] and ticks[i][1] != ticks[i + 1][1] for i in range(0, n_ticks, 2))
    refs = [oracle_backend.tick_batch(b, v) for _, _, b, v in ticks]
    n_follow = sum(int(((r.action_id == _capi.ACT_FOLLOW) & (r.valid == 1)).sum()) for r, _ in refs)
    assert n_follow >= 3 and sum(int(v.vel_plan[0] == 0.0) for _, _, _, v in ticks) >= 2, n_follow
    pers = default_backend(monteblanco, persistent_tick=True)
    try:
        assert pers.persistent_stats()["enabled"] == 1
        for i, (name, n_veh, b, v) in enumerate(ticks):
            res, vres = pers.tick_batch(b, v)
            evx, eax = worst_errors(res, vres, refs[i][1]) if np.array_equal(res.valid, refs[i][0].valid) else (-1.0, -1.0)
            print("variants: %-12s %-22s tick %2d vehicles %d  vx %.1e ax %.1e" % (name, "k_tick_persistent", i, n_veh, evx, eax))
            compare_tick(res, vres, *refs[i])
        st = pers.persistent_stats()
        assert st["ticks"] == n_ticks and st["launches"] == n_ticks // 2, st          # one resident kernel per block of two ticks
    finally:
        pers.close()
        device_synchronize()


# ---------------------------------------------------------------- the sets do what they are named for

def test_every_set_moves_the_profiles_and_both_flag_values_occur(cases):
    """On the oracle alone: a set's vx differs from the control set's by more than 1e-3 relative on most valid slots of the same batch
    (otherwise it does not exercise what it is named for), and every 600-scenario batch holds both values of both flags."""
    for gen in ("random", "c2"):
        base = cases.get(CONTROL, gen)[3](N_BIG)
        for name in NAMES:
            _, _, vel, ref = cases.get(name, gen)
            r, vr = ref(N_BIG)
            worth_comparing(activity(r, vr, vel), N_BIG, gen)
            if name == CONTROL:
                continue
            both = np.nonzero((r.valid == 1) & (base[0].valid == 1) & (r.n_pts == base[0].n_pts))
            moved = 0
            for s, a in zip(*both):
                n = int(r.n_pts[s, a])
                x, b = vr.vx[s, a, :n], base[1].vx[s, a, :n]
                moved += int(np.max(np.abs(x - b) / np.maximum(np.abs(b), 1.0)) > 1e-3)
            assert len(both[0]) >= N_BIG and 2 * moved > len(both[0]), (name, gen, moved, len(both[0]))
