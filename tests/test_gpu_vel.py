"""GPU: seam (2) (velocity kernels) and the fused tick through the C ABI against recordings and the oracle."""
import numpy as np
import pytest

from helpers import load_golden, assert_close_rel, assert_vx_elementwise, assert_ax_elementwise
from scenarios import random_scenarios, raceline_state
from test_oracle_vel_golden import (make_vp, replay_vel_call, check_vel_output, replay_velparams_fixture, assert_velparams_coverage,
                                    VELPARAMS_FIXTURE)
from vel_jobs import (random_jobs, VARIANT_SETS, VARIANT_IDS, CHUNK_EDGE_LENGTHS, params_of, chunk_edge_jobs, edge_jobs,   # noqa: F401
                      brake_job_stopping_at, table_64_rows)
from graphbasedlocaltrajectoryplanner_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fixture", ["c2_vel_calls.npz", "c1_vel_calls.npz", "zonewall_vel_calls.npz"])
def test_hip_matches_reference_vel_recordings(monteblanco, hip_backend, fixture):
    recs = load_golden(fixture)
    seen = set()
    for i, rec in enumerate(recs):
        vp = make_vp(hip_backend, monteblanco, rec['state'])
        out = replay_vel_call(vp, rec)
        check_vel_output(out, rec, "%s call %d (%s)" % (fixture, i, rec['method']))
        seen.add(rec['method'])
    assert {'calc_vel_profile', 'calc_vel_profile_follow'} <= seen or fixture != "c2_vel_calls.npz"


@pytest.mark.parametrize("exp,axm,ctrl,varying_gg", [
    (1.0, [[100.0, 5.0]], "PD", False),
    (1.0, [[0.0, 6.0], [36.0, 6.0], [48.0, 4.8], [60.0, 3.9], [72.0, 2.5]], "PD", True),
    (2.0, [[100.0, 5.0]], "PDtan", False),
    (1.5, [[0.0, 6.0], [72.0, 2.5]], "PD", True),
    (2.0, [[0.0, 6.0], [36.0, 6.0], [72.0, 2.5]], "PD", True),             # with these two: all six kernel variants
    (1.5, [[100.0, 4.0]], "PDtan", False),
])
def test_hip_vel_matches_oracle_on_random_jobs(monteblanco, hip_backend, oracle_backend, exp, axm, ctrl, varying_gg):
    rng = np.random.default_rng(int(exp * 10) + len(axm))
    params = _capi.VelParamSet(dyn_model_exp=exp, drag_coeff=0.85, m_veh=1000.0, len_veh=monteblanco.veh_length,
                               v_max=float(rng.uniform(40, 100)), ax_max_machines=axm, follow_control_type=ctrl,
                               follow_control_params={"c_p": 1.15, "k_d": 0.025, "k_p": 0.2, "tan_w": 15.0})
    jobs = random_jobs(monteblanco, rng, 300, varying_gg)
    got = hip_backend.vel_profile(params, jobs)
    exp_ = oracle_backend.vel_profile(params, jobs)
    n_flag_mismatch = 0
    for i, ((vx, tc, vb), (rx, rtc, rvb)) in enumerate(zip(got, exp_)):
        assert_close_rel(vx, rx, what="job %d mode %d n %d" % (i, jobs[i]["mode"], jobs[i]["kappa"].size))
        assert_vx_elementwise(vx, rx, "job %d mode %d" % (i, jobs[i]["mode"]))
        assert tc == rtc
        n_flag_mismatch += int(vb != rvb)
    assert n_flag_mismatch == 0


def compare_jobs(jobs, got, exp_):
    """The assertions of the random-job test, job by job, a failure naming the job."""
    assert len(got) == len(exp_) == len(jobs)
    for jb, (vx, tc, vb), (rx, rtc, rvb) in zip(jobs, got, exp_):
        what = "job '%s' mode %d n %d" % (jb["name"], jb["mode"], jb["kappa"].size)
        assert_close_rel(vx, rx, what=what)
        assert_vx_elementwise(vx, rx, what)
        assert tc == rtc, what + " too_close"
        assert vb == rvb, what + " vel_bound"


_largest_n = {}


def largest_accepted_n(hip, lat):
    """The longest job ltpl_vel_profile accepts on this handle (its solver keeps a job in LDS; longer ones are refused with
    LTPL_ERR_CAPACITY before anything is launched), found by bisection."""
    if "n" not in _largest_n:
        params = params_of(lat, 1.0, [[100.0, 5.0]], "PD", 60.0)

        def accepted(n):
            job = {"name": "probe", "mode": _capi.VEL_FOLLOW, "kappa": np.zeros(n), "el_lengths": np.full(n, 2.0), "loc_gg": np.full((n, 2), 5.0),
                   "v_start": 10.0, "v_ego": 10.0, "v_obj": 5.0, "safety_d": 20.0, "obj_dist": 50.0, "obj_pos": tuple(lat.glob_rl[0, 1:3])}
            try:
                hip.vel_profile(params, [job])
            except _capi.BackendError as exc:
                assert "capacity exceeded" in str(exc), exc
                return False
            return True
        lo, hi = 512, 65536
        assert accepted(lo) and not accepted(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if accepted(mid) else (lo, mid)
        _largest_n["n"] = lo
    return _largest_n["n"]


@pytest.mark.parametrize("k", range(6), ids=VARIANT_IDS)
def test_hip_vel_matches_oracle_at_the_edges_of_the_sweeps_passes(monteblanco, hip_backend, oracle_backend, k):
    """fb_sweep, brake_profile and the cumulative sums run 64 steps per pass, unrolled by four, with steps that must change nothing beyond
    the job's end: every mode at n - 1 = 1, 2, 3, 4, 62 .. 65, 126 .. 129, 192 and at the longest job the entry point accepts, mixed in one
    call so that neighbouring jobs differ in length and mode."""
    exp, axm, ctrl, varying_gg = VARIANT_SETS[k]
    n_max = largest_accepted_n(hip_backend, monteblanco)
    assert n_max > 1024
    print("largest job ltpl_vel_profile accepts: %d points" % n_max)
    params = params_of(monteblanco, exp, axm, ctrl, 60.0 + 6.0 * k)
    jobs = chunk_edge_jobs(monteblanco, 400 + k, varying_gg, CHUNK_EDGE_LENGTHS + (n_max,))
    assert len(jobs) == 4 * (len(CHUNK_EDGE_LENGTHS) + 1)
    assert all(a["kappa"].size != b["kappa"].size or a["mode"] != b["mode"] for a, b in zip(jobs, jobs[1:]))
    compare_jobs(jobs, hip_backend.vel_profile(params, jobs), oracle_backend.vel_profile(params, jobs))


@pytest.mark.parametrize("v_max", (95.0, 42.0))
@pytest.mark.parametrize("k", range(6), ids=VARIANT_IDS)
def test_hip_vel_matches_oracle_on_named_edge_inputs(monteblanco, hip_backend, oracle_backend, k, v_max):
    """vel_jobs.edge_jobs, and brake jobs that reach standstill at the last point of a pass, the first of the next and next to them.
    v_max = 42 m/s puts the solver's "> v_max" break within reach of the straights; at 95 m/s speeds above the machine tables' last row
    occur."""
    exp, axm, ctrl, varying_gg = VARIANT_SETS[k]
    params = params_of(monteblanco, exp, axm, ctrl, v_max)
    jobs = edge_jobs(monteblanco, 500 + k, varying_gg, v_max)
    for stop in (63, 64, 65, 128, 129):
        jobs.append(brake_job_stopping_at(monteblanco, oracle_backend, params, 600 + 10 * k + stop, varying_gg, stop))
    exp_ = oracle_backend.vel_profile(params, jobs)
    by_name = {jb["name"]: out for jb, out in zip(jobs, exp_)}
    # (on the oracle's result: the jobs do what their names say)
    assert float(by_name["brake that never stops"][0].min()) > 1.0
    assert float(by_name["brake that stops inside the first pass"][0][40]) == 0.0
    for stop in (63, 64, 65, 128, 129):
        vx = by_name["brake that stops at point %d" % stop][0]
        assert vx[stop] == 0.0 and vx[stop - 1] > 0.0
    assert by_name["follow, obj_dist negative"][1] and by_name["follow, obj_dist zero"][1]
    if v_max < 50.0:
        vx = by_name["straight that reaches v_max early, then a corner and a second straight"][0]
        assert vx[:40].max() == v_max and vx.min() < 0.5 * v_max and vx[-1] > vx.min() + 5.0
    compare_jobs(jobs, hip_backend.vel_profile(params, jobs), exp_)


@pytest.mark.parametrize("exp", (1.0, 2.0, 1.5))
def test_hip_vel_machine_table_of_64_rows_and_refusal_of_65(monteblanco, hip_backend, oracle_backend, exp):
    """64 rows is the most make_vel_params admits; the table starts at 10 m/s and ends at 73 m/s, so speeds below its first and above its
    last row occur. 65 rows are refused with LTPL_ERR_CAPACITY."""
    table = table_64_rows()
    assert table.shape == (64, 2)
    params = params_of(monteblanco, exp, table, "PD", 95.0)
    rng = np.random.default_rng(64)
    jobs = edge_jobs(monteblanco, 700, True, 95.0)
    for i, jb in enumerate(random_jobs(monteblanco, rng, 60, True)):
        jb["name"] = "random job %d" % i
        jobs.append(jb)
    exp_ = oracle_backend.vel_profile(params, jobs)
    vmin, vmax = min(float(o[0].min()) for o in exp_), max(float(o[0].max()) for o in exp_)
    assert vmin < table[0, 0] and vmax > table[-1, 0]
    compare_jobs(jobs, hip_backend.vel_profile(params, jobs), exp_)
    v = 10.0 + np.arange(65.0)
    too_long = params_of(monteblanco, exp, np.column_stack((v, 6.5 - 0.06 * (v - 10.0))), "PD", 95.0)
    with pytest.raises(_capi.BackendError, match="capacity exceeded"):
        hip_backend.vel_profile(too_long, jobs[:1])


def test_hip_matches_reference_at_every_variants_parameters(monteblanco, hip_backend):
    """The unmodified reference's VpForwardBackward at the six variants' parameter sets (oracle/gen_golden_velparams.py), replayed on the
    kernels -- the recordings above run at exponent 1, the stock tables and the PD controller only."""
    recs = load_golden(VELPARAMS_FIXTURE)
    assert_velparams_coverage(recs, replay_velparams_fixture(hip_backend, monteblanco, recs))


def make_tick_inputs(lat, n, seed, n_veh=8):
    scen, vels = random_scenarios(lat, n, seed=seed, n_veh=n_veh)
    rng = np.random.default_rng(seed + 1000)
    params = _capi.VelParamSet(len_veh=lat.veh_length)
    vplan = rng.uniform(0.0, 60.0, n)
    vplan[::17] = 0.0
    pos = np.array([lat.node_pos[lat.layer_off[s['start_node'][0]] + s['start_node'][1]] for s in scen])
    pos = pos + rng.uniform(-0.3, 0.3, pos.shape)
    batch = _capi.PathsBatch(scen, w_last_edges=[0.0, 0.5, 0.8])
    vel = _capi.TickVelBatch(params, n, vplan, vplan + rng.uniform(-1, 1, n), pos,
                             np.concatenate(vels) if n_veh else np.zeros(0))
    return batch, vel


def compare_tick(res, vres, ref, vref):
    from test_gpu_paths import compare_results
    compare_results(res, ref, None)
    assert np.array_equal(vres.too_close, vref.too_close)
    assert np.array_equal(vres.vel_bound, vref.vel_bound)
    for s in range(res.n_scen):
        for a in range(int(res.n_actions[s])):
            if res.valid[s, a]:
                n = int(res.n_pts[s, a])
                assert_close_rel(vres.vx[s, a, :n], vref.vx[s, a, :n], what="vx s%d a%d" % (s, a))
                # ax = d(v^2) / (2 ds): compare against the scale of v^2 / ds
                scale = max(float(np.max(np.abs(vref.vx[s, a, :n]))) ** 2 / 2.0, 5.0)
                err = float(np.max(np.abs(vres.ax[s, a, :n] - vref.ax[s, a, :n])))
                assert err <= 1e-5 * scale, "ax s%d a%d err %.3e" % (s, a, err)
                # ... and sample by sample (north_star: velocity profiles within 1e-5 relative; every operand of the stage is fp64)
                assert_vx_elementwise(vres.vx[s, a, :n], vref.vx[s, a, :n], "s%d a%d" % (s, a))
                assert_ax_elementwise(vres.ax[s, a, :n], vref.ax[s, a, :n], "s%d a%d" % (s, a))


@pytest.mark.parametrize("seed,n_veh", [(0, 8), (7, 3), (9, 0)])
def test_fused_tick_matches_oracle(monteblanco, hip_backend, oracle_backend, seed, n_veh):
    batch, vel = make_tick_inputs(monteblanco, 256, seed, n_veh)
    res, vres = hip_backend.tick_batch(batch, vel)
    ref, vref = oracle_backend.tick_batch(batch, vel)
    compare_tick(res, vres, ref, vref)
    if n_veh >= 3:
        assert int(vres.too_close.sum()) > 0 or int((res.action_id == _capi.ACT_FOLLOW).sum()) > 0


def test_resident_batch_equals_tick_batch(monteblanco, hip_backend):
    batch, vel = make_tick_inputs(monteblanco, 512, 3, 8)
    res, vres = hip_backend.tick_batch(batch, vel)
    hip_backend.batch_upload(batch, vel)
    ms = hip_backend.batch_run(reps=3, timed=True)
    assert ms > 0.0
    res2, vres2 = hip_backend.batch_download()
    for name in ("valid", "action_id", "n_pts", "n_nodes", "reduced"):
        assert np.array_equal(getattr(res, name), getattr(res2, name)), name
    assert np.array_equal(vres.vel_bound, vres2.vel_bound)
    # (entries of the capacity slabs behind n_nodes / n_pts are unspecified -- include/ltpl_hip.h -- and the resident pipeline rotates through
    # three buffer sets: compare what is defined, bit for bit)
    for s, a in zip(*np.nonzero(res.valid)):
        nn, npt = int(res.n_nodes[s, a]), int(res.n_pts[s, a])
        assert np.array_equal(res.nodes[s, a, :nn], res2.nodes[s, a, :nn]) and np.array_equal(res.node_idx[s, a, :nn], res2.node_idx[s, a, :nn])
        assert np.array_equal(res.coeff[s, a, :nn - 1], res2.coeff[s, a, :nn - 1]) and np.array_equal(res.path_param[s, a, :npt], res2.path_param[s, a, :npt])
        assert np.array_equal(vres.vx[s, a, :npt], vres2.vx[s, a, :npt]) and np.array_equal(vres.ax[s, a, :npt], vres2.ax[s, a, :npt])
    # ... and after a run that ends on every one of the buffer sets
    for reps in (1, 2, 3, 5):
        hip_backend.batch_run(reps=reps, timed=False)
        res3, vres3 = hip_backend.batch_download()
        assert np.array_equal(res.valid, res3.valid) and np.array_equal(res.n_pts, res3.n_pts)
        for s, a in zip(*np.nonzero(res.valid)):
            npt = int(res.n_pts[s, a])
            assert np.array_equal(vres.vx[s, a, :npt], vres3.vx[s, a, :npt]) and np.array_equal(res.path_param[s, a, :npt], res3.path_param[s, a, :npt]), reps


def test_tick_paths_equal_plan_paths(monteblanco, hip_backend):
    """The fused kernel's path stage is the seam-(1) kernel body: identical bits."""
    batch, vel = make_tick_inputs(monteblanco, 256, 5, 8)
    res, _ = hip_backend.tick_batch(batch, vel)
    res1 = hip_backend.plan_paths(batch)
    for name in ("nodes", "node_idx", "coeff", "path_param", "valid", "action_id", "n_pts", "reduced", "n_ties"):
        assert np.array_equal(getattr(res, name), getattr(res1, name)), name


def compact_inputs(lat, n):
    from scenarios import random_scenarios
    scen, vels = random_scenarios(lat, n, seed=31 + n)
    batch = _capi.PathsBatch(scen, w_last_edges=[0.0, 0.5, 0.8])
    params = _capi.VelParamSet(len_veh=lat.veh_length)
    pos = np.array([lat.node_pos[lat.layer_off[s['start_node'][0]] + s['start_node'][1]] for s in scen])
    return batch, _capi.TickVelBatch(params, n, np.full(n, 25.0), np.full(n, 25.0), pos, np.concatenate(vels))


def check_compact_against_slabs(lat, hip_backend, n, max_rows=115, s_bound=None):
    """One batch of ``n`` scenarios through ltpl_tick_batch and ltpl_tick_batch_compact. ``s_bound``: the s column also against a long-double
    running sum, relative to its last value. Returns (slab results, compact result)."""
    batch, vel = compact_inputs(lat, n)
    res, vres = hip_backend.tick_batch(batch, vel)
    comp = hip_backend.new_compact_trajectories(n, max_rows=max_rows)
    hip_backend.tick_batch_compact(batch, vel, comp)
    cut = max_rows if max_rows > 0 else hip_backend.caps.max_path_pts
    assert comp.struct.total_rows == int(np.minimum(res.n_pts * res.valid, cut).sum())
    for s in range(n):
        tr = comp.trajectories(s)
        names = [_capi.ACTION_NAMES[int(res.action_id[s, a])] for a in range(int(res.n_actions[s])) if res.valid[s, a]]
        assert list(tr.keys()) == names
        for a in range(int(res.n_actions[s])):
            if not res.valid[s, a]:
                continue
            m = min(int(res.n_pts[s, a]), cut)
            t = tr[_capi.ACTION_NAMES[int(res.action_id[s, a])]][0]
            assert t.shape == (m, 7)
            assert np.array_equal(t[:, 1:5], res.path_param[s, a, :m, 0:4])
            assert np.array_equal(t[:, 5], vres.vx[s, a, :m]) and np.array_equal(t[:, 6], vres.ax[s, a, :m])
            s_ref = np.concatenate(([0.0], np.cumsum(res.path_param[s, a, :m - 1, 4])))
            assert_close_rel(t[:, 0], s_ref, what="s column")
            if s_bound is not None:
                s_ld = np.concatenate(([np.longdouble(0)], np.cumsum(res.path_param[s, a, :m - 1, 4].astype(np.longdouble))))
                err = float(np.max(np.abs(t[:, 0].astype(np.longdouble) - s_ld)))
                assert err <= s_bound * float(s_ld[-1]), "s column of scenario %d slot %d: %.3e > %.1e * %.3f" % (s, a, err, s_bound, float(s_ld[-1]))
            assert comp.vel_bound[s * 3 + a] == vres.vel_bound[s, a] and comp.reduced[s * 3 + a] == res.reduced[s, a]
    return res, vres, comp


def test_compact_trajectories_equal_the_slab_outputs(monteblanco, hip_backend):
    """ltpl_tick_batch_compact packs exactly the rows ltpl_tick_batch returns (trimmed to max_rows), for a batch on the
    one-wave pipeline and for a small batch on the fused kernel; s is the running sum of the element lengths (OTH.py:743)."""
    for n in (96, 5):
        check_compact_against_slabs(monteblanco, hip_backend, n)


@pytest.mark.parametrize("max_rows", (115, 0))
@pytest.mark.parametrize("n", (341, 342, 700))
def test_compact_trajectories_with_several_slots_per_thread_of_the_offset_scan(monteblanco, hip_backend, n, max_rows):
    """k_compact_offsets is ONE block of 1024 threads, each of which owns ceil(slots / 1024) consecutive slots: 341, 342 and 700 scenarios
    are 1023, 1026 and 2100 slots -- one, two and three slots per thread, with trailing threads that own fewer or none (the 96- and
    5-scenario batches above give every thread at most one). With trimming to 115 rows and without (max_rows = 0). The s column is held
    against a long-double running sum at 1e-13 of its last value: at most ~150 additions, each half an ulp of the running sum, give
    <= 150 * 1.1e-16 = 2e-14."""
    res, _, comp = check_compact_against_slabs(monteblanco, hip_backend, n, max_rows=max_rows, s_bound=1e-13)
    assert 3 * n == {341: 1023, 342: 1026, 700: 2100}[n]
    rows = res.n_pts * res.valid
    assert int(rows.max()) > 115 and int((rows == 0).sum()) > 0          # trimming bites; empty slots lie between the kept ones
    assert int(comp.n_rows.max()) == (115 if max_rows else int(rows.max()))
    kept = comp.n_rows > 0
    assert np.array_equal(comp.row_off[kept], (np.cumsum(comp.n_rows) - comp.n_rows)[kept])      # back to back, in slot order


def test_compact_capacity_one_row_short_is_refused_and_the_backend_stays_usable(monteblanco, hip_backend):
    n = 342
    batch, vel = compact_inputs(monteblanco, n)
    full = hip_backend.new_compact_trajectories(n, max_rows=115)
    hip_backend.tick_batch_compact(batch, vel, full)
    need = int(full.struct.total_rows)
    assert need > 115
    short = hip_backend.new_compact_trajectories(n, max_rows=115, capacity_rows=need - 1)
    with pytest.raises(_capi.BackendError, match="capacity_rows"):
        hip_backend.tick_batch_compact(batch, vel, short)
    assert int(short.struct.total_rows) == need                           # the need, for the caller's next attempt
    again = hip_backend.new_compact_trajectories(n, max_rows=115, capacity_rows=need)
    hip_backend.tick_batch_compact(batch, vel, again)                     # exactly enough; the backend serves the next call
    assert int(again.struct.total_rows) == need
    assert np.array_equal(again.n_rows, full.n_rows) and np.array_equal(again.row_off, full.row_off)
    assert np.array_equal(again.rows[:need], full.rows[:need])


def test_follow_jobs_finished_by_the_lane_kernel_or_by_the_final_kernel(monteblanco, hip_backend, monkeypatch):
    """Round 6: in large batches the lane kernel finishes a follow job itself (controlled part and unconstrained profile in one lane, capped
    backward sweep); in smaller ones the two halves run on two waves and k_vel_final composes. Same operations on the same values: every
    output of a 600-scenario batch with an opponent ahead in every scenario is IDENTICAL bit for bit between a handle that takes the first
    route (the suite's setting) and one that takes the second."""
    from graphbasedlocaltrajectoryplanner_amd.scenario_gen import c2_scenarios
    n = 600
    scen, vels = c2_scenarios(monteblanco, n, seed=77, lead_gap=(20.0, 80.0))
    rng = np.random.default_rng(5)
    params = _capi.VelParamSet(len_veh=monteblanco.veh_length)
    vplan = rng.uniform(5.0, 60.0, n)
    pos = np.array([monteblanco.node_pos[monteblanco.layer_off[s['start_node'][0]] + s['start_node'][1]] for s in scen])
    batch = _capi.PathsBatch(scen, w_last_edges=[0.0, 0.5, 0.8])
    vel = _capi.TickVelBatch(params, n, vplan, vplan, pos, np.concatenate(vels))
    monkeypatch.setenv("LTPL_FOLLOW_EMIT_MIN_SCEN", "1000000")
    other = _capi.HipBackend(monteblanco)
    (ra, va), (rb, vb) = hip_backend.tick_batch(batch, vel), other.tick_batch(batch, vel)
    assert np.array_equal(ra.n_actions, rb.n_actions) and np.array_equal(va.vel_bound, vb.vel_bound) and np.array_equal(va.too_close, vb.too_close)
    n_follow = 0
    for s in range(n):
        for k in range(int(ra.n_actions[s])):
            if ra.valid[s, k]:
                m = int(ra.n_pts[s, k])
                n_follow += int(ra.action_id[s, k] == _capi.ACT_FOLLOW)
                assert np.array_equal(va.vx[s, k, :m], vb.vx[s, k, :m]) and np.array_equal(va.ax[s, k, :m], vb.ax[s, k, :m]), (s, k)
    assert n_follow >= n // 2, n_follow
    other.close()


def test_large_batches_are_planned_in_the_order_of_their_start_layers_with_identical_results(monteblanco, hip_backend, monkeypatch):
    """Round 6: batches of >= 2 048 scenarios are planned sorted by start layer (block b -> scenario order[b]); outputs are indexed by scenario,
    so every output must be IDENTICAL bit for bit to a handle that plans them in the caller's order (LTPL_NO_SCEN_ORDER=1) -- 2 500 scenarios
    with shuffled start layers, a zero-vehicle scenario and repeated start layers among them."""
    n = 2500
    batch, vel = make_tick_inputs(monteblanco, n, seed=41)
    monkeypatch.setenv("LTPL_NO_SCEN_ORDER", "1")
    other = _capi.HipBackend(monteblanco)
    (ra, va), (rb, vb) = hip_backend.tick_batch(batch, vel), other.tick_batch(batch, vel)
    for name in ("n_actions", "end_layer", "closest_obj_index", "closest_obj_node"):
        assert np.array_equal(getattr(ra, name), getattr(rb, name)), name
    assert np.array_equal(va.vel_bound, vb.vel_bound) and np.array_equal(va.too_close, vb.too_close)
    for s in range(n):
        na = int(ra.n_actions[s])
        for name in ("action_id", "valid", "reduced", "goal_layer", "n_nodes", "n_pts", "n_ties"):
            assert np.array_equal(getattr(ra, name)[s, :na], getattr(rb, name)[s, :na]), (s, name)
        for k in range(na):
            if ra.valid[s, k]:
                m, nn = int(ra.n_pts[s, k]), int(ra.n_nodes[s, k])
                assert np.array_equal(ra.nodes[s, k, :nn], rb.nodes[s, k, :nn]) and np.array_equal(ra.coeff[s, k, :nn - 1], rb.coeff[s, k, :nn - 1]), (s, k)
                assert np.array_equal(ra.path_param[s, k, :m], rb.path_param[s, k, :m]), (s, k)
                assert np.array_equal(va.vx[s, k, :m], vb.vx[s, k, :m]) and np.array_equal(va.ax[s, k, :m], vb.ax[s, k, :m]), (s, k)
    other.close()
