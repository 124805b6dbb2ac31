"""Seam-(2) jobs (the dicts _capi.make_vel_jobs packs) for the velocity tests: the six kernel variants' parameter sets, seeded random
jobs, job lengths around the edges of the sweeps' 64-step passes, and named edge inputs. Shared by tests/test_gpu_vel.py (kernel vs
oracle), oracle/gen_golden_velparams.py (the unmodified reference on the same jobs) and tests/test_oracle_vel_golden.py."""
import numpy as np

from graphbasedlocaltrajectoryplanner_amd import _capi
from graphbasedlocaltrajectoryplanner_amd.scenario_gen import raceline_state

CTRL_PARAMS = {"c_p": 1.15, "k_d": 0.025, "k_p": 0.2, "tan_w": 15.0}

# (dyn_model_exp, ax_max_machines, follow controller, location dependent loc_gg): one per kernel variant = (exponent 1 / 2 / general) x
# (one-row / interpolated machine table); PD and PDtan each on sets whose random jobs carry follow jobs (all do)
VARIANT_SETS = [
    (1.0, [[100.0, 5.0]], "PD", False),
    (1.0, [[0.0, 6.0], [36.0, 6.0], [48.0, 4.8], [60.0, 3.9], [72.0, 2.5]], "PD", True),
    (2.0, [[100.0, 5.0]], "PDtan", False),
    (2.0, [[0.0, 6.0], [36.0, 6.0], [72.0, 2.5]], "PD", True),
    (1.5, [[100.0, 4.0]], "PD", False),
    (1.5, [[0.0, 6.0], [72.0, 2.5]], "PDtan", True),
]
VARIANT_IDS = ["exp%g-%drows-%s" % (e, len(t), c) for e, t, c, _ in VARIANT_SETS]

# job lengths n for which n - 1 (the number of steps of a sweep) lies on either side of a multiple of the 64 steps of a pass, of the
# unroll by four inside a pass, and at the shortest profiles there are
CHUNK_EDGE_LENGTHS = (2, 3, 4, 5, 63, 64, 65, 66, 127, 128, 129, 130, 193)


def params_of(lat, exp, axm, ctrl, v_max):
    return _capi.VelParamSet(dyn_model_exp=exp, drag_coeff=0.85, m_veh=1000.0, len_veh=lat.veh_length, v_max=float(v_max),
                             ax_max_machines=axm, follow_control_type=ctrl, follow_control_params=dict(CTRL_PARAMS))


def random_jobs(lat, rng, n_jobs, varying_gg, n_max=400):
    jobs = []
    track_len = float(lat.glob_rl[-1, 0])
    for _ in range(n_jobs):
        n = int(rng.integers(2, n_max))
        mode = int(rng.integers(0, 3))
        # curvature profile: piecewise smooth with straights (exact zeros) and tight corners
        kappa = 0.08 * np.sin(np.linspace(0, rng.uniform(1, 12), n) + rng.uniform(0, 6)) * rng.uniform(0, 1)
        kappa[np.abs(kappa) < 0.004] = 0.0
        el = rng.uniform(1.5, 3.5, n - 1)
        if varying_gg:
            gg = np.column_stack((rng.uniform(3.0, 8.0, n), rng.uniform(3.0, 8.0, n)))
        else:
            gg = np.ones((n, 2)) * rng.uniform(3.0, 9.0, 2)
        job = {"mode": mode, "kappa": kappa, "loc_gg": gg, "v_start": float(rng.uniform(0, 70))}
        if mode == _capi.VEL_FB:
            job["el_lengths"] = el
            job["v_end"] = float(rng.uniform(0, 60)) if rng.random() < 0.8 else None
        elif mode == _capi.VEL_BRAKE:
            job["el_lengths"] = el
        else:
            job["el_lengths"] = np.append(el, 0.0)
            x, y, _, v = raceline_state(lat, rng.uniform(0, track_len))
            job.update(v_ego=job["v_start"] + rng.uniform(-1, 1), v_obj=float(v) * rng.uniform(0.1, 1.0),
                       safety_d=float(rng.uniform(5, 40)), obj_dist=float(rng.uniform(-5, 400)),
                       obj_pos=(float(x + rng.uniform(-2, 2)), float(y + rng.uniform(-2, 2))))
        jobs.append(job)
    return jobs


def corner_kappa(n, rng):
    """Straights (exact zeros) between corners of either sign, up to 0.07 1/m."""
    kappa = 0.07 * np.sin(np.linspace(0.0, 1.0 + n / 25.0, n) + rng.uniform(0, 6))
    kappa[np.abs(kappa) < 0.02] = 0.0
    return kappa


def follow_fields(lat, rng, v_start, **over):
    x, y, _, v = raceline_state(lat, rng.uniform(0, float(lat.glob_rl[-1, 0])))
    f = dict(v_ego=v_start + 0.4, v_obj=float(v) * 0.6, safety_d=25.0, obj_dist=float(rng.uniform(30, 250)),
             obj_pos=(float(x + 1.0), float(y - 1.0)))
    f.update(over)
    return f


def job_of(lat, rng, mode, n, varying_gg, name, kappa=None, el=2.5, gg=None, v_start=30.0, v_end=None, **follow):
    """One job of ``n`` points. mode: VEL_FB (v_end None = free end), VEL_BRAKE, VEL_FOLLOW."""
    kappa = corner_kappa(n, rng) if kappa is None else np.asarray(kappa, dtype=float)
    el = np.full(n - 1, float(el)) if np.isscalar(el) else np.asarray(el, dtype=float)
    if gg is None:
        gg = (np.column_stack((rng.uniform(3.0, 8.0, n), rng.uniform(3.0, 8.0, n))) if varying_gg
              else np.ones((n, 2)) * rng.uniform(3.5, 8.0, 2))
    job = {"name": name, "mode": mode, "kappa": kappa, "loc_gg": np.asarray(gg, dtype=float), "v_start": float(v_start)}
    if mode == _capi.VEL_FOLLOW:
        job["el_lengths"] = np.append(el, 0.0)
        job.update(follow_fields(lat, rng, float(v_start), **follow))
    else:
        job["el_lengths"] = el
        if mode == _capi.VEL_FB:
            job["v_end"] = v_end
    return job


def chunk_edge_jobs(lat, seed, varying_gg, lengths=CHUNK_EDGE_LENGTHS):
    """Every mode (forward-backward with and without v_end, brake, follow) at every length; the order interleaves the lengths so that
    neighbouring jobs of the call differ in length and mode."""
    rng = np.random.default_rng(seed)
    jobs = []
    for k, n in enumerate(lengths):
        for m, (mode, tag) in enumerate(((_capi.VEL_FB, "fb_v_end"), (_capi.VEL_FB, "fb_free"), (_capi.VEL_BRAKE, "brake"),
                                         (_capi.VEL_FOLLOW, "follow"))):
            v0 = float(rng.uniform(5.0, 45.0))
            jobs.append(job_of(lat, rng, mode, n, varying_gg, "%s n=%d" % (tag, n), v_start=v0,
                               v_end=float(rng.uniform(0.0, 30.0)) if tag == "fb_v_end" else None,
                               el=rng.uniform(1.5, 3.5, n - 1)))
    order = [(i * 5) % len(jobs) for i in range(len(jobs))]
    assert sorted(order) == list(range(len(jobs)))
    return [jobs[i] for i in order]


def table_64_rows():
    """64 rows, the most the library admits, from 10 m/s to 73 m/s: speeds below the first and above the last row occur."""
    v = 10.0 + np.arange(64.0)
    return np.column_stack((v, 6.5 - 0.06 * (v - 10.0)))


def edge_jobs(lat, seed, varying_gg, v_max, n=150):
    """Named edge inputs (every one a job of its own, so that a failure names it). ``v_max`` is the parameter set's."""
    rng = np.random.default_rng(seed)
    FB, BRAKE, FOLLOW = _capi.VEL_FB, _capi.VEL_BRAKE, _capi.VEL_FOLLOW
    alt = np.zeros(n)
    alt[0::4], alt[2::4] = 0.05, -0.05                                   # + 0 - 0 + 0 - 0 ...
    tight_first = corner_kappa(n, rng); tight_first[0] = 0.08
    tight_last = corner_kappa(n, rng); tight_last[-1] = 0.08
    # a straight on which v_max is reached early, a corner that forces the car down, and a second straight (a later acceleration run)
    vmax_break = np.zeros(n)
    vmax_break[n // 2:n // 2 + 12] = 0.06
    jobs = [
        job_of(lat, rng, FB, n, varying_gg, "kappa all zero", kappa=np.zeros(n), v_start=20.0),
        job_of(lat, rng, FB, n, varying_gg, "kappa all zero, v_end", kappa=np.zeros(n), v_start=20.0, v_end=12.0),
        job_of(lat, rng, FB, n, varying_gg, "kappa alternating sign with exact zeros", kappa=alt, v_start=15.0, v_end=10.0),
        job_of(lat, rng, FB, n, varying_gg, "v_start = 0", v_start=0.0),
        job_of(lat, rng, FB, n, varying_gg, "v_start = 0, v_end = 0", v_start=0.0, v_end=0.0),
        job_of(lat, rng, FB, n, varying_gg, "v_start above the first point's lateral limit and above v_max", kappa=tight_first,
               v_start=v_max + 20.0),
        job_of(lat, rng, FB, n, varying_gg, "v_end = 0", v_start=25.0, v_end=0.0),
        job_of(lat, rng, FB, n, varying_gg, "v_end above the last point's limit", kappa=tight_last, v_start=25.0, v_end=80.0),
        job_of(lat, rng, FB, n, varying_gg, "straight that reaches v_max early, then a corner and a second straight", kappa=vmax_break,
               el=3.5, v_start=max(v_max - 4.0, 1.0)),
        job_of(lat, rng, FB, n, varying_gg, "speeds above the last row of the machine table", kappa=np.zeros(n), el=3.5,
               v_start=min(90.0, v_max), v_end=None),
        job_of(lat, rng, FB, n, varying_gg, "speeds below the first row of the machine table", kappa=np.zeros(n), v_start=0.5, v_end=3.0),
        job_of(lat, rng, FB, n, True, "position-varying loc_gg with a backward sweep", v_start=35.0, v_end=2.0),
        job_of(lat, rng, FB, n, True, "position-varying loc_gg on a straight with a backward sweep", kappa=np.zeros(n), v_start=40.0, v_end=0.0),
        job_of(lat, rng, FOLLOW, n, varying_gg, "follow, obj_dist negative", v_start=20.0, obj_dist=-7.5),
        job_of(lat, rng, FOLLOW, n, varying_gg, "follow, obj_dist zero", v_start=20.0, obj_dist=0.0),
        job_of(lat, rng, FOLLOW, n, varying_gg, "follow, obj_dist beyond the path's end", v_start=20.0, obj_dist=2.5 * n + 600.0),
        job_of(lat, rng, FOLLOW, n, varying_gg, "follow, v_obj = 0", v_start=20.0, v_obj=0.0, obj_dist=120.0),
        job_of(lat, rng, FOLLOW, n, varying_gg, "follow, v_obj = 0 right ahead", v_start=30.0, v_obj=0.0, obj_dist=35.0),
        job_of(lat, rng, BRAKE, n, varying_gg, "brake that stops inside the first pass", kappa=np.zeros(n), v_start=9.0),
        job_of(lat, rng, BRAKE, n, varying_gg, "brake in corners that stops inside the first pass", v_start=12.0),
        job_of(lat, rng, BRAKE, 40, varying_gg, "brake that never stops", kappa=np.zeros(40), el=1.5, v_start=60.0),
        job_of(lat, rng, BRAKE, n, varying_gg, "brake from v_start = 0", v_start=0.0),
    ]
    return jobs


def brake_job_stopping_at(lat, oracle, params, seed, varying_gg, stop_index, n=200):
    """A brake job on a straight whose profile first reaches standstill exactly at point ``stop_index`` (by the oracle: v_start found by
    bisection between a start that stops earlier and one that stops later)."""
    rng = np.random.default_rng(seed)
    job = job_of(lat, rng, _capi.VEL_BRAKE, n, varying_gg, "brake that stops at point %d" % stop_index, kappa=np.zeros(n), v_start=1.0)

    def first_zero(v0):
        job["v_start"] = float(v0)
        vx = oracle.vel_profile(params, [job])[0][0]
        z = np.flatnonzero(vx == 0.0)
        return int(z[0]) if z.size else n
    lo, hi = 0.5, 150.0
    assert first_zero(lo) < stop_index < first_zero(hi), (first_zero(lo), first_zero(hi))
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        k = first_zero(mid)
        if k == stop_index:
            return job
        lo, hi = (mid, hi) if k < stop_index else (lo, mid)
    raise AssertionError("no start velocity stops at point %d" % stop_index)
