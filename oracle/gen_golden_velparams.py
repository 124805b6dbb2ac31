"""
ORACLE / TEST INFRASTRUCTURE ONLY. Seam-(2) recordings of the UNMODIFIED reference's VpForwardBackward at general parameters: the
closed-loop recordings (gen_golden.py) run at dyn_model_exp = 1 with the stock tables and the PD controller, so they pin the oracle --
and with it everything compared with the oracle -- to the reference on one of the six velocity-kernel variants only. Here the
reference's class is constructed for each of the six sets of tests/vel_jobs.py (exponent 1 / 2 / 1.5 x one-row / interpolated
machine table, PD / PDtan), one of them with update_dyn_parameters at gg scales other than 1, and called on seeded jobs: random ones,
every mode at the job lengths around the sweeps' pass edges, and the named edge inputs of tests/vel_jobs.py. A call in which the
reference raises (math.sqrt of a negative radicand) is counted and left out.

    python -m oracle.gen_golden_velparams          (container only: needs the reference tree)

  tests/golden/velparams_vel_calls.npz   records {method, params, state, args, out} in the layout tests/test_oracle_vel_golden.py's
                                         replay_vel_call / make_vp read (fixture_io.save_records, packed: arrays and one JSON tree)

Data only: arguments, parameter values and outputs. Running it twice gives the same values (every draw is seeded); the archive's bytes
are whatever numpy's zip writer makes of them.
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_env                                                     # noqa: E402
from oracle.fixture_io import save_records                                     # noqa: E402
from graphbasedlocaltrajectoryplanner_amd import _capi                         # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.lattice import Lattice               # noqa: E402
import vel_jobs                                                                # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "velparams_vel_calls.npz")
V_MAX = (95.0, 42.0, 80.0, 45.0, 100.0, 70.0)          # per set: with and without the solver's "> v_max" break in reach
GG_SCALES = {3: (0.9, 0.8)}                            # set 3: (scale of the earlier ticks = old_gg_scale, current scale)
N_EDGE, N_RANDOM = 72, 10


def jobs_of_set(lat, k):
    """The jobs of set ``k`` (job dicts of tests/vel_jobs.py; a job with 'vel_course' is a check_brake_prefix call)."""
    exp, axm, ctrl, varying_gg = vel_jobs.VARIANT_SETS[k]
    rng = np.random.default_rng(900 + k)
    jobs = vel_jobs.random_jobs(lat, rng, N_RANDOM, varying_gg, n_max=200)
    # every length, the four kinds of job rotating over the lengths (and over the sets: every kind meets every length in some set)
    edge = {j["name"]: j for j in vel_jobs.chunk_edge_jobs(lat, 910 + k, varying_gg)}
    kinds = ("fb_v_end", "fb_free", "brake", "follow")
    jobs += [edge["%s n=%d" % (kinds[(i + k) % 4], n)] for i, n in enumerate(vel_jobs.CHUNK_EDGE_LENGTHS)]
    jobs += vel_jobs.edge_jobs(lat, 920 + k, varying_gg, V_MAX[k], n=N_EDGE)
    for v_plan in (V_MAX[k] + 12.0, V_MAX[k] + 0.05):                   # a braking prefix, and none (within the 0.1 m/s margin)
        j = vel_jobs.job_of(lat, rng, _capi.VEL_BRAKE, 90, varying_gg, "check_brake_prefix from %.2f" % v_plan, v_start=v_plan)
        j["vel_course"] = np.full(3, v_plan)
        jobs.append(j)
    return jobs


def reference_vp(gl, lat, k):
    exp, axm, ctrl, _ = vel_jobs.VARIANT_SETS[k]
    vp = gl.online_graph.src.VpForwardBackward.VpForwardBackward(
        dyn_model_exp=exp, drag_coeff=0.85, m_veh=1000.0, len_veh=lat.veh_length, follow_control_type=ctrl,
        follow_control_params=dict(vel_jobs.CTRL_PARAMS), glob_rl=lat.glob_rl)
    old, cur = GG_SCALES.get(k, (1.0, 1.0))
    vp.update_dyn_parameters(vel_max=V_MAX[k], gg_scale=old, ax_max_machines=np.array(axm, dtype=float))
    vp.update_dyn_parameters(vel_max=V_MAX[k], gg_scale=cur, ax_max_machines=np.array(axm, dtype=float))
    return vp


def call_of(job):
    """(method name, keyword arguments) of the VpForwardBackward call a job stands for."""
    base = {"kappa": job["kappa"], "el_lengths": job["el_lengths"], "loc_gg": job["loc_gg"]}
    if "vel_course" in job:
        return "check_brake_prefix", dict(base, vel_plan=job["v_start"], vel_course=job["vel_course"])
    if job["mode"] == _capi.VEL_FB:
        return "calc_vel_profile", dict(base, v_start=job["v_start"], v_end=job["v_end"])
    if job["mode"] == _capi.VEL_BRAKE:
        return "calc_vel_brake_em", dict(base, v_start=job["v_start"])
    return "calc_vel_profile_follow", dict(base, v_start=job["v_start"], v_ego=job["v_ego"], v_obj=job["v_obj"],
                                           safety_d=job["safety_d"], obj_dist=job["obj_dist"], obj_pos=list(job["obj_pos"]))


def records_of_set(gl, lat, k, only=None):
    """Records of set ``k`` (``only``: indices of the set's jobs) and the names of the jobs in which the reference raised."""
    exp, axm, ctrl, _ = vel_jobs.VARIANT_SETS[k]
    P = '_VpForwardBackward__'
    recs, raised = [], []
    for i, job in enumerate(jobs_of_set(lat, k)):
        if only is not None and i not in only:
            continue
        vp = reference_vp(gl, lat, k)                       # (check_brake_prefix moves old_gg_scale: every call on a fresh object)
        method, kwargs = call_of(job)
        rec = {"method": method, "set": k, "job": i, "name": job.get("name", "random job %d" % i),
               "params": {"dyn_model_exp": float(exp), "follow_control_type": ctrl, "follow_control_params": dict(vel_jobs.CTRL_PARAMS)},
               "state": {"vel_max": float(getattr(vp, P + 'vel_max')), "gg_scale": float(getattr(vp, P + 'gg_scale')),
                         "old_gg_scale": float(getattr(vp, P + 'old_gg_scale')),
                         "ax_max_machines": np.array(getattr(vp, P + 'ax_max_machines'), dtype=float)},
               "args": {key: (np.array(v, dtype=float) if isinstance(v, (np.ndarray, list, tuple)) else (None if v is None else float(v)))
                        for key, v in kwargs.items()}}
        try:
            out = getattr(vp, method)(**{key: (np.array(v, dtype=float) if isinstance(v, np.ndarray) else v) for key, v in kwargs.items()})
        except ValueError as exc:
            raised.append("set %d job %d (%s): %s" % (k, i, rec["name"], exc))
            continue
        if isinstance(out, tuple):
            rec["out"] = [np.array(o, dtype=float) if isinstance(o, (np.ndarray, list)) else
                          (bool(o) if isinstance(o, (bool, np.bool_)) else o) for o in out]
        else:
            rec["out"] = np.array(out, dtype=float)
        recs.append(rec)
    return recs, raised


def main():
    gl, _ = ref_env.load_reference()
    lat = Lattice.load(os.path.join(ROOT, "tests", "golden", "monteblanco_lattice.npz"))
    recs, raised = [], []
    for k in range(len(vel_jobs.VARIANT_SETS)):
        r, x = records_of_set(gl, lat, k)
        recs += r
        raised += x
    save_records(FIXTURE, recs, packed=True)
    print("written %s: %d records, %d bytes; the reference raised in %d calls (left out)"
          % (os.path.relpath(FIXTURE, ROOT), len(recs), os.path.getsize(FIXTURE), len(raised)))
    for line in raised:
        print("  raised:", line)


if __name__ == "__main__":
    main()
