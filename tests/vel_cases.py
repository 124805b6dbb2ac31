"""Seam-(2) jobs placed ON the decision boundaries of the velocity stage (tests/test_vel_cases_host.py on the CPU, tests/test_gpu_vel_ref.py
on the GPU), next to tests/vel_jobs.py whose edge jobs name several of these decisions without placing them. Pure NumPy on top of the
long-double reference tests/vel_ref.py; nothing here runs a kernel.

`families(lat, k)` returns, for the kernel variant k of vel_jobs.VARIANT_SETS (exponent 1 / 2 / general x one-row / interpolated machine
table), a list of (family, group name, VelParamSet, jobs): a group is one call of ltpl_vel_profile. Every job is built TWICE: with a constant loc_gg and with a row-wise one (name suffix
" [gg rows]"; increments are multiples of 1/8 so that sums stay exact where a case relies on it). n <= 200 throughout, except in the
family `chunk` (vel_jobs.chunk_edge_jobs at the chunk-edge lengths and the longest accepted length).

Where a boundary is a value of the SOLUTION (the unclamped speed of a step, the start speed at which standstill moves on by a point, the
start speed at which the brake profile passes 0.1 m/s at a point, the first row at which the brake profile is below the control speed) it
is found by bisection on the long-double reference down to neighbouring doubles, and the input is placed at boundary x (1 -+ 1e-9)
(`REL`). Boundaries that are values of the INPUTS are placed exactly (integers and dyadic values: the sums are exact in every number
type) and at np.nextafter on either side.

The margin is a condition on the cases: on every job the fp64 evaluation of vel_ref must take the decisions of its long-double
evaluation (tests/test_vel_cases_host.py asserts equal traces for all of them and prints the smallest margin that occurs: every job
placed beside a bisected boundary carries its measured relative distance from it, `margin`).

  table      start speeds exactly on a row of the machine table (first, inner, last), np.nextafter on both sides of each, below the first and
             above the last row; tables of 2 and of 64 rows; two rows 1e-3 m/s apart with different limits
  runs       plateaus of exactly equal limit speed (equal kappa: difference exactly 0, no run starts); runs that start at step 0, at the
             last step, at steps 63, 64 and 65 (last lane of a pass, first lanes of the next), each as the only run of a forward sweep and,
             mirrored, of a backward sweep; a run
             that starts at step 60 and breaks at "> v_max" in the next pass
  vmax       v_max at (1 -+ 1e-9) x the unclamped speed of step 10 and of step 70 of a straight; a parameter set whose drag exceeds the
             drive at v_max behind a row that still accelerates past it (breaking and continuing give different profiles there)
  radicand   brake jobs that enter a corner at q = v^2 kappa / ay_max = 0.5, 1, 2, 3 (from 1 on: radicand <= 0, tyre share 0); a backward run
             onto the lateral limit of a corner and along it, bends whose limit a profile rides and brakes along (q = 1 to rounding); a
             straight (kappa = 0: 0^e with the general exponent). A FORWARD run along a constant limit is left out on purpose: it dips
             below the limit by the drag and recovers, a two-step oscillation whose onset rounding decides (no margin to be had)
  standstill v_start at (1 -+ 1e-9) x the start speed at which the stop moves from point k to k + 1, k = 63, 64, 65, 128; v_start = 0;
             v_end = 0 and v_start = v_end = 0 forward-backward; a brake profile that passes 0.1 m/s within 1e-9 at point 40, either side
  follow     see follow_family
  chunk      vel_jobs.chunk_edge_jobs: every mode at n - 1 on either side of the 64 steps of a pass and of the unroll by four, and at the
             longest accepted length

An opponent that never stops within a lap cannot be had on Monteblanco (at 14 m/s^2 from at most the race line's 60 m/s it stops within
130 m of a 2.4 km lap): `short_lap_case` builds an 80 m oval whose corners leave the tyres no longitudinal share, and a follow job on it.
"""
import numpy as np

import vel_ref as R
from projection_cases import Line, restate
from vel_jobs import VARIANT_SETS, CTRL_PARAMS, table_64_rows
from graphbasedlocaltrajectoryplanner_amd import _capi

REL = 1e-9
LD = R.LD
FB, BRAKE, FOLLOW = _capi.VEL_FB, _capi.VEL_BRAKE, _capi.VEL_FOLLOW
N = 150
V_MAX = 95.0


# the follow family's controller constants and vehicle length are dyadic, so that control_d, safety_d + len_veh and v_control are exact in
# fp64 and in long double wherever a case puts an input EXACTLY on one of them (vel_jobs.CTRL_PARAMS: 1.15, 0.025, 0.2, 15 are not)
DYADIC_CTRL = {"c_p": 1.25, "k_d": 0.03125, "k_p": 0.25, "tan_w": 16.0}
DYADIC_LEN_VEH = 4.75


def vp_of(lat, k, v_max=V_MAX, axm=None, drag=0.85, dyadic=False):
    exp, table, ctrl, _ = VARIANT_SETS[k]
    return _capi.VelParamSet(dyn_model_exp=exp, drag_coeff=drag, m_veh=1000.0, len_veh=DYADIC_LEN_VEH if dyadic else lat.veh_length,
                             v_max=float(v_max), ax_max_machines=table if axm is None else axm, follow_control_type=ctrl,
                             follow_control_params=dict(DYADIC_CTRL if dyadic else CTRL_PARAMS))


def gg_of(n, rows, ax=6.0, ay=5.0, ay_rows=True):
    """Constant (ax, ay), or row-wise: ax + k / 4, ay + k / 8 with k cycling (``ay_rows`` False keeps ay constant: the limit speed of a
    plateau of equal kappa stays exactly equal)."""
    if not rows:
        return np.tile([float(ax), float(ay)], (n, 1))
    i = np.arange(n)
    return np.column_stack((ax + 0.25 * ((i * 7) % 9), ay + (0.125 * ((i * 5) % 7) if ay_rows else np.zeros(n))))


def job(name, mode, kappa, rows, el=2.5, v_start=30.0, v_end=None, gg=None, ay_rows=True, **follow):
    kappa = np.asarray(kappa, np.float64)
    n = kappa.size
    el = np.full(n - 1, float(el)) if np.isscalar(el) else np.asarray(el, np.float64)
    jb = {"name": name + (" [gg rows]" if rows else ""), "mode": mode, "kappa": kappa, "v_start": float(v_start),
          "loc_gg": gg_of(n, rows, ay_rows=ay_rows) if gg is None else np.asarray(gg, np.float64)}
    if mode == FOLLOW:
        jb["el_lengths"] = np.append(el, 0.0)
        jb.update(follow)
    else:
        jb["el_lengths"] = el
        if mode == FB:
            jb["v_end"] = v_end
    return jb


def bisect(pred, lo, hi):
    """pred(lo) false, pred(hi) true -> the smallest double at which pred holds (as far as pred is monotonic)."""
    assert not pred(lo) and pred(hi), (lo, hi)
    while True:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            return hi
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)


def both_sides(x):
    return (("below", x * (1.0 - REL)), ("above", x * (1.0 + REL)))


# ---------------------------------------------------------------- the families without an opponent

def table_family(lat, k, rows):
    out = []
    zero = np.zeros(N)
    for tag, table in (("own", VARIANT_SETS[k][1]), ("2 rows", [[20.0, 6.0], [60.0, 3.0]]), ("64 rows", table_64_rows()),
                       ("rows 1e-3 apart", [[0.0, 6.0], [30.0, 6.0], [30.001, 3.0], [80.0, 2.5]])):
        table = np.asarray(table, np.float64)
        speeds = []
        for r in sorted({0, len(table) // 2, len(table) - 1}):
            v = float(table[r, 0])
            speeds += [("on row %d" % r, v), ("just above row %d" % r, float(np.nextafter(v, np.inf)))]
            if v > 0.0:                                 # (a first row at 0 m/s has nothing below it: v_start < 0 is clamped to 0)
                speeds.append(("just below row %d" % r, float(np.nextafter(v, -np.inf))))
        if table[0, 0] > 0.0:
            speeds.append(("below the first row", float(table[0, 0]) / 2.0))
        speeds.append(("above the last row", float(table[-1, 0]) + 3.0))
        jobs = [job("table %s: straight from %s" % (tag, what), FB, zero[:60 + 7 * (i % 5)], rows, v_start=min(v, 110.0), el=1.0 + 0.5 * (i % 3))
                for i, (what, v) in enumerate(speeds)]
        out.append(("table " + tag, vp_of(lat, k, v_max=120.0, axm=table), jobs))
    return out


def corner_then_straight(n, last_corner_row, kappa=0.05):
    kap = np.zeros(n)
    kap[:last_corner_row + 1] = kappa
    return kap


def runs_family(lat, k, rows):
    jobs = []
    # limits that fall from plateau to plateau: no forward run; the backward sweep starts one run per edge and meets every plateau from its
    # slow end (a forward run that RIDES a limit dips below it by the drag and recovers, a two-step oscillation whose onset rounding decides)
    plateau = np.repeat([0.0, 0.03125, 0.05, 0.0625], 30)
    jobs.append(job("runs: plateaus of equal kappa, start above the first limit", FB, plateau, rows, v_start=120.0, v_end=5.0, ay_rows=False))
    jobs.append(job("runs: one plateau, no run at all", FB, np.full(70, 0.05), rows, v_start=60.0, ay_rows=False))
    jobs.append(job("runs: run from step 0", FB, np.zeros(N), rows, v_start=5.0))
    for s in (63, 64, 65):
        kap = corner_then_straight(N, s)
        jobs.append(job("runs: forward run from step %d" % s, FB, kap, rows, v_start=60.0, ay_rows=False))
        # mirrored: the corner's plateau (steps 0 .. s - 1: differences exactly 0), then the straight at v_max. v_start >= v_max and a free end:
        # no forward run (a forward run THROUGH the corner rides its limit, see above) and no backward run from the end clamp
        jobs.append(job("runs: backward run from step %d" % s, FB, kap[::-1].copy(), rows, v_start=120.0, ay_rows=False))
    last = corner_then_straight(N, N - 2)
    jobs.append(job("runs: forward run from the last step", FB, last, rows, v_start=60.0, ay_rows=False))
    jobs.append(job("runs: backward run from the last step", FB, last[::-1].copy(), rows, v_start=120.0, ay_rows=False))
    out = [("runs", vp_of(lat, k), jobs)]
    # a run that starts at step 60 (first pass) and breaks at "> v_max" in the second: v_max = the long-double solution's speed at step 70
    jb = job("probe", FB, corner_then_straight(N, 60), rows, v_start=60.0, ay_rows=False)
    vx, _, _ = R.calc_vel_profile(jb["kappa"], jb["el_lengths"], jb["loc_gg"], 1000.0, jb["v_start"], None, R.Params(vp_of(lat, k)), LD)
    jb["name"] = "runs: starts at step 60, breaks above v_max in the next pass" + (" [gg rows]" if rows else "")
    out.append(("runs across a pass", vp_of(lat, k, v_max=float(vx[70]) * (1.0 - 1e-3)), [jb]))
    return out


def unclamped_speed(P, jb, step):
    """The speed the forward sweep's step ``step`` -> step + 1 computes on a profile no limit touches (v_max far away)."""
    vx, _, _ = R.calc_vel_profile(jb["kappa"], jb["el_lengths"], jb["loc_gg"], 1e4, jb["v_start"], None, P, LD)
    return float(vx[step + 1])


def vmax_family(lat, k, rows):
    out = []
    for step in (10, 70):
        jb = job("probe", FB, np.zeros(N), rows, v_start=20.0, el=3.0)
        v = unclamped_speed(R.Params(vp_of(lat, k)), jb, step)
        for side, vm in both_sides(v):
            j = dict(jb, name="vmax: v_max %s the speed of step %d" % (side, step) + (" [gg rows]" if rows else ""), margin=float(abs(LD(vm) / LD(v) - 1)))
            out.append(("vmax step %d %s" % (step, side), vp_of(lat, k, v_max=vm), [j]))
    # drag 4.0 m/s^2 at v_max = 50 m/s: rows with ax_max 8 drive past v_max (machine 5 or 6 > 4), rows with ax_max 3 cannot hold it
    n = 120
    gg = gg_of(n, rows)
    gg[:, 0] = np.where((np.arange(n) // 8) % 2 == 0, 8.0, 3.0) if rows else 8.0
    jb = job("vmax: drag exceeds the drive at v_max", FB, np.zeros(n), rows, v_start=49.5, el=3.0, gg=gg)
    out.append(("vmax drag", vp_of(lat, k, v_max=50.0, drag=1.6, axm=[[100.0, 5.0]] if len(VARIANT_SETS[k][1]) == 1 else [[0.0, 6.0], [72.0, 5.0]]), [jb]))
    return out


def radicand_family(lat, k, rows):
    jobs = []
    kap = np.full(100, 0.04)
    for q in (0.5, 1.0, 2.0, 3.0):
        jobs.append(job("radicand: brake into a corner at q = %g" % q, BRAKE, kap, rows, v_start=float(np.sqrt(q * 5.0 / 0.04)), ay_rows=False))
    bend = 0.02 + 0.02 * np.sin(np.linspace(0.0, 3.0 * np.pi, N)) ** 2
    jobs.append(job("radicand: forward run towards the lateral limit of a corner", FB, np.full(12, 0.03125), rows, v_start=8.0, ay_rows=False))
    jobs.append(job("radicand: backward run onto the lateral limit, then along it (q = 1 to rounding)", FB, np.full(N, 0.03125), rows, v_start=60.0,
                    v_end=4.0, ay_rows=False))
    jobs.append(job("radicand: rides the limit of a bend of varying curvature", FB, bend, rows, v_start=25.0, v_end=5.0))
    jobs.append(job("radicand: brake along the limit of a bend", BRAKE, bend, rows, v_start=float(np.sqrt(5.0 / bend[0]))))
    jobs.append(job("radicand: straight, kappa = 0", FB, np.zeros(80), rows, v_start=10.0, v_end=3.0))
    jobs.append(job("radicand: brake on a straight, kappa = 0", BRAKE, np.zeros(80), rows, v_start=40.0))
    return [("radicand", vp_of(lat, k), jobs)]


def brake_stop(P, jb, v0, T=LD):
    return R.calc_vel_profile_brake(jb["kappa"], jb["el_lengths"], jb["loc_gg"], v0, P, T)


def standstill_family(lat, k, rows):
    P = R.Params(vp_of(lat, k))
    jobs = []
    for stop in (63, 64, 65, 128):
        jb = job("probe", BRAKE, np.zeros(200), rows, v_start=1.0, el=1.0)
        v_b = bisect(lambda v0: brake_stop(P, jb, v0)[1] > stop, 0.5, 150.0)        # standstill moves from point `stop` to `stop + 1`
        for side, v0 in both_sides(v_b):
            jobs.append(dict(jb, v_start=v0, margin=float(abs(LD(v0) / LD(v_b) - 1)),
                             name="standstill: v_start %s the move of the stop from point %d to %d" % (side, stop, stop + 1) + (" [gg rows]" if rows else "")))
    jb = job("probe", BRAKE, np.zeros(N), rows, v_start=1.0, el=1.0)
    # (the speed at point 40 moves ~1e4 times as fast as v_start there: the two sides are bisected for themselves, 1e-9 of 0.1 m/s apart each)
    for side, target in both_sides(0.1):
        v0 = bisect(lambda v0: brake_stop(P, jb, v0)[0][40] > LD(target), 0.5, 150.0)
        v0 = v0 if side == "above" else float(np.nextafter(v0, -np.inf))
        # (margin: of the boundary VALUE, the speed at point 40 against 0.1 m/s; in v_start the two sides are ~1e-13 apart. Nothing in the
        # trace of a brake job depends on 0.1 m/s, so the condition on the cases holds all the same.)
        jobs.append(dict(jb, v_start=v0, margin=float(abs(brake_stop(P, jb, v0)[0][40] / LD(0.1) - 1)),
                         name="standstill: brake profile %s 0.1 m/s at point 40" % side + (" [gg rows]" if rows else "")))
    jobs.append(job("standstill: brake from v_start = 0", BRAKE, np.zeros(70), rows, v_start=0.0))
    jobs.append(job("standstill: v_start = 0", FB, 0.03 * np.sin(np.linspace(0, 5, N)), rows, v_start=0.0))
    jobs.append(job("standstill: v_end = 0", FB, 0.03 * np.sin(np.linspace(0, 5, N)), rows, v_start=25.0, v_end=0.0))
    jobs.append(job("standstill: v_start = 0, v_end = 0", FB, np.zeros(66), rows, v_start=0.0, v_end=0.0))
    return [("standstill", vp_of(lat, k), jobs)]


# ---------------------------------------------------------------- follow mode

def raceline(lat):
    G = lat.glob_rl.shape[0] - 1
    return Line("raceline", lat.glob_rl[:G, 1], lat.glob_rl[:G, 2], lat.glob_rl[:G, 0], True)


def opp_index(lat, jobs):
    """Index of the race-line point behind every follow job's object (projection reference), None for the other modes."""
    fj = [i for i, jb in enumerate(jobs) if jb["mode"] == FOLLOW]
    out = [None] * len(jobs)
    if fj:
        r = restate(raceline(lat), [jobs[i]["obj_pos"][0] for i in fj], [jobs[i]["obj_pos"][1] for i in fj])
        assert bool(np.all(r.decided)), "an object of a follow job lies on a boundary of the projection"
        for i, p in zip(fj, r.pair[:, 0]):
            out[i] = int(p)
    return out


def obj_at(lat, row, lateral=0.75, along=0.4):
    """A point next to race-line row ``row``: 40 % of the way to the next row and 0.75 m to the side (far from the projection's boundaries)."""
    g = lat.glob_rl
    p, q = g[row, 1:3], g[row + 1, 1:3]
    t = (q - p) / np.hypot(*(q - p))
    return (float(p[0] + along * (q[0] - p[0]) - lateral * t[1]), float(p[1] + along * (q[1] - p[1]) + lateral * t[0]))


def follow_family(lat, k, rows):
    """Straight path of integer element lengths (1 m or 2 m: s[k] and every sum exact) unless said otherwise; safety_d = 20.25, vehicle length
    4.75; the controller's constants dyadic too (DYADIC_CTRL). With v_obj = 0 the opponent's stop distance is 0 and s_stop = obj_dist - (safety_d + len_veh).
      too_close    obj_dist == fl(safety_d + len_veh) and np.nextafter below
      s_stop       exactly s[k] (stop_idx = k), np.nextafter on both sides; beyond s[n_el - 1] (v_end from the race line); stop_idx 0, 1, 2
      ego stop     ego_stop == s_stop and one metre on either side (brake to standstill within an integer number of metres)
      v_control    v_start == v_control, np.nextafter on both sides; clamped to 0 and to v_max; the PDtan argument beyond both clamps
      idx_c        first vx <= v_control at (1 -+ 1e-9) (v_control between two rows of the brake profile); idx_c == 0 (no row at or below
                   v_control: becomes stop_idx); idx_c above stop_idx (v_control 0 and a car that crawls on below 0.1 m/s on ax_max rows of
                   5e-4 m/s^2: cut back to stop_idx)
      standstill   stop_idx = 1 reached with ego_stop < s_stop (v_start below 0.1 m/s: vel_bound 0; stop_idx = 0 cannot be, ego_stop >= 0);
                   v_start and v_obj exactly 0.1 m/s and np.nextafter above (v > 0.1 is strict)
      v_obj        == the race line's speed at the object, np.nextafter on both sides; an opponent whose stop scan crosses the seam
      flags        both values of both flags occur; the two |.| > 1.0 m/s thresholds of vel_bound are passed by >= 0.5 m/s on either side
                   (asserted by the host test on the long-double reference)"""
    vp = vp_of(lat, k, dyadic=True)
    P = R.Params(vp)
    G = lat.glob_rl.shape[0] - 1
    sd = 20.25
    lim = float(np.float64(sd) + np.float64(P.len_veh))
    n = 120
    zero = np.zeros(n)
    mid_row = 300
    far = dict(safety_d=sd, obj_pos=obj_at(lat, mid_row), v_ego=20.0)
    jobs = []

    def fj(name, v_start=20.0, el=1.0, kappa=zero, **kw):
        f = dict(far)
        f.update(kw)
        f.setdefault("v_ego", v_start)
        return job("follow: " + name, FOLLOW, kappa, rows, el=el, v_start=v_start, **f)

    jobs.append(fj("obj_dist == safety_d + len_veh", v_obj=10.0, obj_dist=lim))
    jobs.append(fj("obj_dist just below safety_d + len_veh", v_obj=10.0, obj_dist=float(np.nextafter(lim, -np.inf))))
    for kk in (0, 1, 2, 3, 64, n - 1):
        on = float(np.float64(lim) + np.float64(kk))                                  # exact: 25 + kk, and obj_dist - 25 is exact on either side
        for tag, d in (("on", on), ("just below", float(np.nextafter(on, -np.inf))), ("just above", float(np.nextafter(on, np.inf)))):
            jobs.append(fj("s_stop %s s[%d]" % (tag, kk), v_start=3.0, v_obj=0.0, obj_dist=d))
    jobs.append(fj("s_stop beyond the path's end, v_end from the race line", v_obj=30.0, obj_dist=400.0))
    # ego stop distance: the brake profile from v_start = 6 on 1 m elements falls below 0.1 m/s after idb metres
    idb = R.first_not_above(brake_stop(P, fj("probe", v_start=6.0), 6.0)[0], LD(0.1))
    for tag, d in (("one metre short of", idb - 1), ("equal to", idb), ("one metre beyond", idb + 1)):
        jobs.append(fj("s_stop %s the ego stop distance" % tag, v_start=6.0, v_obj=0.0, obj_dist=float(np.float64(lim) + np.float64(d))))
    # v_control (PD: v_obj - k_p (control_d - obj_dist) + k_d (v_obj - v_ego); PDtan likewise through tan): the job's own fp64 value
    for tag, shift in (("==", 0), ("just above", 1), ("just below", -1)):
        jb = fj("v_start %s v_control" % tag, v_obj=4.0, obj_dist=float(1.25 * sd + DYADIC_LEN_VEH), v_ego=3.0)      # obj_dist == control_d; slow enough to stop short of s_stop
        vc = control_speed(P, jb)
        assert vc == 4.03125
        v0 = float(vc if shift == 0 else np.nextafter(vc, np.inf if shift > 0 else -np.inf))
        jobs.append(dict(jb, v_start=v0))
    jobs.append(fj("v_control clamped to 0", v_obj=0.5, obj_dist=float(lim + 1.0), v_start=4.0))
    jobs.append(fj("v_control clamped to v_max, PDtan argument below its clamp", v_obj=94.9, obj_dist=350.0, v_start=30.0, v_ego=20.0))
    jobs.append(fj("PDtan argument above its clamp", v_obj=12.0, obj_dist=10.0, v_start=15.0))
    # idx_c: v_control between rows 7 and 8 of the ego brake profile, (1 -+ 1e-9) around row 8's speed (obj_dist inside PDtan's clamps: beyond
    # them v_control is a difference of numbers of 2.5e4 m/s and 1e-9 is no margin)
    base = fj("probe", v_start=14.0, v_obj=8.0, obj_dist=44.0)
    vb = brake_stop(P, base, 14.0)[0]
    for side, target in both_sides(float(vb[8])):
        jb = dict(base, name="follow: v_control %s row 8 of the brake profile" % side + (" [gg rows]" if rows else ""))
        jb = with_control_speed(P, jb, target)
        jobs.append(dict(jb, margin=float(abs(LD(control_speed(P, jb, LD)) / vb[8] - 1))))
    # idx_c == 0: v_start above v_control, but no row of the brake profile at or below it within the path (40 points): becomes stop_idx = 39
    jobs.append(fj("no row at or below v_control: idx_c = 0 becomes stop_idx", kappa=np.zeros(40), v_start=60.0, v_obj=40.0, obj_dist=44.0, v_ego=60.0,
                   obj_pos=obj_at(lat, 20 + int(np.argmax(lat.glob_rl[20:G - 20, 4])))))       # (obj_dist inside PDtan's clamps; s_stop beyond the end)
    # idx_c above stop_idx: v_control clamped to 0, ax_max rows that let the car crawl on below 0.1 m/s (idb = 4, standstill rows later), s_stop
    # = 4.5 between them: the first row at or below v_control lies beyond stop_idx = 5 and is cut back to it
    step_row = 5 if rows else 4
    crawl = gg_of(n, False)
    crawl[:, 0] = np.where(np.arange(n) < step_row, 0.0105, 5e-4)
    jobs.append(job("follow: idx_c above stop_idx (ax_max step at row %d)" % step_row, FOLLOW, zero, False, el=1.0, v_start=0.3 if not rows else 0.335, gg=crawl,
                    **dict(far, v_obj=0.0, obj_dist=float(lim + (4.5 if not rows else 5.5)), v_ego=20.0)))     # (v_ego far above: v_control < 0, clamped to 0)
    # stop_idx below 2 with ego_stop < s_stop needs a car below 0.1 m/s (idb = 0): vel_bound 0 through stop_idx = 1
    jobs.append(fj("stop_idx 1 from below 0.1 m/s: vel_bound 0", v_start=0.05, v_obj=0.0, obj_dist=float(lim + 0.5), v_ego=0.05))
    # the standstill threshold itself: v exactly 0.1 m/s is NOT above it (in w = v^2: fl(0.1 * 0.1) > 0.01)
    jobs.append(fj("v_start == 0.1 exactly", v_start=0.1, v_obj=0.0, obj_dist=float(lim + 0.5), v_ego=0.1))
    jobs.append(fj("v_start just above 0.1", v_start=float(np.nextafter(0.1, np.inf)), v_obj=0.0, obj_dist=float(lim + 0.5), v_ego=0.1))
    jobs.append(fj("v_obj == 0.1 exactly", v_start=3.0, v_obj=0.1, obj_dist=float(lim + 10.0), v_ego=3.0))
    jobs.append(fj("v_obj just above 0.1", v_start=3.0, v_obj=float(np.nextafter(0.1, np.inf)), obj_dist=float(lim + 10.0), v_ego=3.0))
    # v_obj against the race line's speed at the object
    v_rl = float(lat.glob_rl[mid_row, 4])
    for tag, v in (("==", v_rl), ("just below", float(np.nextafter(v_rl, -np.inf))), ("just above", float(np.nextafter(v_rl, np.inf)))):
        jobs.append(fj("v_obj %s the race line's speed at the object" % tag, v_obj=v, obj_dist=150.0, v_start=35.0))
    jobs.append(fj("opponent's stop scan crosses the seam", v_obj=60.0, obj_dist=150.0, v_start=35.0, obj_pos=obj_at(lat, G - 6)))
    jobs.append(fj("opponent on the last race-line segment before the seam", v_obj=40.0, obj_dist=100.0, v_start=30.0, obj_pos=obj_at(lat, G - 1)))
    # a bend, so that the segment profile's start is limited: vel_bound 0 through the first threshold
    bend = 0.05 * np.ones(n)
    jobs.append(fj("segment profile starts below v_start by more than 1 m/s", kappa=bend, v_start=25.0, v_obj=30.0, obj_dist=300.0, ay_rows=False))
    jobs.append(fj("far behind a faster opponent", v_start=25.0, v_obj=40.0, obj_dist=300.0))
    return [("follow", vp, jobs)]


def control_speed(P, jb, T=np.float64):
    """v_control of a follow job as fp64 computes it (before the clamps)."""
    control_d = T(P.c_p) * T(jb["safety_d"]) + T(P.len_veh)
    if P.ctrl == 0:
        return float(T(jb["v_obj"]) - T(P.k_p) * (control_d - T(jb["obj_dist"])) + T(P.k_d) * (T(jb["v_obj"]) - T(jb["v_ego"])))
    pi = T(np.pi)
    a = (control_d - T(jb["obj_dist"])) * pi / 2 * 1 / T(P.tan_w)
    a = min(max(a, -pi / 2 + T(1e-5)), pi / 2 - T(1e-5))
    return float(T(jb["v_obj"]) - np.tan(a) * T(P.k_p) + T(P.k_d) * (T(jb["v_obj"]) - T(jb["v_ego"])))


def with_control_speed(P, jb, target):
    """The job with v_obj moved so that the LONG-DOUBLE control speed is ``target`` to a few ulp (v_control is affine in v_obj)."""
    jb = dict(jb)
    for _ in range(4):
        jb["v_obj"] = float(LD(jb["v_obj"]) + (LD(target) - LD(control_speed(P, jb, LD))) / (LD(1) + LD(P.k_d)))
    return jb


LONGEST_N = 2073       # the longest job ltpl_vel_profile accepts on an MI355X (tests/test_gpu_vel.py finds it by bisection; asserted by the GPU test)


def chunk_family(lat, k, rows):
    """vel_jobs.chunk_edge_jobs: every mode at the lengths whose n - 1 lies on either side of the 64 steps of a pass and of the unroll by
    four, and at the longest accepted length (the one exception to n <= 200). Seeded random jobs: they sit on no boundary, and the same
    condition holds for them as for every other job."""
    from vel_jobs import chunk_edge_jobs, CHUNK_EDGE_LENGTHS
    jobs = chunk_edge_jobs(lat, 400 + k, rows, CHUNK_EDGE_LENGTHS + (LONGEST_N,))
    for jb in jobs:
        jb["name"] = "chunk: " + jb["name"] + (" [gg rows]" if rows else "")
    return [("chunk", vp_of(lat, k, v_max=60.0 + 6.0 * k), jobs)]


BUILDERS = (("table", table_family), ("runs", runs_family), ("vmax", vmax_family), ("radicand", radicand_family),
            ("standstill", standstill_family), ("follow", follow_family), ("chunk", chunk_family))
_cache = {}


def families(lat, k):
    """[(family, group name, VelParamSet, jobs)] of variant k; a group is one call of ltpl_vel_profile (one parameter set). Jobs with
    constant and with row-wise loc_gg alternate inside a group, so that neighbours differ."""
    if k not in _cache:
        out = []
        for fam, build in BUILDERS:
            const, rowwise = build(lat, k, False), build(lat, k, True)
            for (name, vp, ja), (_, vp_r, jr) in zip(const, rowwise):
                if R.Params(vp).v_max == R.Params(vp_r).v_max:
                    out.append((fam, name, vp, [j for pair in zip(ja, jr) for j in pair]))
                else:                                       # (a bisected v_max depends on the gg: a parameter set each)
                    out.append((fam, name, vp, ja))
                    out.append((fam, name + " [gg rows]", vp_r, jr))
        _cache[k] = out
    return _cache[k]


def short_lap_lattice():
    """An oval of 80 m (16 layers of 5 m, corner radius 8 m): 55 m/s on its straights, kappa = 0.125 1/m in its corners."""
    from graphbasedlocaltrajectoryplanner_amd.synthetic_lattice import make_oval_lattice
    if "short" not in _cache:
        _cache["short"] = make_oval_lattice(num_layers=16, nodes_per_layer=3, layer_spacing=5.0, lat_resolution=0.5, lat_steps=1, radius=8.0,
                                            horizon=20.0)
    return _cache["short"]


def short_lap_case(k):
    """(lattice, VelParamSet, jobs): follow jobs behind an opponent that enters its stop scan at 55 m/s on an 80 m lap -- 14 m/s^2 take
    2 240 m^2/s^2 of its 3 025 within a lap at best: the scan ends after one lap (opp_idb = G) without a stop -- and behind one that stops."""
    lat = short_lap_lattice()
    vp = vp_of(lat, k, dyadic=True)
    jobs = []
    for rows in (False, True):
        for name, v_obj in (("opponent that never stops within a lap", 55.0), ("opponent that stops within the short lap", 20.0)):
            jobs.append(job("follow: " + name, FOLLOW, np.zeros(60 if rows else 90), rows, el=1.0, v_start=20.0, safety_d=20.25, obj_pos=obj_at(lat, 2),
                            v_ego=20.0, v_obj=v_obj, obj_dist=60.0))
    return lat, vp, jobs


# ---------------------------------------------------------------- tick-level batches

TICK_N = 256
TICK_SEED = 5          # the seed of tests/test_gpu_vel_variants.py; counted share of decision-unstable slots: 0 of 3 870 valid slots over the twelve batches (host test)
TICK_GENS = ("random", "c2")
UNSTABLE_SHARE = 0.02


def tick_inputs(lat, name, gen, n=TICK_N):
    """(scenarios, vehicle speeds, PathsBatch, TickVelBatch) of the first ``n`` scenarios of the batch (parameter set ``name`` of
    test_gpu_vel_variants.SETS, generator ``gen``): 256 Monteblanco scenarios of random_scenarios / c2_scenarios(lead_gap=(8, 80))."""
    from test_gpu_vel_variants import scenarios_of, vel_batch
    from test_gpu_default_routes import sub_batch
    key = ("tick", gen)
    if key not in _cache:
        _cache[key] = scenarios_of(lat, gen, TICK_N)
    scen, vels = _cache[key]
    vel = vel_batch(lat, name, scen, vels, TICK_SEED + 1)
    batch, v = sub_batch(scen, vels, vel, 0, n)
    return scen[:n], vels[:n], batch, v


# ---------------------------------------------------------------- classes, parts and bounds

RAD_SPLIT = 1e-3
PARTS = ("regular", "ill")
# Derived by tests/test_vel_cases_host.py (which asserts that the derivation still gives these): per exponent class, quantity and part
# 100 x the worst deviation of the fp64 evaluation of vel_ref from its long-double evaluation over the class's rows -- every seam job of
# every family and the decision-stable slots of the twelve tick batches on the oracle's paths -- rounded up to one digit, within
# [100 eps, 1e-5]. A class whose single bound would exceed 1e-8 is split at RAD_SPLIT (vel_ref: `rad`): "ill" = the rows whose value went
# through a step with a radicand below 1e-3, "regular" = the rest. A class that is not split has the same bound in both parts.
BOUNDS = {
    ("exp1", "vx", "regular"): 5e-10, ("exp1", "vx", "ill"): 5e-8, ("exp1", "ax", "regular"): 4e-10, ("exp1", "ax", "ill"): 4e-10,
    ("exp2", "vx", "regular"): 3e-10, ("exp2", "vx", "ill"): 1e-5, ("exp2", "ax", "regular"): 5e-10, ("exp2", "ax", "ill"): 1e-5,
    ("general", "vx", "regular"): 3e-10, ("general", "vx", "ill"): 1e-5, ("general", "ax", "regular"): 2e-10, ("general", "ax", "ill"): 8e-8,
}


class Deviations(object):
    """Worst element-wise deviation from the long-double reference per (exponent class, quantity, part), and where it occurred."""

    def __init__(self):
        self.worst = {}

    def add(self, cls, quantity, got, ref, rad, what):
        floor = R.FLOOR_VX if quantity == "vx" else R.FLOOR_AX
        ref = np.asarray(ref, LD)
        if ref.size == 0:
            return
        d = (np.abs(np.asarray(got, LD) - ref) / np.maximum(np.abs(ref), LD(floor))).astype(np.float64)
        ill = np.asarray(rad) < RAD_SPLIT
        for part, sel in (("regular", ~ill), ("ill", ill)):
            if sel.any():
                i = int(np.argmax(np.where(sel, d, -1.0)))
                if d[i] > self.worst.get((cls, quantity, part), (-1.0, ""))[0]:
                    self.worst[cls, quantity, part] = (float(d[i]), "%s row %d" % (what, i))

    def of(self, cls, quantity, part=None):
        keys = [(cls, quantity, p) for p in (PARTS if part is None else (part,))]
        return max([self.worst.get(k, (0.0, ""))[0] for k in keys])

    def bounds(self):
        out = {}
        for cls in ("exp1", "exp2", "general"):
            for q in ("vx", "ax"):
                single = R.bound_of(self.of(cls, q))
                for part in PARTS:
                    out[cls, q, part] = single if single <= 1e-8 else min(R.bound_of(self.of(cls, q, part)), single)
        return out


def ax_rad(rad):
    """The part of an ax row: ax[i] is formed from vx[i] and vx[i + 1]."""
    rad = np.asarray(rad)
    return np.minimum(rad, np.append(rad[1:], np.inf))


def check_rows(cls, quantity, got, ref, rad, what, bounds=None):
    """Assert ``got`` within the class's bound of the long-double ``ref`` row by row, exactly 0 where the reference is 0; the failure
    names the case and the row. Returns the worst deviation. (The converse of the zeros is the bound's business: the kernels carry v^2,
    in which a subnormal v_start is 0.)"""
    bounds = BOUNDS if bounds is None else bounds
    floor = R.FLOOR_VX if quantity == "vx" else R.FLOOR_AX
    got, ref = np.asarray(got, np.float64), np.asarray(ref, LD)
    assert got.shape == ref.shape, "%s: %d rows, reference %d" % (what, got.size, ref.size)
    if ref.size == 0:
        return 0.0
    zero = ref == 0
    assert bool(np.all(got[zero] == 0.0)), "%s %s: not exactly 0 at rows %s where the reference is" % (what, quantity, np.flatnonzero(zero & (got != 0.0))[:8])
    d = (np.abs(got.astype(LD) - ref) / np.maximum(np.abs(ref), LD(floor))).astype(np.float64)
    lim = np.where(np.asarray(rad) < RAD_SPLIT, bounds[cls, quantity, "ill"], bounds[cls, quantity, "regular"])
    bad = np.flatnonzero(~(d <= lim))
    assert bad.size == 0, "%s %s row %d: %.17g, reference %.17g: deviation %.2e > %.1e (radicand %.1e)" % (
        what, quantity, bad[0], got[bad[0]], float(ref[bad[0]]), d[bad[0]], lim[bad[0]], np.asarray(rad)[bad[0]])
    return float(d.max())
