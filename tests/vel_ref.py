"""Reference of the velocity stage (csrc/vel_wave.hpp, csrc/vel_lanes.hpp: k_vel_profile, k_tick, k_tick_persistent, k_follow_prep ->
k_vel_lanes -> k_vel_final) and the comparison against it. NumPy only, with the number type as a parameter: np.longdouble by default (THE
reference), np.float64 on request (what an fp64 evaluation of the same formulas can reach: the source of the bounds and of the margins).

Written in the REFERENCE'S FORMULATION, from the operation as the kernels' comments, oracle/ltpl_oracle.c and
oracle/shims/trajectory_planning_helpers/ document it -- not in the kernels': the state is v (the kernels carry w = v^2 and compare in w),
scalar loops (the wave form is systolic), the machine table through np.interp's formula slope * (x - x0) + f0 (exponent 1 with one row is
an affine fma form in the kernels), divisions are divisions (the kernels use reciprocals with Newton steps), running sums in the order of
np.cumsum. Every input is an fp64 value and is converted exactly; literals (0.1, 14.0, 1e-5, pi) are the fp64 constants in every number type.

  calc_ax_poss   ay = v^2 / radius; radicand = 1 - (ay / ay_max)^e; tyre share = ax_max radicand^(1/e) if radicand > 0 else 0; forward
                 acceleration: min(tyre share, machine table at v); drag v^2 c / m subtracted (forward) or added (backward sweep)
  calc_vel_profile (closed=False)
                 limit profile min(sqrt(ay_max radius), v_max), first point clamped to v_start; forward sweep; last point clamped to v_end;
                 backward sweep on the mirrored profile, radii and element lengths with UNMIRRORED gg rows (the reference's quirk). A sweep
                 finds the first point of every run of positive differences of the profile BEFORE it runs, then integrates from every start
                 until the next start or until a step's unclamped speed exceeds v_max.
  calc_vel_profile_brake
                 v' = sqrt(v^2 + 2 a el) until the radicand turns negative; zeros from there on
  calc_vel_profile_follow, tick_slot     see the functions

Every function returns a DECISION TRACE next to the floats: a nested tuple of integers (run starts, the step every run ended at and
whether the v_max break ended it, the standstill index, the follow mode's indices, branch and flags, v_idx and the row-5 choice). Two
evaluations took the same decisions if and only if their traces are equal. What is continuous across its switch is NOT part of the
trace: the tyre radicand's sign (the share tends to 0 on either side), min(tyre, machine), the machine table's row (np.interp is
continuous), the choice of the smaller of two speeds.

Next to vx every function returns `rad`: per output row the smallest radicand of the steps its value went through -- the step that produced it
and, through that step's start row, the steps upstream of it in the same run and in the sweep before (inf for rows that kept the limit
speed or an input: a step whose result was not taken leaves no trace in the row). A step has two radicands, both under a root: the tyre's |1 - q^e|, and its own
v'^2 / v^2 = (v^2 + 2 a el) / v^2 (next to zero where the car comes to rest: the root turns an error of v^2 into a much larger one of v').
It is the handle by which an ill-conditioned class is split (tests/test_vel_cases_host.py).
"""
import math

import numpy as np

LD = np.longdouble
MARGIN = 100.0
BOUND_FLOOR = MARGIN * float(np.finfo(np.float64).eps)
BOUND_CAP = 1e-5
FLOOR_VX, FLOOR_AX = 1.0, 0.5             # tests/helpers.py: ELEM_FLOOR_VX, ELEM_FLOOR_AX
ACCEL_FORW, DECEL_FORW, DECEL_BACKW = 0, 1, 2


class Params(object):
    """The fields of _capi.VelParamSet the operation reads, as Python floats."""

    def __init__(self, vp):
        s = vp.struct
        self.exp, self.drag, self.m_veh, self.len_veh, self.v_max = s.dyn_model_exp, s.drag_coeff, s.m_veh, s.len_veh, s.v_max
        self.axm = np.array(vp.axm, np.float64).reshape(-1, 2)
        self.ctrl, self.c_p, self.k_p, self.k_d, self.tan_w = int(s.follow_control_type), s.c_p, s.k_p, s.k_d, s.tan_w


def exp_class(exp):
    return "exp1" if exp == 1.0 else "exp2" if exp == 2.0 else "general"


def interp(x, xp, fp, T):
    """np.interp for ascending xp: constant outside, slope * (x - x0) + f0 inside."""
    n = len(xp)
    if n == 1 or x <= xp[0]:
        return T(fp[0])
    if x >= xp[n - 1]:
        return T(fp[n - 1])
    j = 0
    while j + 1 < n and xp[j + 1] <= x:
        j += 1
    x0, x1, f0, f1 = T(xp[j]), T(xp[j + 1]), T(fp[j]), T(fp[j + 1])
    return (f1 - f0) / (x1 - x0) * (x - x0) + f0


def ax_poss(v, radius, ax_max, ay_max, P, mode, T):
    """(available longitudinal acceleration, tyre radicand)."""
    e = T(P.exp)
    ay_used = v * v / radius
    ax_max = abs(ax_max) if mode != DECEL_FORW else -abs(ax_max)
    radicand = T(1) - np.power(ay_used / ay_max, e)
    tyre = ax_max * np.power(radicand, T(1) / e) if radicand > 0 else T(0)
    avail = tyre
    if mode == ACCEL_FORW:
        axm = interp(v, P.axm[:, 0], P.axm[:, 1], T)
        avail = tyre if tyre < axm else axm
    drag = -(v * v) * T(P.drag) / T(P.m_veh)
    return (avail + drag if mode != DECEL_BACKW else avail - drag), radicand


def radii_of(kappa, T):
    return [abs(T(1) / T(k)) if k != 0.0 else T(np.inf) for k in kappa]


def fb_sweep(vx, rad, radii, el, gax, gay, v_max, P, backwards, T):
    """One sweep of the forward-backward solver, in place on ``vx`` (and ``rad``). Returns (run starts, ((last step, broke at v_max), ...))."""
    n = len(vx)
    if backwards:
        rm, em = radii[::-1], el[::-1]
        vx.reverse()
        rad.reverse()
    else:
        rm, em = radii, el
    mode = DECEL_BACKW if backwards else ACCEL_FORW
    starts, prev = [], -3
    for i in range(n - 1):
        if vx[i + 1] - vx[i] > 0:
            if not starts or i - prev > 1:
                starts.append(i)
            prev = i
    ends = []
    for q, i in enumerate(starts):
        broke = 0
        while i < n - 1:
            ax_cur, r0 = ax_poss(vx[i], rm[i], gax[i], gay[i], P, mode, T)
            w_next = vx[i] * vx[i] + 2 * ax_cur * em[i]
            dep = min(rad[i], abs(float(r0)), abs(float(w_next / (vx[i] * vx[i]))) if vx[i] != 0 else np.inf)
            v_next = np.sqrt(w_next)
            if backwards:
                ax_next, r1 = ax_poss(v_next, rm[i + 1], gax[i + 1], gay[i + 1], P, mode, T)
                v_tmp = np.sqrt(vx[i] * vx[i] + 2 * ax_next * em[i])
                if v_tmp < v_next:
                    v_next, dep = v_tmp, min(dep, abs(float(r1)))
            if v_next < vx[i + 1]:
                vx[i + 1], rad[i + 1] = v_next, dep
            i += 1
            if v_next > v_max:
                broke = 1
                break
            if q + 1 < len(starts) and i >= starts[q + 1]:
                break
        ends.append((i, broke))
    if backwards:
        vx.reverse()
        rad.reverse()
    return tuple(starts), tuple(ends)


def calc_vel_profile(kappa, el, gg, v_max, v_start, v_end, P, T=LD):
    """tph.calc_vel_profile(closed=False, loc_gg=gg). ``v_end`` None: free end. Returns (vx, trace, rad)."""
    n = len(kappa)
    with np.errstate(all="ignore"):
        v_max, v_start = T(v_max), max(T(v_start), T(0))
        radii = radii_of(kappa, T)
        el = [T(x) for x in el[:n - 1]]
        gax, gay = [T(x) for x in gg[:, 0]], [T(x) for x in gg[:, 1]]
        vx = [min(np.sqrt(gay[i] * radii[i]), v_max) for i in range(n)]
        rad = [np.inf] * n
        if vx[0] > v_start:
            vx[0] = v_start
        fwd = fb_sweep(vx, rad, radii, el, gax, gay, v_max, P, False, T)
        if v_end is not None and vx[n - 1] > max(T(v_end), T(0)):
            vx[n - 1] = max(T(v_end), T(0))
        bwd = fb_sweep(vx, rad, radii, el, gax, gay, v_max, P, True, T)
    return np.array(vx, T), (fwd, bwd), np.array(rad)


def calc_vel_profile_brake(kappa, el, gg, v_start, P, T=LD):
    """tph.calc_vel_profile_brake. ``gg`` an (n, 2) array or a pair (constant limits). Returns (vx, standstill index, rad): the index is
    the first point the profile does not reach (n if it never stops)."""
    n = len(kappa)
    vx, rad, stop = [T(0)] * n, [np.inf] * n, n
    vx[0] = T(v_start)
    const = not hasattr(gg, "shape")
    with np.errstate(all="ignore"):
        for i in range(n - 1):
            radius = abs(T(1) / T(kappa[i])) if kappa[i] != 0.0 else T(np.inf)
            ax_m, ay_m = (T(gg[0]), T(gg[1])) if const else (T(gg[i, 0]), T(gg[i, 1]))
            ax, r0 = ax_poss(vx[i], radius, -ax_m, ay_m, P, DECEL_FORW, T)
            radicand = vx[i] * vx[i] + 2 * ax * T(el[i])
            if radicand < 0:
                stop = i + 1
                break
            vx[i + 1] = np.sqrt(radicand)
            rad[i + 1] = min(rad[i], abs(float(r0)), abs(float(radicand / (vx[i] * vx[i]))) if vx[i] != 0 else np.inf)
    return np.array(vx, T), stop, np.array(rad)


def first_not_above(v, thr):
    k = 0
    while k < len(v) and v[k] > thr:
        k += 1
    return k


def calc_vel_profile_follow(P, job, glob_rl, idx_s_opp, T=LD, controlled_only=False, info=None):
    """calc_vel_profile_follow for one job dict (tests/vel_jobs.py). ``glob_rl``: the lattice's race line rows (s, x, y, kappa, vel), closed
    (last row = first), ``idx_s_opp``: index of the race-line point behind the object (tests/projection_cases.py). Returns
    (vx, too_close, vel_bound, trace, rad). ``info``: a dict that receives the two differences vel_bound compares with 1.0 m/s.
    trace = (too_close, idb [ego brake profile: first v <= 0.1], the opponent's likewise, stop_idx, index of v_end on the rolled race line or
    -1, PDtan clamp, v_control clamp, branch [0: brake profile, 1: decelerate to v_control first, 2: controlled from the start], idx_c, n_decel,
    vel_bound, trace of the segment profile, trace of the free profile)."""
    kappa, el, gg = np.asarray(job["kappa"]), np.asarray(job["el_lengths"]), np.asarray(job["loc_gg"])
    n, n_el = kappa.size, el.size
    assert n_el == n
    v_start, v_max, v_obj, obj_dist = T(job["v_start"]), T(P.v_max), T(job["v_obj"]), T(job["obj_dist"])
    with np.errstate(all="ignore"):
        control_d = T(P.c_p) * T(job["safety_d"]) + T(P.len_veh)
        safety_d = T(job["safety_d"]) + T(P.len_veh)
        too_close = int(obj_dist - safety_d < 0)

        v_brake, _, rad_b = calc_vel_profile_brake(kappa, el, gg, v_start, P, T)
        idb = first_not_above(v_brake, T(0.1))
        ego_stop = T(0)
        for i in range(min(idb, n_el)):
            ego_stop += T(el[i])

        # the opponent's brake profile along the race line from its own point on; the scan wraps at the seam and ends after one lap
        G = glob_rl.shape[0] - 1
        order = [(i + idx_s_opp) % G for i in range(G)]
        r_vel0 = T(glob_rl[order[0], 4])
        v, opp_idb, opp_stop, r_len = (v_obj if v_obj < r_vel0 else r_vel0), 0, T(0), []
        for i in range(G):
            if not v > T(0.1):
                break
            j = order[i]
            r_len.append(T(glob_rl[j + 1, 0]) - T(glob_rl[j, 0]))
            opp_stop += r_len[i]
            opp_idb = i + 1
            if i == G - 1:
                break
            k = glob_rl[j, 3]
            ax, _ = ax_poss(v, abs(T(1) / T(k)) if k != 0.0 else T(np.inf), T(-14.0), T(14.0), P, DECEL_FORW, T)
            radicand = v * v + 2 * ax * r_len[i]
            v = np.sqrt(radicand) if not radicand < 0 else T(0)

        s = [T(0)]
        for i in range(1, n_el):
            s.append(s[i - 1] + T(el[i - 1]))
        s_stop = obj_dist - safety_d + opp_stop
        stop_idx = 0
        while stop_idx < n_el - 1 and s[stop_idx] < s_stop:
            stop_idx += 1
        v_end, v_end_idx = T(0), -1
        if s_stop > s[n_el - 1]:
            s_ends = opp_stop - (s_stop - s[n_el - 1])
            idx, summed = 0, T(0)
            while summed < s_ends and idx < G:
                j = order[idx]
                summed += T(glob_rl[j + 1, 0]) - T(glob_rl[j, 0])
                idx += 1
            v_end_idx = idx % G
            v_end = T(glob_rl[order[v_end_idx], 4])

        pi = T(math.pi)
        if P.ctrl == 0:
            v_control = v_obj - T(P.k_p) * (control_d - obj_dist) + T(P.k_d) * (v_obj - T(job["v_ego"]))
            clamp = 0
        else:
            a = (control_d - obj_dist) * pi / 2 * 1 / T(P.tan_w)
            lo, hi = -pi / 2 + T(1e-5), pi / 2 - T(1e-5)
            clamp = -1 if a < lo else 1 if a > hi else 0
            a = lo if a < lo else hi if a > hi else a
            v_control = v_obj - np.tan(a) * T(P.k_p) + T(P.k_d) * (v_obj - T(job["v_ego"]))
        vc_clamp = -1 if v_control < 0 else 1 if v_control > v_max else 0
        v_control = T(0) if v_control < 0 else v_max if v_control > v_max else v_control

        vel_bound, seg_trace, idx_c, n_decel, branch = 1, (), 0, 0, 0
        rad = np.full(n, np.inf)
        if ego_stop < s_stop:
            if v_start > v_control and stop_idx >= 2:
                branch = 1
                hit = [i for i in range(n) if v_brake[i] <= v_control]
                idx_c = hit[0] if hit else 0
                if info is not None:
                    info["hit"] = idx_c                 # before the two fix-ups
                if idx_c > stop_idx:
                    idx_c = stop_idx
                if idx_c == 0:
                    idx_c = stop_idx
                n_decel = min(idx_c + 1, n)
                v_cs = v_brake[n_decel - 1]
            else:
                branch = 2
                if not stop_idx >= 2:
                    vel_bound = 0
                v_cs = v_start
            prof = list(v_brake[:max(n_decel - 1, 0)])
            rad[:len(prof)] = rad_b[:len(prof)]
            if stop_idx - idx_c > 0:
                hi_ = min(stop_idx + 1, n)
                seg, seg_trace, seg_rad = calc_vel_profile(kappa[idx_c:hi_], el[idx_c:stop_idx], gg[idx_c:hi_], v_control, v_cs, v_end, P, T)
                if abs(seg[0] - v_cs) > 1:
                    vel_bound = 0
                if info is not None:
                    info["d_seg"] = float(abs(seg[0] - v_cs))
                rad[len(prof):len(prof) + len(seg)] = np.minimum(seg_rad, rad_b[idx_c])
                prof += list(seg)
            elif stop_idx - idx_c == 0:
                rad[len(prof)] = rad_b[idx_c]
                prof.append(v_cs)
            prof += [T(0)] * (n - stop_idx - 1)
            if abs(prof[0] - v_start) > 1:
                vel_bound = 0
            if info is not None:
                info["d_first"] = float(abs(prof[0] - v_start))
            assert len(prof) == n, (len(prof), n)
        else:
            prof, rad = list(v_brake), rad_b.copy()
        if controlled_only:
            vx, free_trace = np.array(prof, T), ()
        else:
            free, free_trace, free_rad = calc_vel_profile(kappa, el, gg, v_max, v_start, None, P, T)
            vx = np.array([prof[i] if prof[i] < free[i] else free[i] for i in range(n)], T)
            rad = np.array([rad[i] if prof[i] < free[i] else free_rad[i] for i in range(n)])
    trace = (too_close, idb, opp_idb, stop_idx, v_end_idx, clamp, vc_clamp, branch, idx_c, n_decel, vel_bound, seg_trace, free_trace)
    return vx, too_close, vel_bound, trace, rad


def run_job(P, job, glob_rl=None, idx_s_opp=None, T=LD, info=None):
    """One seam-(2) job dict -> (vx, too_close, vel_bound, trace, rad)."""
    mode = int(job["mode"])
    if mode == 0:
        vx, tr, rad = calc_vel_profile(job["kappa"], job["el_lengths"], np.asarray(job["loc_gg"]), P.v_max, job["v_start"], job.get("v_end"), P, T)
        return vx, 0, 1, tr, rad
    if mode == 1:
        vx, stop, rad = calc_vel_profile_brake(job["kappa"], job["el_lengths"], np.asarray(job["loc_gg"]), job["v_start"], P, T)
        return vx, 0, 1, (stop,), rad
    return calc_vel_profile_follow(P, job, glob_rl, idx_s_opp, T, info=info)


def tick_slot(P, lat, pp, action_is_follow, reduced, goal_layer, end_node, vel_plan, vel_est, gg, safety_d, v_max_offset, obj, T=LD):
    """The velocity stage of a tick on a fresh path (what tick_vel_stage and k_vel_final do) for one action slot. ``pp``: the slot's
    path_param rows (x, y, psi, kappa, element length); ``obj``: None or (x, y, v, obj_dist, idx_s_opp) of the closest object, the last two
    from the projection reference. Returns (vx, ax, too_close, vel_bound, trace, rad)."""
    n = pp.shape[0]
    kappa, el = pp[:, 3], pp[:, 4]
    ggr = np.tile(np.asarray(gg, np.float64), (n, 1))
    too_close, vel_bound, tr_f, vx_f, rad, choice, v_idx = 0, 1, (), None, np.full(n, np.inf), 0, -1
    with np.errstate(all="ignore"):
        if action_is_follow:
            job = {"kappa": kappa, "el_lengths": el, "loc_gg": ggr, "v_start": vel_plan, "v_ego": vel_est, "safety_d": safety_d,
                   "v_obj": obj[2], "obj_dist": obj[3]}
            vx_f, too_close, vel_bound, tr_f, rad = calc_vel_profile_follow(P, job, lat.glob_rl, obj[4], T)
        tr_g = ()
        if not action_is_follow or reduced:
            if reduced:
                v_end = T(0)
                spl = T(0)
                for i in range(n - 1):
                    spl += T(el[i])
                c, first = T(0), 0
                for i in range(n - 1):
                    c += T(el[i])
                    if not c < spl - T(5):
                        first = i
                        break
                v_idx = first + 1
                if v_idx == 1 and n > 1:
                    v_idx = n
            else:
                v_end = T(lat.vel_raceline[goal_layer])
                red = v_end * T(lat.vel_decrease_lat) * (T(abs(int(end_node) - int(lat.raceline_index[goal_layer]))) * T(lat.lat_offset))
                v_end = v_end - (red if red < v_end else v_end)
                v_idx = n
            vx = [T(0)] * n
            rad_g = np.full(n, np.inf)
            if v_idx > 1:
                g, tr_g, rg = calc_vel_profile(kappa[:v_idx], el[:v_idx - 1], ggr[:v_idx], P.v_max, vel_plan, v_end, P, T)
                vx[:v_idx], rad_g[:v_idx] = list(g), rg
            vel_bound = int(abs(vx[0] - T(vel_plan)) < T(v_max_offset))
            if vx_f is not None and n >= 6 and vx_f[5] < vx[5]:
                choice = 1
            else:
                choice, vx_f, rad = 2, np.array(vx, T), rad_g
        s = [T(0)]
        for i in range(1, n):
            s.append(s[i - 1] + T(el[i - 1]))
        ax = np.zeros(n, T)
        for i in range(n - 1):
            a = (vx_f[i + 1] * vx_f[i + 1] - vx_f[i] * vx_f[i]) / (2 * (s[i + 1] - s[i]))
            ax[i] = T(-5) if abs(vx_f[i]) <= 1e-8 and abs(a) <= 1e-8 else a
    return vx_f, ax, too_close, vel_bound, (v_idx, choice, vel_bound, too_close, tr_f, tr_g), rad


# ---------------------------------------------------------------- comparison and bounds

def rel_dev(got, ref, floor):
    """Largest element-wise deviation relative to max(|ref|, floor), evaluated in long double."""
    got, ref = np.asarray(got, LD), np.asarray(ref, LD)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), LD(floor))))


def round_up_one_digit(x):
    if x <= 0.0:
        return 0.0
    e = math.floor(math.log10(x))
    m = math.ceil(x / 10.0 ** e - 1e-12)
    return float("%de%d" % (m, e))              # (the literal, so that 4e-10 is the double the source text "4e-10" gives)


def bound_of(worst):
    """100 x the worst fp64-vs-long-double deviation of the reference, rounded up to one digit, within [100 eps, 1e-5]."""
    return min(max(round_up_one_digit(MARGIN * worst), BOUND_FLOOR), BOUND_CAP)


# ---------------------------------------------------------------- a whole tick batch

class SlotRef(object):
    """Reference of one valid action slot: vx, ax (number type T), too_close, vel_bound, trace, rad."""

    def __init__(self, out):
        self.vx, self.ax, self.too_close, self.vel_bound, self.trace, self.rad = out


def tick_objects(lat, batch, vel, res):
    """{(s, a): (x, y, v, obj_dist, idx_s_opp)} of every valid follow slot: the closest object's prediction head, its speed, its distance
    along the slot's path (s of the object minus s of the ego position estimate on the path's polyline, s = [0, cumsum(el)]) and the
    race-line point behind it -- all through the projection reference tests/projection_cases.py (fp64, as the product computes them:
    projections have their own boundary tests). Without an object: the ego position at distance 0 and speed 0."""
    from projection_cases import Line, restate
    G = lat.glob_rl.shape[0] - 1
    rl = Line("raceline", lat.glob_rl[:G, 1], lat.glob_rl[:G, 2], lat.glob_rl[:G, 0], True)
    out = {}
    for s, a in zip(*np.nonzero((res.valid == 1) & (res.action_id == 1))):
        n = int(res.n_pts[s, a])
        pp = res.path_param[s, a, :n]
        ci, v0 = int(res.closest_obj_index[s]), int(batch.veh_off[s])
        ex, ey = float(vel.pos_x[s]), float(vel.pos_y[s])
        if ci < 0 or ci >= int(batch.veh_off[s + 1]) - v0:
            ox, oy, ov, dist = ex, ey, 0.0, 0.0
        else:
            q = int(batch.pos_off[v0 + ci])
            ox, oy, ov = float(batch.pos_x[q]), float(batch.pos_y[q]), float(vel.veh_vel[v0 + ci])
            scum = np.concatenate(([0.0], np.cumsum(pp[:, 4])))[:n]
            r = restate(Line("path", pp[:, 0], pp[:, 1], scum, False), [ox, ex], [oy, ey])
            dist = float(r.s[0] - r.s[1])
        out[int(s), int(a)] = (ox, oy, ov, dist, int(restate(rl, [ox], [oy]).pair[0, 0]))
    return out


def tick_batch_ref(lat, batch, vel, res, T=LD, objects=None, slots=None):
    """{(s, a): SlotRef} of the valid slots of a tick batch, on the path_param columns of ``res`` (the oracle's result or the device's)."""
    P = Params(vel.params)
    t = vel.struct
    objects = tick_objects(lat, batch, vel, res) if objects is None else objects
    out = {}
    for s, a in (zip(*np.nonzero(res.valid == 1)) if slots is None else slots):
        s, a = int(s), int(a)
        n = int(res.n_pts[s, a])
        follow = int(res.action_id[s, a]) == 1
        out[s, a] = SlotRef(tick_slot(P, lat, res.path_param[s, a, :n], follow, bool(res.reduced[s, a]), int(res.goal_layer[s, a]),
                                      int(res.nodes[s, a, int(res.n_nodes[s, a]) - 1]), float(vel.vel_plan[s]), float(vel.vel_est[s]),
                                      (t.gg_ax, t.gg_ay), t.safety_d, t.v_max_offset, objects.get((s, a)), T))
    return out
