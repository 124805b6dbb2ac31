"""
Closed-loop simulation of the example driver (``main_std_example.py:98-135``) for the fleet's device loop (``ltpl_fleet_sim_*``,
include/ltpl_hip.h; csrc/fleet_sim.hpp): the race-line table the opponents drive on and scalar host mirrors of the two simulators the
driver runs around the planner on every tick --

  ``opponent_step``  one ``ObjectlistDummy.get_objectlist`` call (graph_ltpl/testing_tools/src/objectlist_dummy.py:148-170): the
                     opponent's arc length integrated in 1 ms steps over the time since its last call, then position, heading and speed
                     interpolated on the race line;
  ``vdc_step``       one ``vdc_dummy`` call (graph_ltpl/testing_tools/src/vdc_dummy.py:5-58): the ideal tracker that moves the ego
                     along its last trajectory for one tick.

and of the races of ``ltpl_fleet_sim_race`` (planners of one fleet that see one another) --

  ``vdc_track``      ``vdc_step`` that also returns the final arc length and segment of the tracker;
  ``peer_heading``   the heading of the tracked pose: psi of the same trajectory at that arc length and segment, across the +-pi wrap;
  ``race_objects``   the object dicts the mates of one planner contribute to its object list.

and of the race telemetry of ``ltpl_fleet_sim_telemetry`` (a record per planner, accumulated on the device) --

  ``Telemetry``      the rules of include/ltpl_hip.h in the operation order of k_fleet_sim_tele / k_fleet_sim_rank.

Both simulators restate ``np.interp`` (numpy's ``arr_interp``) in the operation order of the device functions (``interp_at`` here,
``fleet::sim_interp`` there), so that host and device give the same bits as the reference.
"""
import bisect
import math

import numpy as np

from .offline_build import _closed_line_heading

OPP_DT = 0.001        # integration step of both simulators (objectlist_dummy.py:149, vdc_dummy.py:46)
VDC_MIN_STEP = 0.0001  # vdc_dummy.py:49


def interp_at(x, xp, fp, j):
    """``np.interp(x, xp, fp)`` for a scalar ``x`` once the segment is known: ``j`` = the largest index with ``xp[j] <= x`` (-1 below
    ``xp[0]``, ``len(xp)`` above ``xp[-1]``). numpy's arr_interp: clamps at both ends, ``fp[j]`` on a knot, slope times offset plus
    ``fp[j]`` inside a segment, and the same from the right end of the segment when that gives NaN."""
    n = len(xp)
    if j < 0:
        return float(fp[0])
    if j >= n - 1:
        return float(fp[n - 1])
    if xp[j] == x:
        return float(fp[j])
    slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])
    r = slope * (x - xp[j]) + fp[j]
    if math.isnan(r):
        r = slope * (x - xp[j + 1]) + fp[j + 1]
        if math.isnan(r) and fp[j] == fp[j + 1]:
            r = fp[j]
    return float(r)


def segment(x, xp):
    """Segment index of ``interp_at`` (``xp`` a Python list, non-decreasing)."""
    if x < xp[0]:
        return -1
    if x > xp[-1]:
        return len(xp)
    return bisect.bisect_right(xp, x) - 1


def interp(x, xp, fp):
    """``np.interp`` for a scalar (``xp`` / ``fp`` Python lists)."""
    if math.isnan(x):
        return x
    return interp_at(x, xp, fp, segment(x, xp))


class RaceLineTable(object):
    """The race line an ``ObjectlistDummy`` drives on (objectlist_dummy.py:112-127): ``refline + normvec * alpha``, ``s_rl =
    cumsum(length_rl)`` (it does NOT start at 0), the heading of ``calc_head_curv_num(is_closed=True)`` shifted into [0, 2 pi) and the
    race-line speed. ``rows()`` is the [n, 5] table [s_rl, x, y, psi, vel_rl] of ``ltpl_fleet_sim_in``."""

    def __init__(self, s_rl, x, y, psi, vel_rl):
        self.s_rl, self.x, self.y, self.psi, self.vel_rl = (np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in
                                                            (s_rl, x, y, psi, vel_rl))

    @classmethod
    def from_track(cls, track):
        """``track``: mapping with refline [n, 2], normvec [n, 2], alpha, length_rl, vel_rl (the track npz / the reference's csv)."""
        refline = np.asarray(track['refline'], dtype=float)
        normvec = np.asarray(track['normvec'], dtype=float)
        alpha = np.asarray(track['alpha'], dtype=float)
        length_rl = np.asarray(track['length_rl'], dtype=float)
        raceline = refline + normvec * alpha[:, np.newaxis]
        psi = _closed_line_heading(raceline, length_rl)
        psi = np.where(psi < 0.0, psi + np.pi * 2, psi)
        return cls(np.cumsum(length_rl), raceline[:, 0], raceline[:, 1], psi, np.asarray(track['vel_rl'], dtype=float))

    def rows(self):
        return np.ascontiguousarray(np.column_stack((self.s_rl, self.x, self.y, self.psi, self.vel_rl)))

    def lists(self):
        return [a.tolist() for a in (self.s_rl, self.x, self.y, self.psi, self.vel_rl)]


def opponent_step(tab, s, tic, now, vel_scale, lists=None):
    """One ``ObjectlistDummy.get_objectlist`` call at clock value ``now``: returns (s, tic, x, y, psi, v). ``lists``: ``tab.lists()``
    (pass it in a loop: the conversion is the expensive part)."""
    s_rl, xs, ys, psis, vel = lists if lists is not None else tab.lists()
    vel_s = [v * vel_scale for v in vel]              # the scaled table is formed first (objectlist_dummy.py:121)
    toc = now - tic
    tic = now
    t = 0.0
    while t < toc:
        s += interp(s, s_rl, vel_s) * OPP_DT
        t += OPP_DT
        if s >= s_rl[-1]:
            s = 0.0
    j = segment(s, s_rl)
    x, y = interp_at(s, s_rl, xs, j), interp_at(s, s_rl, ys, j)
    psi = interp_at(s, s_rl, psis, j)
    if psi > np.pi:
        psi -= 2 * np.pi
    return s, tic, x, y, psi, interp_at(s, s_rl, vel_s, j)


def vdc_step(pos_est, traj, iter_time):
    """One ``vdc_dummy`` call: ``traj`` = the exported trajectory (rows [s, x, y, psi, kappa, vx, ax], already trimmed to the exported
    rows). Returns (pos_out [x, y], vel_est). Exact ties of the two-nearest search take the lower index (numpy leaves their order
    open)."""
    pos, vel, _, _ = vdc_track(pos_est, traj, iter_time)
    return pos, vel


def vdc_track(pos_est, traj, iter_time):
    """``vdc_step`` returning (pos_out [x, y], vel_est, s, j): the tracker's final arc length and its segment (``segment``), both None
    where the pose stays (at most 2 rows)."""
    traj = np.asarray(traj, dtype=float)
    sc, px, py, vx = (traj[:, c].tolist() for c in (0, 1, 2, 5))
    n = len(sc)
    if n <= 2:
        return [float(pos_est[0]), float(pos_est[1])], float(vx[0]), None, None
    ex, ey = float(pos_est[0]), float(pos_est[1])
    d2 = [(px[i] - ex) * (px[i] - ex) + (py[i] - ey) * (py[i] - ey) for i in range(n)]
    i1 = min(range(n), key=lambda i: (d2[i], i))
    i2 = min((i for i in range(n) if i != i1), key=lambda i: (d2[i], i))
    i = min(i1, i2)
    s = math.sqrt(d2[i]) + sc[i]
    t = 0.0
    while t < iter_time:
        s += max(interp(s, sc, vx) * OPP_DT, VDC_MIN_STEP)
        t += OPP_DT
    j = segment(s, sc)
    return [interp_at(s, sc, px, j), interp_at(s, sc, py, j)], interp_at(s, sc, vx, j), s, j


def peer_heading(s, j, ts, psi):
    """Heading at arc length ``s`` on segment ``j`` of a trajectory (``ts``: its s column, ``psi``: its heading column; ``vdc_track``'s
    s and j): clamped like np.interp, the step between two rows taken the short way round the circle, the result wrapped into
    (-pi, pi]. The operation order of the device (fleet::sim_heading)."""
    n = len(ts)
    if j < 0:
        return float(psi[0])
    if j >= n - 1:
        return float(psi[n - 1])
    if ts[j + 1] == ts[j]:
        return float(psi[j])
    d = float(psi[j + 1]) - float(psi[j])
    if d > math.pi:
        d -= 2 * math.pi
    elif d < -math.pi:
        d += 2 * math.pi
    theta = float(psi[j]) + d * ((s - float(ts[j])) / (float(ts[j + 1]) - float(ts[j])))
    if theta > math.pi:
        theta -= 2 * math.pi
    elif theta <= -math.pi:
        theta += 2 * math.pi
    return theta


def race_objects(p, race, pos, vel, theta, length, id0=100):
    """The objects planner ``p`` sees of its mates: every other planner of ``race`` (its planner indices, ascending) as a 'physical'
    object at its tracked pose ``pos[q]`` [x, y], speed ``vel[q]``, heading ``theta[q]`` and ``length[q]`` (id ``id0 + q``), in list
    order. They follow the planner's opponents and static objects."""
    return [{'X': float(pos[q][0]), 'Y': float(pos[q][1]), 'theta': float(theta[q]), 'type': 'physical', 'id': id0 + int(q),
             'length': float(length[q]), 'v': float(vel[q])} for q in sorted(race) if q != p]


# name, first index, doubles, integer valued: the record of ltpl_fleet_sim_telemetry (LTPL_FLEET_SIM_TELE_DOUBLES = 22 per planner)
TELEMETRY_FIELDS = (("ticks", 0, 1, True), ("s", 1, 1, False), ("dist", 2, 1, False), ("laps", 3, 1, True), ("t_cross", 4, 1, False),
                    ("lap_last", 5, 1, False), ("lap_best", 6, 1, False), ("vel_sum", 7, 1, False), ("vel_max", 8, 1, False),
                    ("act", 9, 5, True), ("clear_min", 14, 1, False), ("clear_tick", 15, 1, True), ("clear_slot", 16, 1, True),
                    ("contact_ticks", 17, 1, True), ("rank", 18, 1, True), ("passes", 19, 1, True), ("passed", 20, 1, True),
                    ("gap_ahead", 21, 1, False))
TELEMETRY_DOUBLES = 22
_ACT_INDEX = {"straight": 0, "follow": 1, "left": 2, "right": 3, "emergency": 4}


def closed_length(raceline, s_raceline):
    """Closed length of a race line (one point per layer): ``s_raceline[-1]`` plus the distance from the last point back to the first."""
    dx, dy = float(raceline[0][0]) - float(raceline[-1][0]), float(raceline[0][1]) - float(raceline[-1][1])
    return float(s_raceline[-1]) + math.sqrt(dx * dx + dy * dy)


def telemetry_dict(rows, track_length=None):
    """[n, 22] records as a dict of named arrays (integer valued fields as int64, ``act`` as [n, 5])."""
    rows = np.asarray(rows, np.float64).reshape(-1, TELEMETRY_DOUBLES)
    out = {}
    for name, i, cnt, is_int in TELEMETRY_FIELDS:
        a = rows[:, i] if cnt == 1 else rows[:, i:i + cnt]
        out[name] = a.astype(np.int64) if is_int else a.copy()
    if track_length is not None:
        out["track_length"] = float(track_length)
    return out


class Telemetry(object):
    """Host mirror of the fleet's race telemetry (ltpl_fleet_sim_telemetry; k_fleet_sim_tele / k_fleet_sim_rank in csrc/fleet_sim.hpp): the
    rules of include/ltpl_hip.h in the same order of fp64 operations. ``races``: sizes summing to ``n`` (or ranges of consecutive planners);
    ``radius`` / ``grid_s``: scalars or one value per planner (``grid_s`` None: s of the first live tick); ``s_of``: any callable
    pos -> s on the race line; ``track_length``: its closed length (``closed_length``)."""

    def __init__(self, n, races, radius, track_length, s_of, dt, grid_s=None):
        self.n, self.L, self.s_of, self.dt = int(n), float(track_length), s_of, float(dt)
        sizes = [len(r) if isinstance(r, range) else int(r) for r in races]
        if sum(sizes) != self.n:
            raise ValueError("Telemetry: the races must cover the planners")
        self.lo, self.hi = [0] * self.n, [0] * self.n
        a = 0
        for sz in sizes:
            for p in range(a, a + sz):
                self.lo[p], self.hi[p] = a, a + sz
            a += sz
        self.radius = [float(v) for v in np.broadcast_to(np.asarray(radius, np.float64), (self.n,))]
        self.grid = [float("nan")] * self.n if grid_s is None else [float(v) for v in np.broadcast_to(np.asarray(grid_s, np.float64), (self.n,))]
        self.prog = [-math.inf] * self.n
        r = np.zeros((self.n, TELEMETRY_DOUBLES), np.float64)
        r[:, [1, 4, 5, 6, 21]] = np.nan
        r[:, 8], r[:, 14], r[:, 15], r[:, 16] = -np.inf, np.inf, -1.0, -1.0
        self.rec = r

    def update(self, tick_index, recs):
        """One fleet tick: ``recs`` = one dict per planner with ``live``, ``sel`` (action name or id), ``now``, ``pos``, ``vel`` and
        ``objects`` = [(x, y, radius), ...] in list order (a planner that is not live needs ``live`` only)."""
        L, rec = self.L, self.rec
        for p, d in enumerate(recs):
            if not d["live"]:
                continue
            r = rec[p]
            px, py = float(d["pos"][0]), float(d["pos"][1])
            s = float(self.s_of((px, py)))
            cd, ci = math.inf, -1
            for k, (ox, oy, orad) in enumerate(d["objects"]):
                dx, dy = float(ox) - px, float(oy) - py
                c = math.sqrt(dx * dx + dy * dy) - float(orad)
                if c < cd:
                    cd, ci = c, k
            delta, fwd, bwd = 0.0, False, False
            if r[0] == 0.0:
                if math.isnan(self.grid[p]):
                    self.grid[p] = s
            else:
                delta = s - float(r[1])
                if delta < -(L / 2):
                    delta, fwd = delta + L, True
                elif delta > L / 2:
                    delta, bwd = delta - L, True
            r[0] += 1.0
            r[1] = s
            r[2] += delta
            now, vel = float(d["now"]), float(d["vel"])
            if fwd:
                r[3] += 1.0
                tc = now - self.dt * (s / delta) if delta > 0.0 else now
                prev = float(r[4])
                r[4] = tc
                if not math.isnan(prev):
                    lap = tc - prev
                    r[5] = lap
                    if math.isnan(r[6]) or lap < r[6]:
                        r[6] = lap
            if bwd:
                r[3] -= 1.0
            r[7] += vel
            if vel > r[8]:
                r[8] = vel
            sel = d["sel"]
            sel = _ACT_INDEX.get(sel, -1) if isinstance(sel, str) else int(sel)
            if 0 <= sel <= 4:
                r[9 + sel] += 1.0
            if len(d["objects"]) > 0:
                if cd < r[14]:
                    r[14], r[15], r[16] = cd, float(tick_index), float(ci)
                if cd < self.radius[p]:
                    r[17] += 1.0
            self.prog[p] = self.grid[p] + float(r[2])
            if self.hi[p] - self.lo[p] < 2:
                r[18] = 1.0
        for p, d in enumerate(recs):                      # every planner's progress of the tick is known: rank and gap
            lo, hi = self.lo[p], self.hi[p]
            if hi - lo < 2 or not d["live"]:
                continue
            r, mine = rec[p], self.prog[p]
            ahead, gap = 0, math.inf
            for q in range(lo, hi):
                if q != p and (self.prog[q] > mine or (self.prog[q] == mine and q < p)):
                    ahead += 1
                    g = self.prog[q] - mine
                    if g < gap:
                        gap = g
            rank, prev = float(1 + ahead), float(r[18])
            if r[0] > 1.0:
                if rank < prev:
                    r[19] += prev - rank
                elif rank > prev:
                    r[20] += rank - prev
            r[18] = rank
            r[21] = gap if ahead else float("nan")

    def rows(self):
        return self.rec.copy()

    def as_dict(self):
        return telemetry_dict(self.rec, self.L)
