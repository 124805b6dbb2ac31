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

and of the seeded sensor noise of ``ltpl_fleet_sim_noise`` (csrc/fleet_noise.hpp) --

  ``philox4x32``     Philox4x32-10, scalars or arrays;
  ``noise_gauss``    the noise sample g(seed, tick, obj, comp): integer arithmetic and exact fp64 steps, so the device's bits;
  ``NoiseModel``     what a planner perceives of itself, of its objects and of its mates, in the operation order of the kernels.

and of the vehicle model of ``ltpl_fleet_sim_vehicle`` (csrc/fleet_vehicle.hpp) --

  ``VehicleModel``   a kinematic single-track car with actuator lags, a friction circle and a pure-pursuit / speed controller in place
                     of the ideal tracker: + - * / sqrt on Python floats in the operation order of the kernels, so the device's bits;
  ``VEHICLE_DEFAULTS`` / ``VEHICLE_FIELDS`` / ``vehicle_dict``   its parameters and the record of ``Fleet.sim_vehicle_read``.

and of the sensor model of ``ltpl_fleet_sim_sensor`` (csrc/fleet_sensor.hpp) --

  ``SensorModel``    which on-track objects a planner is shown (range, cone, near field, occlusion, dropout) and the statistics record,
                     in the operation order of the header and of k_fleet_sim_sense, so the device's decisions;
  ``sensor_uniform`` / ``sensor_fov_cos`` / ``SENSOR_FIELDS`` / ``sensor_dict``   the dropout draw, the cone's cosine and the record.

and of the object tracker of ``ltpl_fleet_sim_tracker`` (csrc/fleet_track.hpp) --

  ``TrackerModel``   one planner's track table with memory from tick to tick: predict, greedy nearest-neighbour association, update,
                     coasting, births and the list handed on, in the operation order of the header, so the device's bits;
  ``TRACKER_FIELDS`` / ``TRACK_FIELDS`` / ``TRACKER_DEFAULTS`` / ``tracker_dict``   the statistics record, a table row and the defaults.

and of the prediction model of ``ltpl_fleet_sim_predictor`` (csrc/fleet_predict.hpp) --

  ``PredictorModel``   K predicted points per object in place of the ingestion's one: as ingested, straight line, or along the race line
                       at the object's lateral offset, in the operation order of the header, so the device's bits;
  ``PREDICTOR_FIELDS`` / ``PREDICTOR_DEFAULTS`` / ``predictor_dict``   the statistics record and the defaults.

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


def fields_dict(rows, fields, doubles=None, wide=(), nan_int=None):
    """Records [..., doubles] as a dict of named arrays in the order of a ``*_FIELDS`` table -- (name, first index, integer valued), or
    (name, first index, doubles, integer valued): integer valued fields as int64 (a NaN reads ``nan_int`` there, if given), the others
    as copies. ``doubles``: the records are reshaped to [-1, doubles]; ``wide`` = ((name, doubles), ...): array-valued fields of a
    three-column table."""
    rows = np.asarray(rows, np.float64) if doubles is None else np.asarray(rows, np.float64).reshape(-1, doubles)
    out = {}
    for name, i, cnt, is_int in ((f[0], f[1], f[2] if len(f) == 4 else dict(wide).get(f[0], 1), f[-1]) for f in fields):
        a = rows[..., i] if cnt == 1 else rows[..., i:i + cnt]
        out[name] = (a if nan_int is None else np.where(np.isnan(a), nan_int, a)).astype(np.int64) if is_int else a.copy()
    return out


def telemetry_dict(rows, track_length=None):
    """[n, 22] records as a dict of named arrays (integer valued fields as int64, ``act`` as [n, 5])."""
    out = fields_dict(rows, TELEMETRY_FIELDS, TELEMETRY_DOUBLES)
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


# ---- scripted events (ltpl_fleet_sim_events, include/ltpl_hip.h; csrc/fleet_events.hpp) ---------------------------------------------
WHEN_KINDS = {"tick": 0, "opp_within": 1, "vel_below": 2, "vel_above": 3, "after": 4}                       # LTPL_SIM_WHEN_*
SET_KINDS = {"opp_vel_scale": 0, "opp_length": 1, "static_x": 2, "static_y": 3, "static_theta": 4, "static_v": 5, "static_length": 6,
             "pref": 7, "vel_max": 8, "gg_scale": 9, "gg_ax": 10, "gg_ay": 11, "safety_d": 12, "incl_emerg": 13,
             "friction_scale": 14}                                                                             # LTPL_SIM_SET_*
SET_INDEXED = ("opp_vel_scale", "opp_length", "static_x", "static_y", "static_theta", "static_v", "static_length", "pref")
MAX_TRIGGERS = 16                                                                                            # LTPL_FLEET_SIM_MAX_TRIGGERS
_ACT_IDS = {"straight": 0, "follow": 1, "left": 2, "right": 3, "emergency": 4}
_ACT_NAMES = {v: k for k, v in _ACT_IDS.items()}


class Event(object):
    """One scripted event of planner ``planner``: a condition and one write into the planner's configuration; it fires at most once.
    ``when``: ("tick", k) | ("opp_within", opponent, distance) | ("vel_below", v) | ("vel_above", v) | ("after", j, delay) with j = the
    place of an EARLIER state-conditioned event in this planner's own list (the events of the planner in the order given).
    ``set``: (kind, index, value) for "opp_vel_scale", "opp_length", "static_x" / "_y" / "_theta" / "_v" / "_length" and "pref" (value:
    an action name or id); (kind, value) for "vel_max", "gg_scale", "gg_ax", "gg_ay", "safety_d", "incl_emerg" (timed only) and
    "friction_scale"."""

    def __init__(self, planner, when, set):
        self.planner, self.when, self.set = int(planner), tuple(when), tuple(set)
        wk = self.when[0]
        if wk not in WHEN_KINDS or len(self.when) != (2 if wk in ("tick", "vel_below", "vel_above") else 3):
            raise ValueError("Event: when=%r" % (when,))
        sk = self.set[0]
        if sk not in SET_KINDS or len(self.set) != (3 if sk in SET_INDEXED else 2):
            raise ValueError("Event: set=%r" % (set,))
        self.when_kind, self.set_kind = WHEN_KINDS[wk], SET_KINDS[sk]
        self.when_index = int(self.when[1]) if wk in ("tick", "opp_within", "after") else 0
        self.when_value = 0.0 if wk == "tick" else float(self.when[-1])
        self.set_index = int(self.set[1]) if sk in SET_INDEXED else 0
        v = self.set[-1]
        self.set_value = float(_ACT_IDS[v]) if isinstance(v, str) else float(v)

    def write(self):
        """The write as (kind name, index, value); the value of "pref" as an action name, of "incl_emerg" as a bool."""
        sk, v = self.set[0], self.set_value
        return sk, self.set_index, (_ACT_NAMES.get(int(v), int(v)) if sk == "pref" else bool(v) if sk == "incl_emerg" else v)

    def __repr__(self):
        return "Event(%d, when=%r, set=%r)" % (self.planner, self.when, self.set)


def pack_events(events, n):
    """The arrays of ``ltpl_fleet_sim_events_in`` for a list of ``Event``: dict of ev_off [n + 1], when_kind, when_index, when_value,
    set_kind, set_index, set_value and ``order``: order[e] = the place in ``events`` of packed event e (planner by planner, each
    planner's events in the order given)."""
    events = list(events)
    for e in events:
        if not 0 <= e.planner < n:
            raise ValueError("event of planner %d: the fleet has %d planners" % (e.planner, n))
    order = sorted(range(len(events)), key=lambda i: (events[i].planner, i))
    cnt = np.bincount([e.planner for e in events], minlength=n) if events else np.zeros(n, np.int64)
    ev = [events[i] for i in order]

    def col(name, dt):
        a = np.array([getattr(e, name) for e in ev], dt)
        return np.ascontiguousarray(a if a.size else np.zeros(1, dt))
    return dict(ev_off=np.ascontiguousarray(np.concatenate(([0], np.cumsum(cnt))).astype(np.int32)),
                when_kind=col("when_kind", np.int32), when_index=col("when_index", np.int32), when_value=col("when_value", np.float64),
                set_kind=col("set_kind", np.int32), set_index=col("set_index", np.int32), set_value=col("set_value", np.float64),
                order=np.asarray(order, np.int64))


class EventScript(object):
    """Host mirror of the scripted events (k_fleet_sim_events_timed / k_fleet_sim_triggers, csrc/fleet_events.hpp) in the same
    operation order. ``events``: the list given to ``Fleet.sim_events``; ``n``: planners; ``race``: the ``RaceLineTable`` of the simulation
    (needed by "opp_within" only). ``fired_tick[i]``: schedule tick in which ``events[i]`` fired, -1: not yet; ``tick``: the schedule tick."""

    def __init__(self, events, n, race=None):
        self.events, self.n = list(events), int(n)
        packed = pack_events(self.events, self.n)              # (the range checks that need no simulation)
        self.lists = race.lists() if race is not None else None
        self.fired_tick = np.full(len(self.events), -1, np.int64)
        self.tick = 0
        self.own = [[] for _ in range(self.n)]                 # the planner's events in list order
        for i in packed["order"]:
            self.own[self.events[i].planner].append(int(i))
        for p, own in enumerate(self.own):
            trig = [i for i in own if self.events[i].when[0] != "tick"]
            if len(trig) > MAX_TRIGGERS:
                raise ValueError("planner %d: more than %d triggers" % (p, MAX_TRIGGERS))
            for j, i in enumerate(own):
                e = self.events[i]
                if e.when[0] == "after":
                    if not 0 <= e.when_index < j or self.events[own[e.when_index]].when[0] == "tick":
                        raise ValueError("planner %d event %d: 'after' refers to an earlier state-conditioned event of the planner" % (p, j))
                    if e.when_value < 1 or e.when_value != int(e.when_value):
                        raise ValueError("planner %d event %d: a delay must be integral and at least 1" % (p, j))
                if e.set[0] == "incl_emerg" and e.when[0] != "tick":
                    raise ValueError("planner %d event %d: incl_emerg is timed only" % (p, j))
        self.timed = {}
        for i in packed["order"]:
            if self.events[i].when[0] == "tick":
                self.timed.setdefault(self.events[i].when_index, []).append(int(i))

    def before_tick(self, state):
        """The events that fire in front of the next tick, [(place in ``events``, planner, (kind, index, value))] in the order of
        application: the timed events of the schedule tick, then per planner its triggers in list order. ``state``: what the tick before
        left (before the first tick: the setup) -- ``pos`` [n][2], ``vel`` [n], ``opp_s`` [n][opponents] (or flat with ``opp_off``
        [n + 1]), ``failed`` [n] (error flags; default none). A failed planner fires nothing. Advances the schedule tick."""
        k = self.tick
        pos, vel, failed = state["pos"], state["vel"], state.get("failed")
        off = state.get("opp_off")
        out = []

        def is_failed(p):
            return failed is not None and bool(failed[p])
        for i in self.timed.get(k, ()):
            e = self.events[i]
            if not is_failed(e.planner):
                self.fired_tick[i] = k
                out.append((i, e.planner, e.write()))
        for p in range(self.n):
            if is_failed(p):
                continue
            for i in self.own[p]:
                e = self.events[i]
                wk = e.when[0]
                if wk == "tick" or self.fired_tick[i] >= 0:
                    continue
                v = e.when_value
                if wk == "opp_within":
                    s = float(state["opp_s"][off[p] + e.when_index] if off is not None else state["opp_s"][p][e.when_index])
                    s_rl, xs, ys = self.lists[0], self.lists[1], self.lists[2]
                    dx = interp(s, s_rl, xs) - float(pos[p][0])
                    dy = interp(s, s_rl, ys) - float(pos[p][1])
                    fire = dx * dx + dy * dy <= v * v
                elif wk == "vel_below":
                    fire = float(vel[p]) < v
                elif wk == "vel_above":
                    fire = float(vel[p]) > v
                else:
                    t0 = self.fired_tick[self.own[p][e.when_index]]
                    fire = t0 >= 0 and k == t0 + int(v)
                if fire:
                    self.fired_tick[i] = k
                    out.append((i, p, e.write()))
        self.tick += 1
        return out

    def opp_dist2(self, state, p, q):
        """dx dx + dy dy of planner ``p`` to its opponent ``q`` as the "opp_within" condition forms it."""
        off = state.get("opp_off")
        s = float(state["opp_s"][off[p] + q] if off is not None else state["opp_s"][p][q])
        dx = interp(s, self.lists[0], self.lists[1]) - float(state["pos"][p][0])
        dy = interp(s, self.lists[0], self.lists[2]) - float(state["pos"][p][1])
        return dx * dx + dy * dy


# ---- seeded sensor noise (ltpl_fleet_sim_noise, include/ltpl_hip.h; csrc/fleet_noise.hpp) ------------------------------------------------
NOISE_EGO = 0xFFFFFFFF          # obj of the ego estimate
NOISE_MATE = 0x80000000         # obj of mate q of a race: NOISE_MATE | (q - first planner of the race)
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(counter, key):
    """Philox4x32-10: ``counter`` 4 words, ``key`` 2 words (ints or arrays that broadcast) -> tuple of 4 output words (uint32)."""
    c = [np.asarray(v, np.uint64) & _M32 for v in counter]
    k0, k1 = (np.asarray(v, np.uint64) & _M32 for v in key)
    m0, m1, w0, w1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                      # (32 x 32 bits: no overflow of the uint64)
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _M32, (p0 >> _S32) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return tuple(np.asarray(v).astype(np.uint32) for v in c)


def noise_words(seed, tick, obj, comp):
    """[..., 12] uint32: the output words of the three blocks (tick, obj, 3 comp + b, 0), b = 0, 1, 2, under the key (seed low, seed high)."""
    seed = np.asarray(seed, np.uint64)
    comp = np.asarray(comp, np.uint64)
    out = []
    for b in range(3):
        out += philox4x32((tick, obj, np.uint64(3) * comp + np.uint64(b), 0), (seed & _M32, seed >> _S32))
    return np.stack(np.broadcast_arrays(*out), axis=-1)


def noise_gauss(seed, tick, obj, comp):
    """g(seed, tick, obj, comp): the sum K of the 12 words, ((double)K + 6.0) 2^-32 - 6.0 -- twelve uniforms minus six. Every step is exact
    in fp64. Scalars give a float, arrays an array."""
    k = noise_words(seed, tick, obj, comp).astype(np.uint64).sum(axis=-1, dtype=np.uint64)
    g = (k.astype(np.float64) + 6.0) * 2.0 ** -32 - 6.0
    return float(g) if g.ndim == 0 else g


class NoiseModel(object):
    """Host mirror of the sensor noise of k_fleet_sim_step_noise / k_fleet_sim_mates_noise: ``value + sigma * g`` (one multiply, one add), a
    sigma of 0 draws nothing and hands the value through, speeds clamped at 0. ``seed`` and the sigmas: scalars or one per planner;
    ``races``: sizes summing to ``n`` (default: every planner alone)."""

    def __init__(self, n, seed, pos=0.0, vel=0.0, obj_pos=0.0, obj_theta=0.0, obj_vel=0.0, races=None):
        self.n = int(n)
        self.seed = [int(v) for v in np.broadcast_to(np.asarray(seed, np.uint64), (self.n,))]

        def per(v):
            return [float(x) for x in np.broadcast_to(np.asarray(v, np.float64), (self.n,))]
        self.pos, self.vel, self.obj_pos, self.obj_theta, self.obj_vel = per(pos), per(vel), per(obj_pos), per(obj_theta), per(obj_vel)
        sizes = [1] * self.n if races is None else [len(r) if isinstance(r, range) else int(r) for r in races]
        if sum(sizes) != self.n:
            raise ValueError("NoiseModel: the races must cover the planners")
        self.lo, self.hi = [0] * self.n, [0] * self.n
        a = 0
        for sz in sizes:
            for p in range(a, a + sz):
                self.lo[p], self.hi[p] = a, a + sz
            a += sz

    def _add(self, v, sigma, p, tick, obj, comp, speed=False):
        if sigma == 0.0:
            return float(v)
        w = float(v) + sigma * noise_gauss(self.seed[p], tick, obj, comp)
        return (w if w > 0.0 else 0.0) if speed else w

    def ego(self, p, tick, pos, vel):
        """([est_x, est_y], est_v) of planner ``p`` at noise tick ``tick`` from its true ``pos`` / ``vel``."""
        return ([self._add(pos[0], self.pos[p], p, tick, NOISE_EGO, 0), self._add(pos[1], self.pos[p], p, tick, NOISE_EGO, 1)],
                self._add(vel, self.vel[p], p, tick, NOISE_EGO, 2, speed=True))

    def _rows(self, p, tick, rows, objs):
        return [(self._add(r[0], self.obj_pos[p], p, tick, o, 0), self._add(r[1], self.obj_pos[p], p, tick, o, 1),
                 self._add(r[2], self.obj_theta[p], p, tick, o, 2), self._add(r[3], self.obj_vel[p], p, tick, o, 3, speed=True)) + tuple(r[4:])
                for r, o in zip(rows, objs)]

    def objects(self, p, tick, rows):
        """``rows`` [(x, y, theta, v, length)]: the planner's own object list (opponents, then statics) -> the rows as perceived."""
        return self._rows(p, tick, rows, range(len(rows)))

    def mates(self, p, tick, rows):
        """``rows``: every other planner of ``p``'s race, ascending -> the rows as ``p`` perceives them."""
        objs = [NOISE_MATE | (q - self.lo[p]) for q in range(self.lo[p], self.hi[p]) if q != p]
        if len(objs) != len(rows):
            raise ValueError("NoiseModel.mates: one row per mate expected")
        return self._rows(p, tick, rows, objs)


# ---- vehicle model (ltpl_fleet_sim_vehicle, include/ltpl_hip.h; csrc/fleet_vehicle.hpp) ---------------------------------------------------
# name, index, integer valued: the record of ltpl_fleet_sim_vehicle_read (LTPL_FLEET_SIM_VEH_DOUBLES = 15 per planner)
VEHICLE_FIELDS = (("x", 0, False), ("y", 1, False), ("c", 2, False), ("s", 3, False), ("v", 4, False), ("a", 5, False), ("kappa", 6, False),
                  ("e", 7, False), ("e_max", 8, False), ("e2_sum", 9, False), ("dv_max", 10, False), ("ctl_steps", 11, True),
                  ("sat_lat", 12, True), ("sat_lon", 13, True), ("off_track_ticks", 14, True))
VEHICLE_DOUBLES = 15
VEHICLE_PARAMS = ("ax_max", "ay_max", "grip", "kappa_max", "tau_a", "tau_kappa", "k_v", "t_look", "ld_min")
# A car with 20 % headroom over a planner that plans on a gg of 5 m/s^2 (the stock local_gg): with less it saturates and runs wide
VEHICLE_DEFAULTS = dict(ax_max=6.0, ay_max=6.0, grip=1.0, kappa_max=0.2, tau_a=0.1, tau_kappa=0.08, k_v=1.0, t_look=0.3, ld_min=4.0,
                        ctl_steps=10)
VEH_STEP = 0.001


def vehicle_dict(rows):
    """[n, 15] records as a dict of named arrays (counters as int64; planners on the ideal tracker hold NaN and read -1 there)."""
    return fields_dict(rows, VEHICLE_FIELDS, VEHICLE_DOUBLES, nan_int=-1.0)


def _veh_interp(x, xp, fp, n):
    return x if math.isnan(x) else interp_at(x, xp, fp, segment(x, xp))


class VehicleModel(object):
    """Scalar host mirror of one planner's vehicle model in the operation order of csrc/fleet_vehicle.hpp (veh_tick): plain Python
    floats, + - * / sqrt only, so the device's bits. ``tick(traj_rows, dt)`` advances the car along a trajectory; ``stats`` are the
    accumulated statistics of ltpl_fleet_sim_vehicle_read. Parameters: ``VEHICLE_DEFAULTS``. (c, s) is the unit vector of the direction
    of travel; ``theta`` is the project's heading, measured from the y axis (the direction of travel is (-sin theta, cos theta), as in
    the psi column of a trajectory): c = -sin theta, s = cos theta, theta = atan2(-c, s)."""

    def __init__(self, x, y, theta, v, **params):
        par = dict(VEHICLE_DEFAULTS, **params)
        unknown = set(par) - set(VEHICLE_DEFAULTS)
        if unknown:
            raise TypeError("VehicleModel: unknown parameter(s) %s" % sorted(unknown))
        self.ctl_steps = int(par.pop("ctl_steps"))
        self.par = {k: float(par[k]) for k in VEHICLE_PARAMS}
        self.x, self.y, self.c, self.s, self.v, self.a, self.kappa = float(x), float(y), -math.sin(theta), math.cos(theta), float(v), 0.0, 0.0
        self.stats = dict(e=0.0, e_max=0.0, e2_sum=0.0, dv_max=0.0, ctl_steps=0, sat_lat=0, sat_lon=0, off_track_ticks=0)

    @property
    def theta(self):
        return math.atan2(-self.c, self.s)

    def state(self):
        return [self.x, self.y, self.c, self.s, self.v, self.a, self.kappa]

    def set_state(self, state, stats=None):
        self.x, self.y, self.c, self.s, self.v, self.a, self.kappa = (float(q) for q in state)
        if stats is not None:
            st = self.stats
            st["e"], st["e_max"], st["e2_sum"], st["dv_max"] = (float(q) for q in stats[:4])
            st["ctl_steps"], st["sat_lat"], st["sat_lon"], st["off_track_ticks"] = (int(q) for q in stats[4:8])

    def record(self):
        """The planner's record of ltpl_fleet_sim_vehicle_read (VEHICLE_FIELDS)."""
        st = self.stats
        return self.state() + [st["e"], st["e_max"], st["e2_sum"], st["dv_max"], float(st["ctl_steps"]), float(st["sat_lat"]),
                               float(st["sat_lon"]), float(st["off_track_ticks"])]

    @staticmethod
    def columns(traj_rows):
        """(s, x, y, vx, ax) as Python lists from rows [s, x, y, vx, ax] or trajectory rows [s, x, y, psi, kappa, vx, ax]."""
        a = np.asarray(traj_rows, np.float64)
        a = a.reshape(-1, 5) if a.size == 0 else a
        cols = (0, 1, 2, 5, 6) if a.shape[1] == 7 else (0, 1, 2, 3, 4)
        return tuple(a[:, k].tolist() for k in cols)

    @staticmethod
    def _seg(tx, ty, i, px, py):
        dx, dy = tx[i + 1] - tx[i], ty[i + 1] - ty[i]
        l2 = dx * dx + dy * dy
        if not l2 > 0.0:
            return None
        u = ((px - tx[i]) * dx + (py - ty[i]) * dy) / l2
        if u < 0.0:
            u = 0.0
        if u > 1.0:
            u = 1.0
        fx, fy = tx[i] + u * dx, ty[i] + u * dy
        ex, ey = px - fx, py - fy
        return ex * ex + ey * ey, u, dx, dy, l2

    def control(self, cols):
        """One control step at the present state -> (kappa_cmd, a_cmd)."""
        ts, tx, ty, tv, ta = cols
        P, st, n = self.par, self.stats, len(ts)
        ax_lim, ay_lim = P["ax_max"] * P["grip"], P["ay_max"] * P["grip"]
        px, py = self.x, self.y
        best, bd = None, math.inf
        if n > 2:
            for i in range(n - 1):
                r = self._seg(tx, ty, i, px, py)
                if r is not None and (r[0] < bd or (best is None and r[0] == bd)):       # (ties: the lower i stays; a NaN never wins)
                    best, bd = (i, r), r[0]
        if best is None:
            return self.kappa, -ax_lim
        i, (_, u, dx, dy, l2) = best
        e = (dx * (py - ty[i]) - dy * (px - tx[i])) / math.sqrt(l2)
        sf = ts[i] + u * (ts[i + 1] - ts[i])
        vref, aff = _veh_interp(sf, ts, tv, n), _veh_interp(sf, ts, ta, n)
        tl = P["t_look"] * self.v
        ld = tl if tl > P["ld_min"] else P["ld_min"]
        sl = sf + ld
        gx, gy = _veh_interp(sl, ts, tx, n), _veh_interp(sl, ts, ty, n)
        if sl > ts[n - 1]:
            for k in range(n - 2, -1, -1):
                ex, ey = tx[k + 1] - tx[k], ty[k + 1] - ty[k]
                m2 = ex * ex + ey * ey
                if m2 > 0.0:
                    m, over = math.sqrt(m2), sl - ts[n - 1]
                    gx += over * (ex / m)
                    gy += over * (ey / m)
                    break
        rx, ry = gx - px, gy - py
        yl = -self.s * rx + self.c * ry
        l2r = rx * rx + ry * ry
        kc = (2.0 * yl) / l2r if l2r > 0.0 else 0.0
        if kc > P["kappa_max"]:
            kc = P["kappa_max"]
        if kc < -P["kappa_max"]:
            kc = -P["kappa_max"]
        v2 = self.v * self.v
        if abs(kc) * v2 > ay_lim:
            kc = math.copysign(ay_lim / v2, kc)
            st["sat_lat"] += 1
        q = (kc * v2) / ay_lim
        w = 1.0 - q * q
        rem = ax_lim * math.sqrt(w if w > 0.0 else 0.0)
        dv = vref - self.v
        ac = aff + P["k_v"] * dv
        if ac > rem:
            ac = rem
            st["sat_lon"] += 1
        elif ac < -rem:
            ac = -rem
            st["sat_lon"] += 1
        st["e"] = e
        if abs(e) > st["e_max"]:
            st["e_max"] = abs(e)
        st["e2_sum"] += e * e
        if abs(dv) > st["dv_max"]:
            st["dv_max"] = abs(dv)
        st["ctl_steps"] += 1
        return kc, ac

    def plant(self, kappa_cmd, a_cmd):
        """One 1 ms plant step."""
        P, h = self.par, VEH_STEP
        self.a += (a_cmd - self.a) * (h / P["tau_a"])
        self.kappa += (kappa_cmd - self.kappa) * (h / P["tau_kappa"])
        self.v += self.a * h
        if self.v < 0.0:
            self.v = 0.0
        ds = self.v * h
        t = 0.5 * self.kappa * ds
        tt, t2 = t * t, 2.0 * t
        cn, sn = ((1.0 - tt) * self.c - t2 * self.s) / (1.0 + tt), ((1.0 - tt) * self.s + t2 * self.c) / (1.0 + tt)
        self.x += ds * (0.5 * (self.c + cn))
        self.y += ds * (0.5 * (self.s + sn))
        self.c, self.s = cn, sn

    def tick(self, traj_rows, dt, on_track=None):
        """One tick of ``dt`` on ``traj_rows`` (``columns``); ``on_track(x, y)`` (optional): the track test of the pose at the end of the
        tick, counted in ``stats['off_track_ticks']``. Returns ([x, y], v, theta)."""
        cols = traj_rows if isinstance(traj_rows, tuple) else self.columns(traj_rows)
        t, k = 0.0, 0
        cmd = (self.kappa, 0.0)
        while t < dt:
            if k % self.ctl_steps == 0:
                cmd = self.control(cols)
            self.plant(*cmd)
            t += VEH_STEP
            k += 1
        r = math.sqrt(self.c * self.c + self.s * self.s)
        self.c, self.s = self.c / r, self.s / r
        if on_track is not None and not on_track(self.x, self.y):
            self.stats["off_track_ticks"] += 1
        return [self.x, self.y], self.v, self.theta


# ---- sensor model (ltpl_fleet_sim_sensor, include/ltpl_hip.h; csrc/fleet_sensor.hpp) ------------------------------------------------------
# name, index, integer valued: the record of ltpl_fleet_sim_sensor_read (LTPL_FLEET_SIM_SENSOR_DOUBLES = 10 per planner)
SENSOR_FIELDS = (("ticks", 0, True), ("n_obj", 1, True), ("n_seen", 2, True), ("n_range", 3, True), ("n_fov", 4, True), ("n_occl", 5, True),
                 ("n_drop", 6, True), ("blind_ticks", 7, True), ("blind_clear_min", 8, False), ("blind_clear_tick", 9, True))
SENSOR_DOUBLES = 10
SENSOR_PARAMS = ("range", "r_near", "fov_cos", "occl", "p_drop")
SENSOR_SEEN, SENSOR_RANGE, SENSOR_FOV, SENSOR_OCCL, SENSOR_DROP = 0, 1, 2, 3, 4      # cause of loss, in the order of the tests


def sensor_dict(rows):
    """[n, 10] records as a dict of named arrays (counters as int64; blind_clear_tick reads -1 until an object was lost)."""
    return fields_dict(rows, SENSOR_FIELDS, SENSOR_DOUBLES)


def sensor_fov_cos(fov_deg):
    """Cosine of the half angle of the FULL opening angle ``fov_deg``; exactly 360 gives -1 (the test switched off)."""
    d = np.asarray(fov_deg, np.float64)
    return np.where(d == 360.0, -1.0, np.cos(np.radians(d) / 2.0))


def sensor_uniform(seed, tick, k):
    """u of the dropout test: ((double)w0 + 0.5) 2^-32 with w0 the first word of the block (tick, k, 0, 1) under the key (seed low, seed
    high). Scalars give a float, arrays an array."""
    seed = np.asarray(seed, np.uint64)
    w0 = philox4x32((tick, k, 0, 1), (seed & _M32, seed >> _S32))[0]
    u = (np.asarray(w0).astype(np.float64) + 0.5) * 2.0 ** -32
    return float(u) if u.ndim == 0 else u


class SensorModel(object):
    """Scalar host mirror of the sensor model in the operation order of csrc/fleet_sensor.hpp (sensor_cause) and of the statistics of
    k_fleet_sim_sense: plain Python floats, + - * sqrt and comparisons, so the device's bits. Parameters: scalars or one per planner;
    ``fov_deg`` is the full opening angle (``fov_cos`` given directly takes precedence)."""

    def __init__(self, n, range=float("inf"), fov_deg=360.0, r_near=0.0, occl=0.0, p_drop=0.0, seed=0, tick0=0, fov_cos=None):
        self.n = int(n)

        def per(v):
            return [float(x) for x in np.broadcast_to(np.asarray(v, np.float64), (self.n,))]
        self.range, self.r_near, self.occl, self.p_drop = per(range), per(r_near), per(occl), per(p_drop)
        self.fov_cos = per(sensor_fov_cos(fov_deg) if fov_cos is None else fov_cos)
        self.seed = [int(v) for v in np.broadcast_to(np.asarray(seed, np.uint64), (self.n,))]
        self.tick0 = int(tick0)
        self.rec = np.zeros((self.n, SENSOR_DOUBLES))
        self.rec[:, 8], self.rec[:, 9] = np.inf, -1.0

    @staticmethod
    def forward(theta):
        """Forward unit vector of the library's heading (measured from the y axis)."""
        return (-math.sin(theta), math.cos(theta))

    def evaluate(self, p, tick, pos, f, objs):
        """``objs``: [(x, y, r)] at the TRUE positions, in list order -> (causes, u): the cause of loss of every object (0: seen) and
        the dropout draw where one was made (NaN otherwise)."""
        px, py, fx, fy = float(pos[0]), float(pos[1]), float(f[0]), float(f[1])
        rng, near, fc, occl, pd = self.range[p], self.r_near[p], self.fov_cos[p], self.occl[p], self.p_drop[p]
        dx = [float(o[0]) - px for o in objs]
        dy = [float(o[1]) - py for o in objs]
        rad = [float(o[2]) for o in objs]
        L2 = [a * a + b * b for a, b in zip(dx, dy)]
        n = len(objs)
        causes, us = [], []
        for k in range(n):
            causes.append(self._cause(p, tick, fx, fy, dx, dy, L2, rad, n, k, rng, near, fc, occl, pd, us))
        return causes, us

    def _cause(self, p, tick, fx, fy, dx, dy, L2, rad, n, k, rng, near, fc, occl, pd, us):
        us.append(float("nan"))
        dxk, dyk, L2k = dx[k], dy[k], L2[k]
        if L2k > rng * rng:
            return SENSOR_RANGE
        if not L2k <= near * near:
            if fc > -1.0 and fx * dxk + fy * dyk < fc * math.sqrt(L2k):
                return SENSOR_FOV
            if occl > 0.0:
                for j in range(n):
                    if j == k or not L2[j] < L2k or not dx[j] * dxk + dy[j] * dyk > 0.0:
                        continue
                    cross, s = dx[j] * dyk - dy[j] * dxk, occl * rad[j]
                    if cross * cross <= (s * s) * L2k:
                        return SENSOR_OCCL
        if pd > 0.0:
            us[-1] = sensor_uniform(self.seed[p], tick & 0xFFFFFFFF, k)
            if us[-1] < pd:
                return SENSOR_DROP
        return SENSOR_SEEN

    def sense(self, p, tick, pos, theta, objs, f=None):
        """One live tick of planner ``p`` at sensor tick ``tick`` (tick0 + fleet ticks since the sensor was set): the causes of
        ``evaluate`` with f formed from ``theta`` (unless given), and the planner's statistics record updated."""
        causes, _ = self.evaluate(p, tick, pos, self.forward(theta) if f is None else f, objs)
        r = self.rec[p]
        r[0] += 1.0
        r[1] += len(objs)
        r[2] += causes.count(SENSOR_SEEN)
        for c in (SENSOR_RANGE, SENSOR_FOV, SENSOR_OCCL, SENSOR_DROP):
            r[2 + c] += causes.count(c)
        lost = [k for k, c in enumerate(causes) if c != SENSOR_SEEN]
        if lost:
            r[7] += 1.0
            px, py = float(pos[0]), float(pos[1])
            best = float("inf")
            for k in lost:
                dx, dy = float(objs[k][0]) - px, float(objs[k][1]) - py
                c = math.sqrt(dx * dx + dy * dy) - float(objs[k][2])
                if c < best:
                    best = c
            if best < r[8]:
                r[8], r[9] = best, float(tick)
        return causes

    def as_dict(self):
        return sensor_dict(self.rec)


# ---- object tracker (ltpl_fleet_sim_tracker, include/ltpl_hip.h; csrc/fleet_track.hpp) ----------------------------------------------------
# name, index, integer valued: the record of ltpl_fleet_sim_tracker_read (LTPL_FLEET_SIM_TRACKER_DOUBLES = 12 per planner)
TRACKER_FIELDS = (("ticks", 0, True), ("n_det", 1, True), ("n_matched", 2, True), ("n_born", 3, True), ("n_confirmed", 4, True),
                  ("n_del_tentative", 5, True), ("n_del_coast", 6, True), ("n_out", 7, True), ("n_out_coast", 8, True), ("n_withheld", 9, True),
                  ("n_overflow", 10, True), ("tracks_max", 11, True))
TRACKER_DOUBLES = 12
# a row of a planner's track table (LTPL_FLEET_SIM_TRACK_DOUBLES = 10)
TRACK_FIELDS = ("x", "y", "ex", "ey", "r", "v", "id", "hits", "miss", "born_tick")
TRACK_DOUBLES = 10
TRACK_CAP = 96
TRACKER_PARAMS = ("gate", "w_pos", "w_vel", "n_confirm", "n_coast")
TRACKER_DEFAULTS = dict(gate=5.0, w_pos=0.5, w_vel=0.5, n_confirm=2, n_coast=3)
TRACKER_HORIZON = 0.2                     # s: the prediction horizon of the object ingestion (ObjectListInterface.py:121)
TRACK_UNMATCHED, TRACK_OVERFLOW = -1, -2  # assignment of a detection that no track took: a track was born from it / the table was full


def tracker_dict(rows):
    """[n, 12] records as a dict of named int64 arrays."""
    return fields_dict(rows, TRACKER_FIELDS, TRACKER_DOUBLES)      # (every field of the table is integer valued)


def tracker_capacity(slots):
    """C_p = min(96, 2 S_p)."""
    return min(TRACK_CAP, 2 * int(slots))


class TrackerModel(object):
    """Scalar host mirror of ONE planner's tracker in the operation order of csrc/fleet_track.hpp: plain Python floats, + - * and
    comparisons, so the device's bits. ``slots``: the planner's staging slots S_p (``cap`` = min(96, 2 S_p) unless given); ``adv`` = dt / 0.2
    (or ``dt``). A detection is (x, y, px, py, r, v): a staged object. ``step(dets)`` -> the list handed on as [x, y, px, py, r, v] rows;
    ``assign`` then holds per detection the id of the matched track, -1 (a track was born) or -2 (overflow), ``last`` the 12 counters of
    the step; ``rec`` accumulates them."""

    def __init__(self, slots, gate=TRACKER_DEFAULTS["gate"], w_pos=TRACKER_DEFAULTS["w_pos"], w_vel=TRACKER_DEFAULTS["w_vel"],
                 n_confirm=TRACKER_DEFAULTS["n_confirm"], n_coast=TRACKER_DEFAULTS["n_coast"], tick0=0, adv=None, dt=None, cap=None):
        self.slots = int(slots)
        self.cap = tracker_capacity(slots) if cap is None else int(cap)
        self.gate, self.w_pos, self.w_vel = float(gate), float(w_pos), float(w_vel)
        self.n_confirm, self.n_coast = float(n_confirm), float(n_coast)
        if adv is None:
            adv = float(dt) / TRACKER_HORIZON
        self.adv = float(adv)
        self.tick = int(tick0)
        self.tracks = []                  # rows of TRACK_FIELDS
        self.next_id = 0.0
        self.rec = np.zeros(TRACKER_DOUBLES)
        self.assign, self.last, self.out_live = [], np.zeros(TRACKER_DOUBLES), 0

    @property
    def params(self):
        return [self.gate, self.w_pos, self.w_vel, self.n_confirm, self.n_coast]

    def table(self):
        """[96, 10], unused rows NaN (the form of ``Fleet.sim_tracker_read``)."""
        out = np.full((TRACK_CAP, TRACK_DOUBLES), np.nan)
        if self.tracks:
            out[:len(self.tracks)] = np.asarray(self.tracks, np.float64)
        return out

    def pairs(self, dets):
        """[(d2, t, k)] of every track-detection pair, in (t, k) order."""
        out = []
        for t, r in enumerate(self.tracks):
            sx, sy = self.adv * r[2], self.adv * r[3]
            xp, yp = r[0] + sx, r[1] + sy
            for k, d in enumerate(dets):
                dx, dy = float(d[0]) - xp, float(d[1]) - yp
                out.append((dx * dx + dy * dy, t, k))
        return out

    def candidates(self, dets):
        """The pairs inside the gate in ascending (d2, t, k), and gate^2 (the margins of a scenario are read off both)."""
        g2 = self.gate * self.gate
        return sorted(c for c in self.pairs(dets) if c[0] <= g2), g2

    @staticmethod
    def _blend(det, w, pred):
        diff = pred - det
        part = w * diff
        return det + part

    def skip(self):
        """A tick in which the planner is not live: the table is untouched, the tracker tick advances."""
        self.tick += 1

    def step(self, dets):
        dets = [[float(v) for v in d] for d in dets]
        K, T = len(dets), len(self.tracks)
        if K > self.slots:
            raise ValueError("TrackerModel: more detections than staging slots")
        e = [(d[2] - d[0], d[3] - d[1]) for d in dets]
        pred = []
        for r in self.tracks:
            sx, sy = self.adv * r[2], self.adv * r[3]
            pred.append((r[0] + sx, r[1] + sy))
        cand, _ = self.candidates(dets)
        tm, dm = [-1] * T, [-1] * K
        for _, t, k in cand:
            if tm[t] < 0 and dm[k] < 0:
                tm[t], dm[k] = k, t
        c = np.zeros(TRACKER_DOUBLES)
        self.assign = [TRACK_UNMATCHED] * K
        new, live = [], []
        for t, r in enumerate(self.tracks):
            r = list(r)
            xp, yp = pred[t]
            if tm[t] >= 0:
                k = tm[t]
                d = dets[k]
                r[0], r[1] = self._blend(d[0], self.w_pos, xp), self._blend(d[1], self.w_pos, yp)
                r[2], r[3] = self._blend(e[k][0], self.w_vel, r[2]), self._blend(e[k][1], self.w_vel, r[3])
                r[5] = self._blend(d[5], self.w_vel, r[5])
                r[4] = d[4]
                r[7] += 1.0
                r[8] = 0.0
                self.assign[k] = int(r[6])
                c[2] += 1
                c[4] += r[7] == self.n_confirm
                new.append(r)
                live.append(True)
            elif r[7] < self.n_confirm:
                c[5] += 1
            else:
                r[8] += 1.0
                if r[8] > self.n_coast:
                    c[6] += 1
                else:
                    r[0], r[1] = xp, yp
                    new.append(r)
                    live.append(False)
        for k, d in enumerate(dets):
            if dm[k] >= 0:
                continue
            if len(new) < self.cap:
                new.append([d[0], d[1], e[k][0], e[k][1], d[4], d[5], self.next_id, 1.0, 0.0, float(self.tick)])
                live.append(True)
                self.next_id += 1.0
                c[3] += 1
                c[4] += 1.0 == self.n_confirm
            else:
                self.assign[k] = TRACK_OVERFLOW
                c[10] += 1
        self.tracks = new
        out = [[r[0], r[1], r[0] + r[2], r[1] + r[3], r[4], r[5]] for r, lv in zip(new, live) if lv and r[7] >= self.n_confirm]
        self.out_live = len(out)
        for r, lv in zip(new, live):
            if lv:
                continue
            if len(out) < self.slots:
                out.append([r[0], r[1], r[0] + r[2], r[1] + r[3], r[4], r[5]])
                c[8] += 1
            else:
                c[9] += 1
        c[0], c[1], c[7], c[11] = 1, K, len(out), len(new)
        self.last = c
        self.rec[:11] += c[:11]
        self.rec[11] = max(self.rec[11], c[11])
        self.tick += 1
        return out

    def as_dict(self):
        return tracker_dict(self.rec[None])


# ---- prediction model (ltpl_fleet_sim_predictor, include/ltpl_hip.h; csrc/fleet_predict.hpp) ----------------------------------------------
# name, index, integer valued: the record of ltpl_fleet_sim_predictor_read (LTPL_FLEET_SIM_PREDICTOR_DOUBLES = 11 per planner)
PREDICTOR_FIELDS = (("ticks", 0, True), ("n_obj", 1, True), ("n_ingested", 2, True), ("n_still", 3, True), ("n_straight_mode", 4, True),
                    ("n_straight_dmax", 5, True), ("n_straight_dir", 6, True), ("n_straight_noseg", 7, True), ("n_track", 8, True),
                    ("d_abs_max", 9, False), ("n_wrap", 10, True))
PREDICTOR_DOUBLES = 11
PREDICTOR_PARAMS = ("mode", "horizon", "relax", "d_max")
PREDICTOR_DEFAULTS = dict(n_points=4, mode=2, horizon=2.0, relax=0.0, d_max=float("inf"))
PREDICTOR_MAX_POINTS = 8
PREDICTOR_MAX_POS = 192                   # positions per planner the path kernel holds: slots (1 + n_points) may not exceed it
PREDICTOR_INGEST_T = 0.2                  # s: the horizon of the ingestion's point (ObjectListInterface.py:121)
# outcome of an object, in the order of the record's counters [2] .. [8]
PRED_INGESTED, PRED_STILL, PRED_STRAIGHT_MODE, PRED_STRAIGHT_DMAX, PRED_STRAIGHT_DIR, PRED_STRAIGHT_NOSEG, PRED_TRACK = range(7)


def predictor_dict(rows):
    """[n, 11] records as a dict of named arrays (counters as int64)."""
    return fields_dict(rows, PREDICTOR_FIELDS, PREDICTOR_DOUBLES)


def _fdiv(a, b):
    """a / b of two floats by IEEE 754 (Python raises on a zero divisor)."""
    try:
        return a / b
    except ZeroDivisionError:
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))


class PredictorModel(object):
    """Scalar host mirror of the prediction model in the operation order of csrc/fleet_predict.hpp: plain Python floats, + - * / sqrt and
    comparisons, so the device's bits. ``table``: a ``RaceLineTable`` (columns s_rl, x, y are read); ``n_points`` K in 1 .. 8, fleet-wide;
    ``mode`` / ``horizon`` / ``relax`` / ``d_max``: scalars or one per planner. An object is (x, y, px, py, v): its staged position, the
    ingestion's 0.2 s point and its speed. ``predict(p, objs)`` -> (points [len(objs), K, 2], outcomes); ``step`` does the same and
    updates the planner's record ``rec[p]``; ``positions`` gives the [len(objs), 1 + K, 2] array the planner is handed."""

    def __init__(self, n, table, n_points=PREDICTOR_DEFAULTS["n_points"], mode=PREDICTOR_DEFAULTS["mode"], horizon=PREDICTOR_DEFAULTS["horizon"],
                 relax=PREDICTOR_DEFAULTS["relax"], d_max=PREDICTOR_DEFAULTS["d_max"]):
        self.n, self.K = int(n), int(n_points)
        if not 1 <= self.K <= PREDICTOR_MAX_POINTS:
            raise ValueError("PredictorModel: n_points must lie in 1 .. 8")

        def per(v):
            return [float(x) for x in np.broadcast_to(np.asarray(v, np.float64), (self.n,))]
        self.mode, self.horizon, self.relax, self.d_max = per(mode), per(horizon), per(relax), per(d_max)
        self.S, self.X, self.Y = (np.ascontiguousarray(np.asarray(a, np.float64)) for a in (table.s_rl, table.x, table.y))
        self.s, self.x, self.y = self.S.tolist(), self.X.tolist(), self.Y.tolist()
        self.rows = len(self.s)
        self.rec = np.zeros((self.n, PREDICTOR_DOUBLES))
        self.last_wraps = 0

    def params(self, p):
        return [self.mode[p], self.horizon[p], self.relax[p], self.d_max[p]]

    def nearest(self, x, y):
        """Step 1: the first row with the smallest d2; a d2 that is NaN or +inf is never smaller (every one: row 0)."""
        with np.errstate(all="ignore"):
            dx, dy = self.X - x, self.Y - y
            d2 = dx * dx + dy * dy
        ok = d2 < np.inf
        return int(np.argmin(np.where(ok, d2, np.inf))) if ok.any() else 0

    def _candidate(self, a, x, y):
        ex, ey = self.x[a + 1] - self.x[a], self.y[a + 1] - self.y[a]
        l2 = ex * ex + ey * ey
        if l2 == 0.0:
            return None
        t = ((x - self.x[a]) * ex + (y - self.y[a]) * ey) / l2
        if t < 0.0:
            t = 0.0
        if t > 1.0:
            t = 1.0
        fx, fy = self.x[a] + t * ex, self.y[a] + t * ey
        gx, gy = x - fx, y - fy
        return t, gx * gx + gy * gy, ex, ey, l2

    def project(self, p, x, y, px, py, v, istar=None):
        """Steps 2 and 4 -> (outcome, s0, d, segment or -1)."""
        mode = self.mode[p]
        if mode == 0.0:
            return PRED_INGESTED, 0.0, 0.0, -1
        if not v > 0.0:
            return PRED_STILL, 0.0, 0.0, -1
        if mode == 1.0:
            return PRED_STRAIGHT_MODE, 0.0, 0.0, -1
        if istar is None:
            istar = self.nearest(x, y)
        a, c = -1, None
        if istar >= 1:
            c = self._candidate(istar - 1, x, y)
            if c is not None:
                a = istar - 1
        if istar + 1 < self.rows:
            hi = self._candidate(istar, x, y)
            if hi is not None and (a < 0 or hi[1] < c[1]):
                a, c = istar, hi
        if a < 0:
            return PRED_STRAIGHT_NOSEG, 0.0, 0.0, -1
        t, _, ex, ey, l2 = c
        s0 = self.s[a] + t * (self.s[a + 1] - self.s[a])
        d = (ex * (y - self.y[a]) - ey * (x - self.x[a])) / math.sqrt(l2)
        if d > self.d_max[p] or -d > self.d_max[p]:
            return PRED_STRAIGHT_DMAX, s0, d, a
        if (px - x) * ex + (py - y) * ey < 0.0:
            return PRED_STRAIGHT_DIR, s0, d, a
        return PRED_TRACK, s0, d, a

    def _segment(self, x):
        if not x >= self.s[0]:
            return -1
        return bisect.bisect_right(self.s, x) - 1

    def _interp(self, x, fp, j):
        xp, n = self.s, self.rows
        if x != x:
            return x
        if j < 0:
            return fp[0]
        if j >= n - 1:
            return fp[n - 1]
        if xp[j] == x:
            return fp[j]
        slope = _fdiv(fp[j + 1] - fp[j], xp[j + 1] - xp[j])
        r = slope * (x - xp[j]) + fp[j]
        if r != r:
            r = slope * (x - xp[j + 1]) + fp[j + 1]
            if r != r and fp[j] == fp[j + 1]:
                r = fp[j]
        return r

    def point(self, p, j, proj, x, y, px, py, v):
        """Point j = 1 .. K -> (x, y, wrapped)."""
        oc, s0, d = proj[0], proj[1], proj[2]
        if oc in (PRED_INGESTED, PRED_STILL):
            return px, py, False
        K = self.K
        tj = (self.horizon[p] * float(j)) / float(K)
        if oc != PRED_TRACK:
            cj = tj / PREDICTOR_INGEST_T
            return x + (px - x) * cj, y + (py - y) * cj, False
        sj = s0 + v * tj
        wrapped = False
        if sj >= self.s[-1]:
            sj, wrapped = sj - self.s[-1], True
        g = self._segment(sj)
        X, Y = self._interp(sj, self.x, g), self._interp(sj, self.y, g)
        q = 0 if g < 0 else min(g, self.rows - 2)
        ex, ey = self.x[q + 1] - self.x[q], self.y[q + 1] - self.y[q]
        l2 = ex * ex + ey * ey
        if l2 == 0.0:
            return X, Y, wrapped
        ln = math.sqrt(l2)
        ux, uy = ex / ln, ey / ln
        dj = d * (1.0 - self.relax[p] * (float(j) / float(K)))
        return X - dj * uy, Y + dj * ux, wrapped

    def predict(self, p, objs):
        pts, ocs, wraps, projs = np.zeros((len(objs), self.K, 2)), [], 0, []
        for i, o in enumerate(objs):
            x, y, px, py, v = (float(c) for c in o)
            proj = self.project(p, x, y, px, py, v)
            ocs.append(proj[0])
            projs.append(proj)
            for j in range(1, self.K + 1):
                qx, qy, w = self.point(p, j, proj, x, y, px, py, v)
                pts[i, j - 1] = (qx, qy)
                wraps += w
        self.last_wraps, self.last_proj = wraps, projs
        return pts, ocs

    def counters(self, objs, ocs):
        """The record of ONE evaluation (the form of ``Fleet.sim_predictor_eval``'s ``rec``)."""
        c = np.zeros(PREDICTOR_DOUBLES)
        c[0], c[1] = 1.0, len(objs)
        for oc in ocs:
            c[2 + oc] += 1.0
        c[9] = max([abs(pr[2]) for pr in self.last_proj if pr[0] == PRED_TRACK] + [0.0])
        c[10] = self.last_wraps
        return c

    def step(self, p, objs):
        """One live tick of planner ``p``: ``predict`` and the planner's record updated."""
        pts, ocs = self.predict(p, objs)
        c = self.counters(objs, ocs)
        self.rec[p, :9] += c[:9]
        self.rec[p, 9] = max(self.rec[p, 9], c[9])
        self.rec[p, 10] += c[10]
        return pts, ocs

    def positions(self, p, objs, update=True):
        """[len(objs), 1 + K, 2]: own position, then the K points -- what the planner is handed."""
        pts, _ = self.step(p, objs) if update else self.predict(p, objs)
        own = np.asarray([[float(o[0]), float(o[1])] for o in objs], np.float64).reshape(-1, 1, 2)
        return np.concatenate((own, pts), axis=1)

    def as_dict(self):
        return predictor_dict(self.rec)


# ---- behaviour selector (ltpl_fleet_sim_selector, include/ltpl_hip.h; csrc/fleet_select.hpp) ----------------------------------------------
# name, index, integer valued: the record of ltpl_fleet_sim_selector_read (LTPL_FLEET_SIM_SELECTOR_DOUBLES = 12 per planner)
SELECTOR_FIELDS = (("ticks", 0, True), ("n_scored", 1, True), ("n_switch", 2, True), ("n_override", 3, True), ("n_unsafe", 4, True),
                   ("n_emergency", 5, True), ("chosen_straight", 6, True), ("chosen_follow", 7, True), ("chosen_left", 8, True),
                   ("chosen_right", 9, True), ("clear_min", 10, False), ("j_last", 11, False))
SELECTOR_DOUBLES = 12
SELECTOR_PARAMS = ("horizon", "r_ego", "c_hard", "c_soft", "w_clear", "w_switch")
SELECTOR_DEFAULTS = dict(horizon=2.0, r_ego=1.5, c_hard=0.0, c_soft=3.0, w_clear=2.0, w_switch=0.5)
SELECTOR_INGEST_T = 0.2                   # s: the horizon of the ingestion's point (ObjectListInterface.py:121)
SELECTOR_MAX_ROWS = 256                   # LTPL_FLEET_SIM_MAX_EXPORT
SEL_SCORED, SEL_UNSAFE, SEL_NAN, SEL_EXPORTED = 1, 2, 4, 8      # flags of an action
SEL_EMERGENCY = 4                         # LTPL_ACT_EMERGENCY


def selector_dict(rows):
    """[n, 12] records as a dict of named arrays (counters as int64)."""
    return fields_dict(rows, SELECTOR_FIELDS, SELECTOR_DOUBLES)


def selector_first(order, exported):
    """The action taken from a list: its first entry in the exported set (a set of action ids), -1 without one."""
    for a in order:
        if a in exported:
            return int(a)
    return -1


class SelectorModel(object):
    """Scalar host mirror of the behaviour selector in the operation order of csrc/fleet_select.hpp: plain Python floats (the clearance as
    elementwise numpy float64), + - * / sqrt and comparisons, so the device's bits. ``on`` and the parameters of ``SELECTOR_PARAMS``:
    scalars or one per planner. ``evaluate`` is one evaluation of the rule (the test hook's case); ``select`` is the tick's use of it for
    planner p: the list is copied unchanged for a planner that is off, has not started or has failed, and for a one-entry list; otherwise
    the planner's record ``rec[p]`` is updated. Actions are ids 0 .. 4 (straight, follow, left, right, emergency); ``actions``: for each of
    the four scored kinds None (not exported) or the rows [n, 4] = s, x, y, vx already trimmed to n_export; ``objs``: [cnt, 5] = x, y, px,
    py, r, the previous tick's staged list."""

    def __init__(self, n, on=True, **params):
        self.n = int(n)
        unknown = set(params) - set(SELECTOR_PARAMS)
        if unknown:
            raise ValueError("SelectorModel: unknown parameter %s" % sorted(unknown))
        val = dict(SELECTOR_DEFAULTS, **params)
        self.on = [bool(x) for x in np.broadcast_to(np.asarray(on), (self.n,))]
        self.par = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(val[k], np.float64), (self.n,)) for k in SELECTOR_PARAMS], axis=1))
        self.rec = np.zeros((self.n, SELECTOR_DOUBLES))
        self.rec[:, 10] = np.inf
        self.last = None                  # the actions of the latest evaluation

    def params(self, p):
        return [float(x) for x in self.par[p]]

    @staticmethod
    def times(s, v, T):
        """Steps 1 and 2: (t, n_r, last, vbar) of a trajectory with n >= 2 rows."""
        n = len(s)
        t = [0.0]
        n_r = n
        for i in range(1, n):
            m = v[i] + v[i - 1]
            if not m > 0.0:
                n_r = i
                break
            t.append(t[i - 1] + _fdiv(2.0 * (s[i] - s[i - 1]), m))
        last = 0
        for i in range(1, n_r):
            if t[i] <= T:
                last = i
        if last + 1 < n_r:
            f = _fdiv(T - t[last], t[last + 1] - t[last])
            s_t = s[last] + f * (s[last + 1] - s[last])
            vbar = _fdiv(s_t - s[0], T)
        elif n_r < n:
            vbar = _fdiv(s[last] - s[0], T)
        elif t[last] == 0.0:
            vbar = v[0]
        else:
            vbar = _fdiv(s[last] - s[0], t[last])
        return t, n_r, last, vbar

    @staticmethod
    def clearance(x, y, t, last, T, objs, r_ego):
        """Step 3: (clear, clear_obj) over the window rows (t_i <= T, i <= last) and the objects."""
        objs = np.asarray(objs, np.float64).reshape(-1, 5)
        if objs.shape[0] == 0:
            return float("inf"), -1
        tt = np.asarray(t[:last + 1], np.float64)
        xx, yy = np.asarray(x[:last + 1], np.float64), np.asarray(y[:last + 1], np.float64)
        with np.errstate(all="ignore"):
            c = tt / SELECTOR_INGEST_T
            ox, oy, px, py, rr = (objs[:, k:k + 1] for k in range(5))
            X = ox + (px - ox) * c[None, :]
            Y = oy + (py - oy) * c[None, :]
            dx, dy = xx[None, :] - X, yy[None, :] - Y
            d = (np.sqrt(dx * dx + dy * dy) - rr) - r_ego
            ok = (tt <= T)[None, :] & ~np.isnan(d)
        if not ok.any():
            return float("inf"), -1
        k = int(np.argmin(np.where(ok, d, np.inf)))             # the first minimum in (object, row) order
        if not ok.flat[k]:                                      # every candidate is +inf: the first of them
            k = int(np.argmax(ok))
        return float(d.flat[k]), k // d.shape[1]

    @staticmethod
    def _group(a, acts):
        if a == SEL_EMERGENCY:
            return 1, 0.0
        if not 0 <= a < 4 or not acts[a]["flags"] & SEL_SCORED:
            return 3, 0.0
        if acts[a]["flags"] & SEL_UNSAFE:
            return 2, (-float("inf") if acts[a]["flags"] & SEL_NAN else acts[a]["clear"])
        return 0, acts[a]["J"]

    def evaluate(self, params, user, sel_prev, actions, objs, emergency=False, rec=None):
        """One evaluation: (ordered list, the four actions as dicts flags / clear_obj / vbar / clear / J); ``rec``: a record updated in place."""
        T, r_ego, c_hard, c_soft, w_clear, w_switch = (float(q) for q in params)
        user = [int(a) for a in user]
        exported = set(a for a in range(4) if actions[a] is not None)
        if emergency:
            exported.add(SEL_EMERGENCY)
        acts = []
        for a in range(4):
            A = dict(flags=SEL_EXPORTED if a in exported else 0, clear_obj=-1, vbar=0.0, clear=float("inf"), J=0.0)
            acts.append(A)
            if a not in user or a not in exported:
                continue
            rows = np.asarray(actions[a], np.float64).reshape(-1, 4)
            if rows.shape[0] < 2:
                continue
            A["flags"] |= SEL_SCORED
            s, x, y, v = (rows[:, k].tolist() for k in range(4))
            t, n_r, last, A["vbar"] = self.times(s, v, T)
            A["clear"], A["clear_obj"] = self.clearance(x, y, t, last, T, objs, r_ego)
            pen = c_soft - A["clear"]
            if not pen > 0.0:
                pen = 0.0
            with np.errstate(all="ignore"):
                J = float((np.float64(A["vbar"]) - np.float64(w_clear) * np.float64(pen)) - np.float64(w_switch if a != sel_prev else 0.0))
            A["J"] = J
            if J != J:
                A["flags"] |= SEL_NAN | SEL_UNSAFE
            elif not A["clear"] >= c_hard:
                A["flags"] |= SEL_UNSAFE
        L = len(user)
        keys = [self._group(a, acts) for a in user]
        order = [0] * L
        for e in range(L):
            ge, ke = keys[e]
            r = 0
            for f in range(L):
                if f == e:
                    continue
                gf, kf = keys[f]
                if gf < ge or (gf == ge and (kf > ke or (not ke > kf and f < e))):
                    r += 1
            order[r] = user[e]
        if rec is not None:
            taken, alone = selector_first(order, exported), selector_first(user, exported)
            scored = [A for A in acts if A["flags"] & SEL_SCORED]
            rec[0] += 1.0
            rec[1] += float(len(scored))
            if taken >= 0 and taken != sel_prev:
                rec[2] += 1.0
            if taken != alone:
                rec[3] += 1.0
            if not any(not A["flags"] & SEL_UNSAFE for A in scored):
                rec[4] += 1.0
            if taken == SEL_EMERGENCY:
                rec[5] += 1.0
            elif taken >= 0:
                rec[6 + taken] += 1.0
            if 0 <= taken < 4 and acts[taken]["flags"] & SEL_SCORED:
                if acts[taken]["clear"] < rec[10]:
                    rec[10] = acts[taken]["clear"]
                rec[11] = acts[taken]["J"]
        self.last = acts
        return order, acts

    def select(self, p, user, sel_prev, actions, objs, emergency=False, started=True, failed=False):
        """The tick's ordered list of planner p (see the class comment)."""
        user = [int(a) for a in user]
        if not self.on[p] or len(user) < 2 or not started or failed:
            return user
        return self.evaluate(self.params(p), user, sel_prev, actions, objs, emergency, self.rec[p])[0]

    def as_dict(self):
        return selector_dict(self.rec)


# ---- safety monitor (ltpl_fleet_sim_safety, include/ltpl_hip.h; csrc/fleet_safety.hpp) ------------------------------------------------------
# name, index, integer valued: the record of ltpl_fleet_sim_safety_read (LTPL_FLEET_SIM_SAFETY_DOUBLES = 31 per planner; hist: 8 bins)
SAFETY_FIELDS = (("ticks", 0, True), ("ticks_eval", 1, True), ("prev_x", 2, False), ("prev_y", 3, False), ("prev_valid", 4, True),
                 ("gap_min", 5, False), ("gap_tick", 6, True), ("gap_slot", 7, True), ("ttc_min", 8, False), ("ttc_tick", 9, True),
                 ("ttc_slot", 10, True), ("tet", 11, False), ("tit", 12, False), ("drac_max", 13, False), ("drac_tick", 14, True),
                 ("drac_ticks", 15, True), ("thw_min", 16, False), ("thw_ticks", 17, True), ("overlap_ticks", 18, True), ("impact_max", 19, False),
                 ("n_skipped", 20, True), ("n_incidents", 21, True), ("inc_open", 22, True), ("hist", 23, True))
SAFETY_DOUBLES = 31
SAFETY_HIST = 8
# an entry of the incident ring (LTPL_FLEET_SIM_SAFETY_INCIDENTS = 8 entries of 6 doubles per planner; unwritten entries are NaN)
INCIDENT_FIELDS = ("tick_first", "tick_last", "ttc_min", "slot", "gap_min", "closing_max")
SAFETY_INCIDENTS = 8
INCIDENT_DOUBLES = 6
SAFETY_PARAMS = ("r_ego", "ttc_thr", "drac_thr", "thw_thr", "margin")
SAFETY_DEFAULTS = dict(r_ego=1.5, ttc_thr=3.0, drac_thr=3.0, thw_thr=1.0, margin=0.5)
SAFETY_INGEST_T = 0.2                     # s: the horizon of the ingestion's point (ObjectListInterface.py:121)
SAFETY_KEEP_STATE = 1                     # LTPL_SIM_SAFETY_KEEP_STATE
SAF_SKIPPED, SAF_OVERLAP, SAF_COURSE, SAF_CORRIDOR = 1, 2, 4, 8      # flags of an object
_INF = float("inf")


def safety_dict(rows):
    """[n, 31] records as a dict of named arrays (counters as int64; ``hist``: [n, 8])."""
    return fields_dict(rows, SAFETY_FIELDS, SAFETY_DOUBLES, wide=(("hist", SAFETY_HIST),))


def safety_incidents(ring, n_incidents):
    """The incidents a planner's ring [8, 6] still holds, oldest first, as dicts of ``INCIDENT_FIELDS``."""
    ring = np.asarray(ring, np.float64).reshape(SAFETY_INCIDENTS, INCIDENT_DOUBLES)
    n = int(n_incidents)
    return [dict(zip(INCIDENT_FIELDS, (float(v) for v in ring[i % SAFETY_INCIDENTS]))) for i in range(max(0, n - SAFETY_INCIDENTS), n)]


def safety_start(n=1):
    """(records [n, 31], rings [n, 8, 6]) in the start state."""
    rec = np.zeros((int(n), SAFETY_DOUBLES))
    rec[:, [5, 8, 16]] = np.inf
    return rec, np.full((int(n), SAFETY_INCIDENTS, INCIDENT_DOUBLES), np.nan)


def _saf_finite(v):
    return v - v == 0.0


def _saf_div(a, b):
    """a / b as IEEE fp64 does it where Python raises."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return float("nan")
    return math.copysign(_INF, a) * math.copysign(1.0, b)


def _saf_sqrt(v):
    return math.sqrt(v) if v >= 0.0 else (v if v == 0.0 else float("nan"))


def safety_object(par, px, py, wx, wy, obj):
    """Steps 1 .. 11 of csrc/fleet_safety.hpp for one object (x, y, px, py, r): (ttc, drac, thw, gap, closing, flags)."""
    r_ego, margin = par[0], par[4]
    ox, oy, qx, qy, r_o = (float(v) for v in obj)
    ux, uy = (qx - ox) / 0.2, (qy - oy) / 0.2
    rx, ry, vx, vy = ox - px, oy - py, ux - wx, uy - wy
    rr = rx * rx + ry * ry
    dist = _saf_sqrt(rr)
    gap = (dist - r_o) - r_ego
    rho = r_o + r_ego
    c, b, a = rr - rho * rho, rx * vx + ry * vy, vx * vx + vy * vy
    if not (_saf_finite(rr) and _saf_finite(a) and _saf_finite(b) and _saf_finite(r_o)):
        return (_INF, 0.0, _INF, gap, 0.0, SAF_SKIPPED)
    overlap = not gap > 0.0
    closing = 0.0
    if dist == 0.0:
        closing = _saf_sqrt(a)
    elif b < 0.0:
        closing = (-b) / dist
    disc = b * b - a * c
    course = b < 0.0 and disc >= 0.0
    ttc = _INF
    if overlap or not c > 0.0:
        ttc = 0.0
    elif course:
        ttc = _saf_div(c, _saf_sqrt(disc) - b)
    drac = _saf_div(closing * closing, 2.0 * gap) if (not overlap and course) else 0.0
    w2 = wx * wx + wy * wy
    wn = _saf_sqrt(w2)
    thw, corridor = _INF, False
    if wn > 0.0:
        lon, lat = (rx * wx + ry * wy) / wn, (rx * wy - ry * wx) / wn
        al = -lat if lat < 0.0 else lat
        if lon > 0.0 and al <= rho + margin:
            corridor = True
            d = lon - rho
            thw = d / wn if d > 0.0 else 0.0
    return (ttc, drac, thw, gap, closing, (SAF_OVERLAP if overlap else 0) | (SAF_COURSE if course else 0) | (SAF_CORRIDOR if corridor else 0))


def safety_objects(staged, true_xy=None):
    """The rule's objects [n, 5] = x, y, px, py, r from a staged list ``staged`` [n, 5] (the positions the planner PERCEIVED, the 0.2 s
    points built from them, radii) and, under sensor noise, the TRUE positions ``true_xy`` [n, 2] of the same objects: the true position
    and the perceived displacement, Q = X_true + (Q_staged - X_perceived), as k_fleet_sim_safety forms it. ``true_xy`` None (noise off):
    the staged list as it is."""
    staged = np.asarray(staged, np.float64).reshape(-1, 5)
    if true_xy is None:
        return staged.copy()
    t = np.asarray(true_xy, np.float64).reshape(-1, 2)
    out = staged.copy()
    out[:, 0:2] = t
    out[:, 2:4] = t + (staged[:, 2:4] - staged[:, 0:2])
    return out


def safety_tick(par, px, py, dt, tick, objs, rec, inc):
    """One live tick of the rule on a record ``rec`` [31] and a ring ``inc`` [8, 6], both updated in place (the test hook's case).
    ``objs``: [n, 5] = x, y, px, py, r. Returns (per_obj [n, 6], per_tick [8] = gap_t, gap_slot, ttc_t, ttc_slot, drac_t, thw_t, impact_t,
    closing_t)."""
    par = [float(v) for v in par]
    px, py, dt, tick = float(px), float(py), float(dt), float(tick)
    objs = np.asarray(objs, np.float64).reshape(-1, 5)
    evaluated = rec[4] != 0.0
    wx, wy = ((px - float(rec[2])) / dt, (py - float(rec[3])) / dt) if evaluated else (0.0, 0.0)
    gap_t, gap_slot, ttc_t, ttc_slot, drac_t, thw_t, impact_t, closing_t, overlaps, skipped = _INF, -1, _INF, -1, 0.0, _INF, 0.0, 0.0, 0, 0
    per_obj = np.zeros((objs.shape[0], 6))
    for k in range(objs.shape[0]):
        o = safety_object(par, px, py, wx, wy, objs[k])
        per_obj[k] = o
        ttc, drac, thw, gap, closing, flags = o
        if flags & SAF_SKIPPED:
            skipped += 1
            continue
        if gap < gap_t or (gap == gap_t and gap_slot < 0):
            gap_t, gap_slot = gap, k
        if ttc < ttc_t or (ttc == ttc_t and ttc_slot < 0):
            ttc_t, ttc_slot = ttc, k
        drac_t = drac if drac > drac_t else drac_t
        thw_t = thw if thw < thw_t else thw_t
        closing_t = closing if closing > closing_t else closing_t
        if flags & SAF_OVERLAP:
            overlaps += 1
            impact_t = closing if closing > impact_t else impact_t
    per_tick = np.array([gap_t, gap_slot, ttc_t, ttc_slot, drac_t, thw_t, impact_t, closing_t], np.float64)
    ttc_thr, drac_thr, thw_thr = par[1], par[2], par[3]
    rec[0] += 1.0
    if gap_t < rec[5]:
        rec[5], rec[6], rec[7] = gap_t, tick, float(gap_slot)
    if overlaps > 0:
        rec[18] += 1.0
    rec[2], rec[3], rec[4] = px, py, 1.0
    if not evaluated:
        return per_obj, per_tick
    rec[1] += 1.0
    if ttc_t < rec[8]:
        rec[8], rec[9], rec[10] = ttc_t, tick, float(ttc_slot)
    below = ttc_t < ttc_thr
    if below:
        rec[11] = float(rec[11]) + dt
        rec[12] = float(rec[12]) + (ttc_thr - ttc_t) * dt
    if drac_t > rec[13]:
        rec[13], rec[14] = drac_t, tick
    if drac_t > drac_thr:
        rec[15] += 1.0
    if thw_t < rec[16]:
        rec[16] = thw_t
    if thw_t < thw_thr:
        rec[17] += 1.0
    if impact_t > rec[19]:
        rec[19] = impact_t
    rec[20] += float(skipped)
    b = 7
    for j in range(6, -1, -1):
        if ttc_t < (ttc_thr * float(j + 1)) / 7.0:
            b = j
    rec[23 + b] += 1.0
    if not below:
        rec[22] = 0.0
        return per_obj, per_tick
    if rec[22] == 0.0:
        rec[21] += 1.0
        rec[22] = 1.0
        inc[(int(rec[21]) - 1) % SAFETY_INCIDENTS] = (tick, tick, ttc_t, float(ttc_slot), gap_t, closing_t)
    else:
        e = inc[(int(rec[21]) - 1) % SAFETY_INCIDENTS]
        e[1] = tick
        if ttc_t < e[2]:
            e[2], e[3] = ttc_t, float(ttc_slot)
        if gap_t < e[4]:
            e[4] = gap_t
        if closing_t > e[5]:
            e[5] = closing_t
    return per_obj, per_tick


class SafetyModel(object):
    """Scalar host mirror of the safety monitor in the operation order of csrc/fleet_safety.hpp: plain Python floats, + - * / sqrt and
    comparisons, so the device's bits. ``on`` and the parameters of ``SAFETY_PARAMS``: scalars or one per planner. ``tick0``: the monitor's
    tick of the next fleet tick. One fleet tick: ``step(p, pose, objs, dt)`` for every LIVE planner p (pose: the TRUE (x, y) of the tick,
    objs: [cnt, 5] = x, y, px, py, r of the staged list; under sensor noise ``safety_objects(staged, true_xy)``: true positions, perceived
    displacements), then ``advance()`` -- the tick index advances whether or not a planner was live. ``rec`` [n, 31] and ``inc`` [n, 8, 6] are the records and rings."""

    def __init__(self, n, on=True, tick0=0, **params):
        self.n = int(n)
        unknown = set(params) - set(SAFETY_PARAMS)
        if unknown:
            raise ValueError("SafetyModel: unknown parameter %s" % sorted(unknown))
        self.rec, self.inc = safety_start(self.n)
        self.configure(on, tick0, **params)
        self.last = [None] * self.n       # (per_obj, per_tick) of every planner's latest tick

    def configure(self, on=True, tick0=0, **params):
        """New mask, parameters and tick index; records and rings stay (LTPL_SIM_SAFETY_KEEP_STATE)."""
        val = dict(SAFETY_DEFAULTS, **params)
        self.on = [bool(x) for x in np.broadcast_to(np.asarray(on), (self.n,))]
        self.par = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(val[k], np.float64), (self.n,)) for k in SAFETY_PARAMS], axis=1))
        self.tick = int(tick0)

    def step(self, p, pose, objs, dt):
        if not self.on[p]:
            return None
        self.last[p] = safety_tick(self.par[p], pose[0], pose[1], dt, self.tick, objs, self.rec[p], self.inc[p])
        return self.last[p]

    def advance(self):
        self.tick += 1

    def as_dict(self):
        return safety_dict(self.rec)


# ---- reactive opponents (ltpl_fleet_sim_react, include/ltpl_hip.h; csrc/fleet_react.hpp) -----------------------------------------------------
# name, index, integer valued: the record of ltpl_fleet_sim_react_read (LTPL_FLEET_SIM_REACT_DOUBLES = 16 per planner)
REACT_FIELDS = (("ticks", 0, True), ("opp_ticks", 1, True), ("follow_ticks", 2, True), ("ego_lead_ticks", 3, True), ("clamped", 4, True),
                ("overlaps", 5, True), ("passive", 6, True), ("gap_min", 7, False), ("gap_tick", 8, True), ("gap_slot", 9, True),
                ("acc_min", 10, False), ("acc_tick", 11, True), ("acc_slot", 12, True), ("ego_gap_min", 13, False), ("ego_gap_tick", 14, True),
                ("ego_outside", 15, True))
REACT_DOUBLES = 16
REACT_PARAMS = ("on", "a_max", "b_comf", "b_max", "headway", "gap0", "look", "lat_gate", "ego_len")
# a race car's order of magnitude (reactive opponents): 3 m/s^2 to get back to the configured speed, 4 m/s^2 of
# comfortable and 9 m/s^2 of hardest braking, 1 s of headway on 2 m at standstill, 150 m of sight, the ego within 2 m of the race line, 5 m long
REACT_DEFAULTS = dict(a_max=3.0, b_comf=4.0, b_max=9.0, headway=1.0, gap0=2.0, look=150.0, lat_gate=2.0, ego_len=5.0)
REACT_KEEP_STATE = 1                      # LTPL_SIM_REACT_KEEP_STATE
REACT_MAX_OPP = 96
REACT_NONE, REACT_EGO = -2, -1            # `leader` of an opponent: none, the ego, else the opponent's index


def react_dict(rows):
    """[n, 16] records as a dict of named arrays (counters, ticks and slots as int64)."""
    return fields_dict(rows, REACT_FIELDS, REACT_DOUBLES)


def react_start(n=1):
    """Records [n, 16] in the start state: zeros, +inf in the minima, -1 in their ticks and slots."""
    rec = np.zeros((int(n), REACT_DOUBLES))
    rec[:, [7, 10, 13]] = np.inf
    rec[:, [8, 9, 11, 12, 14]] = -1.0
    return rec


def react_tick(par, proj, x, y, v, dt, tick, opp, rec):
    """One tick of the rule of csrc/fleet_react.hpp for one planner (the test hook's case). ``par``: the nine values of ``REACT_PARAMS``
    (``on`` is not read here); ``proj``: a ``PredictorModel`` on the race table (its nearest row, candidate segment and interpolation are
    the rule's), with the table's speed column as ``proj.vrl``; ``x, y, v``: the ego's TRUE pose and speed; ``opp`` [n, 4] = s, c, e,
    length; ``rec`` [16] is updated in place. Returns (e_new [n], per_opp [n, 4] = leader, delta, gap, acc, ego (s_e, d_e, has))."""
    _, a_max, b_comf, b_max, headway, gap0, look, lat_gate, ego_len = (float(t) for t in par)
    x, y, v, dt, tick = float(x), float(y), float(v), float(dt), float(tick)
    opp = np.asarray(opp, np.float64).reshape(-1, 4)
    n = opp.shape[0]
    # step 0
    istar = proj.nearest(x, y)
    a, c = -1, None
    if istar >= 1:
        c = proj._candidate(istar - 1, x, y)
        if c is not None:
            a = istar - 1
    if istar + 1 < proj.rows:
        hi = proj._candidate(istar, x, y)
        if hi is not None and (a < 0 or hi[1] < c[1]):
            a, c = istar, hi
    has, lead, s_e, d_e = a >= 0, False, 0.0, 0.0
    if has:
        t, _, ex, ey, l2 = c
        s_e = proj.s[a] + t * (proj.s[a + 1] - proj.s[a])
        d_e = (ex * (y - proj.y[a]) - ey * (x - proj.x[a])) / math.sqrt(l2)
        lead = (-d_e if d_e < 0.0 else d_e) <= lat_gate
    L = proj.s[-1]
    s, cs, es, ln = ([float(t) for t in opp[:, k]] for k in range(4))
    V = [proj._interp(s[q], proj.vrl, proj._segment(s[q])) for q in range(n)]
    passive = [not cs[q] > 0.0 or not V[q] > 0.0 for q in range(n)]
    u = [(cs[q] if passive[q] else es[q]) * V[q] for q in range(n)]
    e_new, per_opp = np.zeros(n), np.zeros((n, 4))
    gap_t, gap_slot, acc_t, acc_slot, ego_gap_t = _INF, -1, _INF, -1, _INF
    follow = ego_lead = clamped = overlaps = n_passive = 0
    for q in range(n):
        if passive[q]:
            n_passive += 1
            e_new[q], per_opp[q] = cs[q], (REACT_NONE, _INF, _INF, 0.0)
            continue
        v_q = es[q] * V[q]
        best, leader, ul, ll = _INF, REACT_NONE, 0.0, 0.0
        if lead:
            D = s_e - s[q]
            if D < 0.0:
                D = D + L
            if D < best:
                best, leader, ul, ll = D, REACT_EGO, v, ego_len
        for r in range(n):
            if r == q:
                continue
            D = s[r] - s[q]
            if D < 0.0:
                D = D + L
            if D == 0.0 and r > q:
                D = L
            if D < best:
                best, leader, ul, ll = D, r, u[r], ln[r]
        if leader != REACT_NONE and not best <= look:
            leader = REACT_NONE
        r = es[q] / cs[q]
        free = 1.0 - (r * r) * (r * r)
        delta, gap = _INF, _INF
        if leader == REACT_NONE:
            acc = a_max * free
        else:
            delta = best
            gap = (best - 0.5 * ll) - 0.5 * ln[q]
            follow += 1
            ego_lead += leader == REACT_EGO
            if not gap > 0.0:
                acc = -b_max
                overlaps += 1
            else:
                dv = v_q - ul
                z = v_q * headway + (v_q * dv) / (2.0 * math.sqrt(a_max * b_comf))
                if not z > 0.0:
                    z = 0.0
                k = (gap0 + z) / gap
                acc = a_max * (free - k * k)
        if acc < -b_max:
            acc = -b_max
            clamped += 1
        if acc > a_max:
            acc = a_max
        e = es[q] + (acc * dt) / V[q]
        if not e > 0.0:
            e = 0.0
        if e > cs[q]:
            e = cs[q]
        e_new[q], per_opp[q] = e, (leader, delta, gap, acc)
        if acc < acc_t:
            acc_t, acc_slot = acc, q
        if leader != REACT_NONE:
            if gap < gap_t or (gap == gap_t and gap_slot < 0):
                gap_t, gap_slot = gap, q
            if leader == REACT_EGO and gap < ego_gap_t:
                ego_gap_t = gap
    rec[0] += 1.0
    rec[1] += float(n)
    rec[2] += float(follow)
    rec[3] += float(ego_lead)
    rec[4] += float(clamped)
    rec[5] += float(overlaps)
    rec[6] += float(n_passive)
    if gap_t < rec[7]:
        rec[7], rec[8], rec[9] = gap_t, tick, float(gap_slot)
    if acc_t < rec[10]:
        rec[10], rec[11], rec[12] = acc_t, tick, float(acc_slot)
    if ego_gap_t < rec[13]:
        rec[13], rec[14] = ego_gap_t, tick
    if has and not lead:
        rec[15] += 1.0
    return e_new, per_opp, (s_e, d_e, 1.0 if has else 0.0)


def react_projector(table):
    """The race table in the form ``react_tick`` reads: a ``PredictorModel`` (nearest row, candidate segment, interpolation) with the
    speed column ``vrl``."""
    proj = PredictorModel(1, table)
    proj.vrl = np.asarray(table.vel_rl, np.float64).tolist()
    return proj


class ReactModel(object):
    """Scalar host mirror of the reactive opponents in the operation order of csrc/fleet_react.hpp: plain Python floats, + - * / sqrt and
    comparisons, so the device's bits. ``table``: the ``RaceLineTable``; ``scales``: per planner the CONFIGURED vel_scale of its
    opponents (the start value of the effective scale ``eff[p]``); ``on`` and the parameters of ``REACT_PARAMS``: scalars or one per
    planner; ``tick0``: the model's tick of the next fleet tick. One fleet tick, at its head: ``step(p, pose, vel, opp_s, scales, lengths,
    dt)`` for every planner without an error word (pose, vel: the TRUE ones of the previous tick; scales: the configured ones as the
    events left them) returns and stores the effective scales the tick's opponents drive with, then ``advance()`` -- the tick index
    advances whether or not a planner is live. A planner with ``on`` 0 gets its configured scales."""

    def __init__(self, n, table, scales, on=True, tick0=0, **params):
        self.n = int(n)
        self.proj = react_projector(table)
        self.eff = [np.array(c, np.float64).reshape(-1) for c in scales]
        self.rec = react_start(self.n)
        self.configure(on, tick0, **params)
        self.last = [None] * self.n       # (per_opp, ego) of every planner's latest tick

    def configure(self, on=True, tick0=0, **params):
        """New mask, parameters and tick index; effective scales and records stay (LTPL_SIM_REACT_KEEP_STATE)."""
        unknown = set(params) - set(REACT_PARAMS)
        if unknown:
            raise ValueError("ReactModel: unknown parameter %s" % sorted(unknown))
        val = dict(REACT_DEFAULTS, **params)
        self.on = [bool(x) for x in np.broadcast_to(np.asarray(on), (self.n,))]
        val["on"] = [1.0 if x else 0.0 for x in self.on]
        self.par = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(val[k], np.float64), (self.n,)) for k in REACT_PARAMS], axis=1))
        self.tick = int(tick0)

    def step(self, p, pose, vel, opp_s, scales, lengths, dt):
        scales = np.asarray(scales, np.float64).reshape(-1)
        if not self.on[p]:
            self.eff[p] = scales.copy()
            return self.eff[p]
        opp = np.column_stack((np.asarray(opp_s, np.float64).reshape(-1), scales, self.eff[p], np.asarray(lengths, np.float64).reshape(-1)))
        e, per_opp, ego = react_tick(self.par[p], self.proj, pose[0], pose[1], vel, dt, self.tick, opp, self.rec[p])
        self.eff[p], self.last[p] = e, (per_opp, ego)
        return e

    def advance(self):
        self.tick += 1

    def as_dict(self):
        return react_dict(self.rec)


# ---- campaign statistics (ltpl_fleet_sim_stats, include/ltpl_hip.h; csrc/fleet_stats.hpp) ---------------------------------------------------
# name, index, integer valued: the row of ltpl_fleet_sim_stats_reduce (LTPL_FLEET_SIM_STATS_DOUBLES = 27 per group and measure; hist: 16 cells)
STATS_FIELDS = (("n", 0, True), ("n_nan", 1, True), ("n_inf", 2, True), ("min", 3, False), ("argmin", 4, True), ("max", 5, False),
                ("argmax", 6, True), ("sum", 7, False), ("sumsq", 8, False), ("under", 9, True), ("over", 10, True), ("hist", 11, True))
STATS_DOUBLES = 27
STATS_BINS = 16                           # LTPL_FLEET_SIM_STATS_MAX_BINS
STATS_MAX_TOP = 8                         # LTPL_FLEET_SIM_STATS_MAX_TOP
STATS_CHUNK, STATS_LANES = 1024, 64       # the sum order: chunks of 1024 members, 64 lane sums per chunk
STATS_KEEP_SERIES = 1                     # LTPL_SIM_STATS_KEEP_SERIES
STATS_FAMILIES = ("telemetry", "vehicle", "sensor", "tracker", "predictor", "selector", "safety", "react", "state")      # LTPL_SIM_STATS_*
STATE_FIELDS = (("failed", 0, True),)     # the pseudo-family: 1.0 for a planner whose error word is set


def _stats_family_columns():
    cols = {}
    for fam, fields in (("telemetry", TELEMETRY_FIELDS), ("vehicle", VEHICLE_FIELDS), ("sensor", SENSOR_FIELDS), ("tracker", TRACKER_FIELDS),
                        ("predictor", PREDICTOR_FIELDS), ("selector", SELECTOR_FIELDS), ("safety", SAFETY_FIELDS), ("react", REACT_FIELDS),
                        ("state", STATE_FIELDS)):
        cols[fam] = {f[0]: int(f[1]) for f in fields}
    return cols


STATS_FAMILY_DOUBLES = dict(telemetry=TELEMETRY_DOUBLES, vehicle=VEHICLE_DOUBLES, sensor=SENSOR_DOUBLES, tracker=TRACKER_DOUBLES,
                            predictor=PREDICTOR_DOUBLES, selector=SELECTOR_DOUBLES, safety=SAFETY_DOUBLES, react=REACT_DOUBLES, state=1)


def stats_column(family, field):
    """(family id, column) of a measure: ``family`` a name of ``STATS_FAMILIES`` (or its id), ``field`` a name of the family's ``*_FIELDS``
    table, ``"name[k]"`` for element k of a field with several doubles (``"act[2]"``, ``"hist[3]"``), or the column itself."""
    fam = STATS_FAMILIES[family] if isinstance(family, (int, np.integer)) else str(family)
    if fam not in STATS_FAMILIES:
        raise ValueError("stats: unknown family %r" % (family,))
    if isinstance(field, (int, np.integer)):
        return STATS_FAMILIES.index(fam), int(field)
    name, k = str(field), 0
    if name.endswith("]") and "[" in name:
        name, k = name[:-1].split("[")
        k = int(k)
    cols = _stats_family_columns()[fam]
    if name not in cols:
        raise ValueError("stats: family %s has no field %r" % (fam, field))
    return STATS_FAMILIES.index(fam), cols[name] + k


def stats_edges(lo, hi, bins):
    """The bins + 1 edges e_j = lo + ((hi - lo) * j) / bins, in exactly this order."""
    lo, hi = float(lo), float(hi)
    return [lo + ((hi - lo) * float(j)) / float(int(bins)) for j in range(int(bins) + 1)]


def stats_sum(x):
    """The sum of the doubles ``x`` (member order; a skipped member as +0.0) in THE order of csrc/fleet_stats.hpp: chunks of 1024, inside
    a chunk 64 lane sums (lane i mod 64, serially in ascending i from +0.0), folded by t[l] += t[l + s] for s = 32 .. 1, the chunk sums
    added serially from +0.0. Adding +0.0 for a skipped member leaves every bit: a sum that starts at +0.0 is never -0.0."""
    x = np.asarray(x, np.float64).reshape(-1)
    nch = (x.size + STATS_CHUNK - 1) // STATS_CHUNK
    a = np.zeros(nch * STATS_CHUNK)
    a[:x.size] = x
    a = a.reshape(nch, STATS_CHUNK // STATS_LANES, STATS_LANES)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.zeros((nch, STATS_LANES))
        for j in range(a.shape[1]):
            t = t + a[:, j, :]
        s = STATS_LANES // 2
        while s >= 1:
            t = t[:, :s] + t[:, s:2 * s]
            s //= 2
        total = 0.0
        for c in range(nch):
            total = total + float(t[c, 0])
    return total


def stats_reduce(values, planners, lo, hi, bins, top_dir, top_k):
    """One group and one measure on the host, bit for bit what k_fleet_sim_stats_chunk / _merge leave: (row [27], top [8, 2]).
    ``values`` in member order, ``planners`` their planner indices (None: the positions), distinct."""
    v = np.asarray(values, np.float64).reshape(-1)
    p = np.arange(v.size, dtype=np.int64) if planners is None else np.asarray(planners, np.int64).reshape(-1)
    bins, top_dir, top_k = int(bins), int(top_dir), int(top_k)
    row = np.zeros(STATS_DOUBLES)
    top = np.full((STATS_MAX_TOP, 2), np.nan)
    top[:, 1] = -1.0
    nan = np.isnan(v)
    fin = np.isfinite(v)
    row[0], row[1], row[2] = fin.sum(), nan.sum(), (~nan & ~fin).sum()
    row[3], row[4], row[5], row[6] = np.inf, -1.0, -np.inf, -1.0
    ok = np.flatnonzero(~nan)
    if ok.size:
        for at, val in ((3, v[ok].min()), (5, v[ok].max())):
            tie = ok[v[ok] == val]                               # (== : a -0.0 ties with a +0.0)
            i = tie[np.argmin(p[tie])]
            row[at], row[at + 1] = v[i], p[i]
    with np.errstate(over="ignore"):
        good = np.where(fin, v, 0.0)
        row[7] = stats_sum(good)
        row[8] = stats_sum(good * good)
    e = stats_edges(lo, hi, bins)
    with np.errstate(invalid="ignore"):
        under, over = ~nan & (v < e[0]), ~nan & (v >= e[bins])
        cell = np.zeros(v.size, np.int64)
        for j in range(1, bins):
            cell += (e[j] <= v)
    row[9], row[10] = under.sum(), over.sum()
    inside = fin & ~under & ~over
    row[11:11 + STATS_BINS] = np.bincount(cell[inside], minlength=STATS_BINS)[:STATS_BINS]
    if top_dir != 0 and top_k > 0 and ok.size:
        key = -v[ok] if top_dir > 0 else v[ok]
        order = ok[np.lexsort((p[ok], key))][:top_k]
        top[:order.size, 0], top[:order.size, 1] = v[order], p[order]
    return row, top


def stats_dict(rows):
    """[..., 27] rows as a dict of named arrays (counts as int64; ``hist``: [..., 16]) plus ``mean`` = sum / n and ``var`` = sumsq / n -
    mean^2, computed here on the host (NaN where n == 0)."""
    rows = np.asarray(rows, np.float64)
    out = fields_dict(rows, STATS_FIELDS, wide=(("hist", STATS_BINS),))
    with np.errstate(divide="ignore", invalid="ignore"):
        n = rows[..., 0]
        out["mean"] = np.where(n > 0, rows[..., 7] / n, np.nan)
        out["var"] = np.where(n > 0, rows[..., 8] / n - out["mean"] * out["mean"], np.nan)
    return out


class StatsModel(object):
    """Host mirror of a statistics plan (ltpl_fleet_sim_stats): ``groups`` [n] in -1 .. G - 1, ``measures`` a list of (family, field, lo,
    hi, bins, top_dir) as ``Fleet.sim_stats`` takes them, ``top_k``, ``period``, ``depth``, ``tick0``. ``reduce(records, failed)`` takes
    the record arrays a test has from the ``_read`` calls or the other mirrors -- a dict family name -> [n, D] -- and ``failed`` [n] (the
    STATE family; default: nobody) and returns (rows [G, M, 27], tops [G, M, top_k, 2]). ``tick(records, failed)`` is one fleet tick: the
    index advances, and on the ticks of the rule ((index + 1) % period == 0) a row enters the ring; ``series()`` returns (ticks, rows
    [held, G, M, 27], rows ever written), oldest first."""

    def __init__(self, groups, measures, top_k=0, period=0, depth=0, tick0=0, n_groups=None):
        self.group = np.asarray(groups, np.int64).reshape(-1)
        self.G = int(self.group.max()) + 1 if n_groups is None else int(n_groups)
        self.members = [np.flatnonzero(self.group == g) for g in range(self.G)]      # planners ascending inside a group
        self.measures = [stats_column(m[0], m[1]) + (float(m[2]), float(m[3]), int(m[4]), int(m[5])) for m in measures]
        self.top_k, self.period, self.depth, self.index = int(top_k), int(period), int(depth), int(tick0)
        self.ring, self.ring_tick, self.n_rows = [], [], 0

    def values(self, records, failed, fam, col):
        if STATS_FAMILIES[fam] == "state":
            f = np.zeros(self.group.size) if failed is None else np.asarray(failed).reshape(-1)
            return np.where(f != 0, 1.0, 0.0)
        return np.asarray(records[STATS_FAMILIES[fam]], np.float64).reshape(self.group.size, -1)[:, col]

    def reduce(self, records, failed=None):
        rows = np.zeros((self.G, len(self.measures), STATS_DOUBLES))
        tops = np.zeros((self.G, len(self.measures), self.top_k, 2))
        for m, (fam, col, lo, hi, bins, top_dir) in enumerate(self.measures):
            col_v = self.values(records, failed, fam, col)
            for g, mem in enumerate(self.members):
                rows[g, m], top = stats_reduce(col_v[mem], mem, lo, hi, bins, top_dir, self.top_k)
                tops[g, m] = top[:self.top_k]
        return rows, tops

    def tick(self, records, failed=None):
        index = self.index
        self.index += 1
        if self.period > 0 and (index + 1) % self.period == 0:
            row = self.reduce(records, failed)[0]
            if len(self.ring) < self.depth:
                self.ring.append(row)
                self.ring_tick.append(index)
            else:
                self.ring[self.n_rows % self.depth], self.ring_tick[self.n_rows % self.depth] = row, index
            self.n_rows += 1
            return True
        return False

    def series(self):
        held = len(self.ring)
        order = [(self.n_rows - held + k) % self.depth for k in range(held)] if held else []
        return (np.asarray([self.ring_tick[i] for i in order], np.int32), np.asarray([self.ring[i] for i in order]).reshape(held, self.G, -1, STATS_DOUBLES),
                self.n_rows)
