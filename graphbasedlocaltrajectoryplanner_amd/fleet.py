"""
ctypes binding of the fleet entry points (``ltpl_fleet_*``, include/ltpl_hip.h ABI v5): the planner of ``planner.py`` -- the
iterative memory of the reference's ``OnlineTrajectoryHandler`` (graph_ltpl/online_graph/src/OnlineTrajectoryHandler.py:24-1040) -- for
MANY vehicles on one lattice with the state in device memory. Every stage the host planner runs per vehicle on the CPU runs as a kernel
with one wave64 per planner (csrc/fleet_core.hpp); arguments, views and accessors are those of ``Planner``.

The tape form pre-uploads the inputs of many ticks and advances all planners through them without host synchronisation
(``tape_append`` / ``tape_append_groups`` / ``tape_run``): the closed-loop, state-carrying throughput of the hot path.
"""
import ctypes as C
import math

import numpy as np

from . import _capi
from .planner import KEY_IDS, KEY_NAMES, PathsView, Planner, PlannerPathsIn, PlannerVelIn, TrajView
from .sim import TELEMETRY_DOUBLES, TELEMETRY_FIELDS, telemetry_dict      # noqa: F401  (published here: fleet.TELEMETRY_FIELDS)
from .sim import VEHICLE_DEFAULTS, VEHICLE_DOUBLES, VEHICLE_FIELDS, VEHICLE_PARAMS, vehicle_dict      # noqa: F401  (fleet.VEHICLE_FIELDS)
from .sim import SENSOR_DOUBLES, SENSOR_FIELDS, SENSOR_PARAMS, sensor_dict, sensor_fov_cos      # noqa: F401  (fleet.SENSOR_FIELDS)
from .sim import TRACK_CAP, TRACK_DOUBLES, TRACK_FIELDS, TRACKER_DEFAULTS, TRACKER_DOUBLES, TRACKER_FIELDS, TRACKER_PARAMS, tracker_dict      # noqa: F401
from .sim import PREDICTOR_DEFAULTS, PREDICTOR_DOUBLES, PREDICTOR_FIELDS, PREDICTOR_MAX_POINTS, PREDICTOR_PARAMS, predictor_dict      # noqa: F401
from .sim import SELECTOR_DEFAULTS, SELECTOR_DOUBLES, SELECTOR_FIELDS, SELECTOR_MAX_ROWS, SELECTOR_PARAMS, selector_dict      # noqa: F401
from .sim import (INCIDENT_DOUBLES, INCIDENT_FIELDS, SAFETY_DEFAULTS, SAFETY_DOUBLES, SAFETY_FIELDS, SAFETY_INCIDENTS, SAFETY_KEEP_STATE,      # noqa: F401
                  SAFETY_PARAMS, safety_dict, safety_start)
from .sim import REACT_DEFAULTS, REACT_DOUBLES, REACT_FIELDS, REACT_KEEP_STATE, REACT_MAX_OPP, REACT_PARAMS, react_dict, react_start      # noqa: F401
from .sim import (STATE_FIELDS, STATS_BINS, STATS_DOUBLES, STATS_FAMILIES, STATS_FIELDS, STATS_KEEP_SERIES, STATS_MAX_TOP, stats_column,      # noqa: F401
                  stats_dict)
from .sim import pack_events as sim_pack_events


class SimIn(C.Structure):                 # ltpl_fleet_sim_in (pointer members as plain addresses)
    _fields_ = [("n_rl", C.c_int32), ("race", C.c_void_p),
                ("opp_off", C.c_void_p), ("opp_s0", C.c_void_p), ("opp_vel_scale", C.c_void_p), ("opp_length", C.c_void_p),
                ("static_off", C.c_void_p), ("static_x", C.c_void_p), ("static_y", C.c_void_p), ("static_theta", C.c_void_p),
                ("static_v", C.c_void_p), ("static_length", C.c_void_p),
                ("t0", C.c_double), ("tic0", C.c_double), ("dt", C.c_double), ("n_export", C.c_int32),
                ("pref_off", C.c_void_p), ("pref_action", C.c_void_p),
                ("pos_est_x", C.c_void_p), ("pos_est_y", C.c_void_p), ("vel_est", C.c_void_p),
                ("zone_off", C.c_void_p), ("zone_gid", C.c_void_p)]


class SimRaceIn(C.Structure):             # ltpl_fleet_sim_race_in
    _fields_ = [("n_races", C.c_int32), ("race_off", C.c_void_p), ("length", C.c_void_p), ("heading0", C.c_void_p)]


class FrictionIn(C.Structure):            # ltpl_fleet_friction_in
    _fields_ = [("n_maps", C.c_int32), ("x0", C.c_void_p), ("y0", C.c_void_p), ("dx", C.c_void_p), ("dy", C.c_void_p),
                ("nx", C.c_void_p), ("ny", C.c_void_p), ("node_off", C.c_void_p), ("nodes", C.c_void_p),
                ("map_idx", C.c_void_p), ("scale", C.c_void_p)]


class SimTeleIn(C.Structure):             # ltpl_fleet_sim_tele_in
    _fields_ = [("radius", C.c_void_p), ("grid_s", C.c_void_p)]


class SimEventsIn(C.Structure):            # ltpl_fleet_sim_events_in
    _fields_ = [("n_events", C.c_int32), ("ev_off", C.c_void_p), ("when_kind", C.c_void_p), ("when_index", C.c_void_p),
                ("when_value", C.c_void_p), ("set_kind", C.c_void_p), ("set_index", C.c_void_p), ("set_value", C.c_void_p)]


class SimNoiseIn(C.Structure):             # ltpl_fleet_sim_noise_in
    _fields_ = [("seed", C.c_void_p), ("sigma_pos", C.c_void_p), ("sigma_vel", C.c_void_p), ("sigma_obj_pos", C.c_void_p),
                ("sigma_obj_theta", C.c_void_p), ("sigma_obj_vel", C.c_void_p), ("tick0", C.c_int32)]


class SimVehicleIn(C.Structure):           # ltpl_fleet_sim_vehicle_in
    _fields_ = [("model", C.c_void_p)] + [(k, C.c_void_p) for k in VEHICLE_PARAMS] + [("ctl_steps", C.c_int32), ("flags", C.c_uint32)]


class SimSensorIn(C.Structure):            # ltpl_fleet_sim_sensor_in
    _fields_ = [(k, C.c_void_p) for k in SENSOR_PARAMS] + [("seed", C.c_void_p), ("tick0", C.c_int32)]


class SimTrackerIn(C.Structure):           # ltpl_fleet_sim_tracker_in
    _fields_ = [(k, C.c_void_p) for k in TRACKER_PARAMS] + [("tick0", C.c_int32)]


class SimPredictorIn(C.Structure):         # ltpl_fleet_sim_predictor_in
    _fields_ = [("n_points", C.c_int32)] + [(k, C.c_void_p) for k in PREDICTOR_PARAMS]


class SimSelectorIn(C.Structure):          # ltpl_fleet_sim_selector_in
    _fields_ = [("on", C.c_void_p)] + [(k, C.c_void_p) for k in SELECTOR_PARAMS]


class SimSafetyIn(C.Structure):            # ltpl_fleet_sim_safety_in
    _fields_ = [("on", C.c_void_p)] + [(k, C.c_void_p) for k in SAFETY_PARAMS] + [("tick0", C.c_int32), ("flags", C.c_uint32)]


class SimReactIn(C.Structure):             # ltpl_fleet_sim_react_in
    _fields_ = [("on", C.c_void_p)] + [(k, C.c_void_p) for k in REACT_PARAMS[1:]] + [("tick0", C.c_int32), ("flags", C.c_uint32)]


class SimStatsIn(C.Structure):             # ltpl_fleet_sim_stats_in
    _fields_ = [("n_groups", C.c_int32), ("group", C.c_void_p), ("n_measures", C.c_int32), ("family", C.c_void_p), ("column", C.c_void_p),
                ("lo", C.c_void_p), ("hi", C.c_void_p), ("bins", C.c_void_p), ("top_dir", C.c_void_p), ("top_k", C.c_int32),
                ("period", C.c_int32), ("depth", C.c_int32), ("tick0", C.c_int32), ("flags", C.c_uint32)]


class SimRecordHead(C.Structure):         # ltpl_fleet_sim_record_head
    _fields_ = [("tick", C.c_int32), ("planner", C.c_int32), ("error", C.c_int32), ("sel_action", C.c_int32),
                ("t_now", C.c_double), ("pos_x", C.c_double), ("pos_y", C.c_double), ("vel_est", C.c_double), ("heading", C.c_double),
                ("n_objects", C.c_int32), ("reserved0", C.c_int32)]


SIM_TRACE_DOUBLES = 8 + 8 + 9 * _capi.PLANNER_MAX_KEYS     # LTPL_FLEET_SIM_TRACE_DOUBLES
SIM_RECORD_OBJECTS = 96                                    # LTPL_FLEET_SIM_RECORD_OBJECTS
SIM_SNAPSHOTS = 8                                          # LTPL_FLEET_SIM_SNAPSHOTS
SIM_MAX_TRIGGERS = 16                                      # LTPL_FLEET_SIM_MAX_TRIGGERS


def _per(v, dtype, n):
    """A scalar, or one value per planner / per case, as a contiguous array of ``dtype`` with ``n`` entries (``n`` may be a shape)."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype), n if isinstance(n, tuple) else (n,)))


def _zeros(m, *tail, dtype=np.float64):
    """An output buffer for ``m`` cases that holds at least one, so that no pointer is empty; the caller cuts the result back to [:m]."""
    return np.zeros((max(int(m), 1),) + tail, dtype)


def _offsets(counts):
    """int32 offsets [len(counts) + 1] of lists laid back to back, starting at 0."""
    return np.ascontiguousarray(np.concatenate(([0], np.cumsum(counts))).astype(np.int32))


def _ragged(lists, width=None, dtype=np.float64):
    """Per-case lists of rows [n_q, width] (``width=None``: values [n_q]) for a test hook: (int32 offsets [m + 1] starting at 0, the rows
    back to back with one zero row appended, so that no pointer is empty)."""
    tail = () if width is None else (width,)
    rows = [np.asarray(x, dtype).reshape((-1,) + tail) for x in lists]
    return _offsets([r.shape[0] for r in rows]), np.ascontiguousarray(np.concatenate(rows + [np.zeros((1,) + tail)]))


def _split(buf, off):
    """What a test hook wrote per row of ``_ragged``'s flat array, cut back into one copy per case."""
    return [buf[off[q]:off[q + 1]].copy() for q in range(len(off) - 1)]


_h = _p = C.c_void_p                      # the handle; an array handed over as its address
_i, _d, _pi = C.c_int32, C.c_double, C.POINTER(C.c_int32)
# (probe symbol, ((entry point, argtypes), ...)): a group is declared when the library exports its probe (None: always) -- a build without
# the simulation binds too
_ENTRY_POINTS = (
    (None, (("set_start_range", (_h, _i, _i, _d, _d, _d, _d, _d, _pi, _pi)),
            ("tape_clear", (_h,)),
            ("tape_append", (_h, C.POINTER(PlannerPathsIn), C.POINTER(PlannerVelIn))),
            ("tape_run", (_h, _i, _i, C.POINTER(C.c_float))))),
    ("digest", (("digest", (_h, C.POINTER(_d), _i)),)),
    ("sim_run", (("sim_setup", (_h, C.POINTER(SimIn))),
                 ("sim_vel", (_h, C.POINTER(PlannerVelIn))),
                 ("sim_run", (_h, _i, _p, _i, C.POINTER(C.c_float))),
                 ("sim_state", (_h,) + (_p,) * 7))),
    ("sim_race", (("sim_race", (_h, C.POINTER(SimRaceIn))),
                  ("sim_heading", (_h, _p)))),
    ("sim_telemetry", (("sim_telemetry", (_h, C.POINTER(SimTeleIn))),
                       ("sim_telemetry_read", (_h, _p, _i, C.POINTER(_d))))),
    ("sim_record", (("sim_record", (_h, _p, _i, _i)),
                    ("sim_record_info", (_h,) + (_pi,) * 4),
                    ("sim_record_get", (_h, _i, _i, C.POINTER(SimRecordHead), _p, C.POINTER(PathsView), _p, C.POINTER(TrajView))))),
    ("sim_branch", (("sim_snapshot", (_h, _i, _p, _i)),
                    ("sim_snapshot_info", (_h, _i, _pi, _p, _i, C.POINTER(C.c_uint64))),
                    ("sim_snapshot_drop", (_h, _i)),
                    ("sim_branch", (_h, _i, _p, _p, _i, C.POINTER(C.c_float))))),
    ("sim_events", (("sim_events", (_h, C.POINTER(SimEventsIn))),
                    ("sim_events_read", (_h, _p, _pi, _pi)))),
    ("sim_noise", (("sim_noise", (_h, C.POINTER(SimNoiseIn))),
                   ("sim_estimate", (_h, _p, _p, _p)),
                   ("sim_noise_draws", (_h, _p, _p, _p, _p, _i, _p, _p)))),
    ("sim_vehicle", (("sim_vehicle", (_h, C.POINTER(SimVehicleIn))),
                     ("sim_vehicle_read", (_h, _p, _i)),
                     ("sim_vehicle_step", (_h, _i) + (_p,) * 7 + (_i, _p)))),
    ("sim_sensor", (("sim_sensor", (_h, C.POINTER(SimSensorIn))),
                    ("sim_sensor_read", (_h, _p, _i)),
                    ("sim_sensor_eval", (_h, _i) + (_p,) * 8))),
    ("sim_tracker", (("sim_tracker", (_h, C.POINTER(SimTrackerIn))),
                     ("sim_tracker_read", (_h, _p, _i, _i, _p, _p, _p)),
                     ("sim_tracker_eval", (_h, _i) + (_p,) * 16))),
    ("sim_predictor", (("sim_predictor", (_h, C.POINTER(SimPredictorIn))),
                       ("sim_predictor_read", (_h, _p, _i)),
                       ("sim_predictor_eval", (_h, _i, _i) + (_p,) * 6))),
    ("sim_selector", (("sim_selector", (_h, C.POINTER(SimSelectorIn))),
                      ("sim_selector_read", (_h, _p, _i, _p, _i)),
                      ("sim_selector_eval", (_h, _i) + (_p,) * 10))),
    ("sim_safety", (("sim_safety", (_h, C.POINTER(SimSafetyIn))),
                    ("sim_safety_read", (_h, _p, _i, _p, _i)),
                    ("sim_safety_eval", (_h, _i) + (_p,) * 10))),
    ("sim_react", (("sim_react", (_h, C.POINTER(SimReactIn))),
                   ("sim_react_read", (_h, _p, _i, _p)),
                   ("sim_react_eval", (_h, _i) + (_p,) * 10))),
    ("sim_stats", (("sim_stats", (_h, C.POINTER(SimStatsIn))),
                   ("sim_stats_reduce", (_h, _p, _i, _p, _i)),
                   ("sim_stats_series", (_h, _p, _p, _i, _pi, C.POINTER(C.c_int64))),
                   ("sim_stats_eval", (_h, _i) + (_p,) * 6))),
    ("friction", (("friction", (_h, C.POINTER(FrictionIn))),
                  ("friction_scale", (_h, _p)),
                  ("friction_rows", (_h, _i, _p, _p, _i, _d, _p)))))


class Fleet(Planner):
    def __init__(self, backend, n_planners, **config):
        Planner.__init__(self, backend, n_scen=n_planners, prefix="ltpl_fleet_", **config)

    def _declare(self):
        Planner._declare(self)
        for probe, group in _ENTRY_POINTS:
            if probe is None or hasattr(self.lib, "ltpl_fleet_" + probe):
                for name, argtypes in group:
                    self._fn(name).argtypes = list(argtypes)

    # ---- one path each for the setters, the reads and (with _ragged / _split) the test hooks of the simulation's models ----------------------
    def _set(self, name, struct=None, columns=(), **scalars):
        """A setter's call: ``struct`` with its plain members ``scalars`` and an array per entry of ``columns`` = (member, value, dtype[,
        entries]) -- a scalar or one value per planner (or per ``entries``); a member without an entry stays NULL. ``struct=None`` hands
        NULL, the off switch. The arrays live until the call is back."""
        if struct is None:
            return self._check(self._fn(name)(self.handle, None))
        si = struct(**scalars)
        keep = [_per(c[1], c[2], c[3] if len(c) > 3 else self.n_scen) for c in columns]
        for c, a in zip(columns, keep):
            setattr(si, c[0], a.ctypes.data)
        self._check(self._fn(name)(self.handle, C.byref(si)))

    def _read(self, name, doubles, *extra, rows=None):
        """A read's call: the records [n_planners (or the shape ``rows``), doubles], filled by ``name`` (out, doubles, *extra)."""
        out = np.zeros((rows if rows is not None else (self.n_scen,)) + (doubles,), np.float64)
        self._check(self._fn(name)(self.handle, out.ctypes.data, doubles, *extra))
        return out

    def set_start(self, scen, pos, heading, vel=0.0, max_heading_offset=math.pi / 4):
        out = Planner.set_start(self, scen, pos, heading, vel, max_heading_offset)
        self._start_heading()[int(scen)] = float(heading)
        return out

    def _start_heading(self):
        if getattr(self, "_heading", None) is None:
            self._heading = np.zeros(self.n_scen, np.float64)
        return self._heading

    def set_start_range(self, first, past_last, pos, heading, vel=0.0, max_heading_offset=math.pi / 4):
        """``set_start`` with the same pose for the planners [first, past_last) in one call (ltpl_fleet_set_start_range)."""
        it, ch = C.c_int32(1), C.c_int32(1)
        self._check(self._fn("set_start_range")(self.handle, int(first), int(past_last), float(pos[0]), float(pos[1]), float(heading),
                                                float(vel), float(max_heading_offset), C.byref(it), C.byref(ch)))
        self._start_heading()[int(first):int(past_last)] = float(heading)
        return bool(it.value), bool(ch.value)

    # ---- tape ---------------------------------------------------------------------------------------------------------------
    def tape_clear(self):
        self._check(self._fn("tape_clear")(self.handle))

    def tape_append(self, prev_actions, t_now, vehicles, zone_gids, pos_est, vel_est, **vel_kwargs):
        """Inputs of one tick, arguments as ``calc_paths`` followed by ``calc_vel_profile``."""
        pi, keep1 = self._pack_paths_in(prev_actions, t_now, vehicles, zone_gids)
        vi, keep2 = self._pack_vel_in(pos_est, vel_est, **vel_kwargs)
        self._check(self._fn("tape_append")(self.handle, C.byref(pi), C.byref(vi)))

    @staticmethod
    def _machine_tables(vi, tables, idx, keep):
        """Machine limits per planner (ABI v6): ``tables`` = list of (rows, 2) arrays [v, ax], ``idx`` = table of every planner. One table:
        the plain form (ax_max_machines / n_ax_max_machines); several: stacked back to back with row offsets and the per-planner index."""
        f64, i32 = np.float64, np.int32
        tabs = [np.ascontiguousarray(np.asarray(t, f64).reshape(-1, 2)) for t in tables]
        stacked = np.ascontiguousarray(np.concatenate(tabs))
        vi.ax_max_machines, vi.n_ax_max_machines = stacked.ctypes.data, stacked.shape[0]
        keep.append(stacked)
        if len(tabs) > 1:
            off = np.ascontiguousarray(np.concatenate(([0], np.cumsum([t.shape[0] for t in tabs]))).astype(i32))
            ti = np.ascontiguousarray(np.asarray(idx, i32).reshape(-1))
            vi.n_ax_tables, vi.ax_table_off, vi.ax_table_idx = len(tabs), off.ctypes.data, ti.ctypes.data
            keep += [off, ti]
        else:
            vi.n_ax_tables, vi.ax_table_off, vi.ax_table_idx = 0, None, None

    def pack_groups(self, groups, ax_max_machines=((100.0, 5.0),)):
        """Input structs of one tick for planners that come in GROUPS with identical inputs (vectorised: no Python loop over planners).
        ``groups``: list of (count, dict) in planner order; dict keys: prev_action (name), t_now, vehicles [(radius, vel, positions)],
        zone_gids, pos_est, vel_est, vel_max, gg_scale, local_gg (ax, ay), safety_d, incl_emerg_traj. Returns (paths struct, velocity struct,
        keep-alive): pass the structs to ``calc_paths_packed`` / ``calc_vel_profile_packed`` / ``tape_append_packed``."""
        if sum(c for c, _ in groups) != self.n_scen:
            raise ValueError("pack_groups: the group sizes must add up to the number of planners")
        i32, f64 = np.int32, np.float64
        acts, ts, veh_cnt, pos_cnt, rad, vel, px, py, zcnt, zg = [], [], [], [], [], [], [], [], [], []
        vcols = [[] for _ in range(8)]
        emerg = []
        for cnt, g in groups:
            a = g["prev_action"]
            acts.append(np.full(cnt, KEY_IDS.get(a, _capi.ACT_NONE) if isinstance(a, str) else _capi.ACT_NONE, i32))
            ts.append(np.full(cnt, float(g["t_now"]), f64))
            vs = g["vehicles"]
            veh_cnt.append(np.full(cnt, len(vs), np.int64))
            pc = np.array([len(v[2]) for v in vs], np.int64)
            pos_cnt.append(np.tile(pc, cnt))
            rad.append(np.tile(np.array([float(v[0]) for v in vs], f64), cnt))
            vel.append(np.tile(np.array([float(v[1]) for v in vs], f64), cnt))
            pp = np.concatenate([np.asarray(v[2], f64).reshape(-1, 2) for v in vs]) if vs else np.zeros((0, 2))
            px.append(np.tile(pp[:, 0], cnt)); py.append(np.tile(pp[:, 1], cnt))
            z = np.asarray(sorted(set(int(q) for q in (g.get("zone_gids") or []))), i32)
            zcnt.append(np.full(cnt, len(z), np.int64)); zg.append(np.tile(z, cnt))
            lg = g.get("local_gg", (5.0, 5.0))
            if type(lg) not in (tuple, list) or len(lg) != 2:
                raise ValueError("Provided local_gg does not satisfy requested format! Read parameter documentation.")
            vals = (g["pos_est"][0], g["pos_est"][1], g["vel_est"], g.get("vel_max", 100.0), g.get("gg_scale", 1.0), lg[0], lg[1],
                    g.get("safety_d", 30.0))
            for k in range(8):
                vcols[k].append(np.full(cnt, float(vals[k]), f64))
            emerg.append(np.full(cnt, int(bool(g.get("incl_emerg_traj", False))), i32))

        def cat(lst, dt, pad):
            a = np.concatenate(lst).astype(dt) if lst else np.zeros(0, dt)
            return np.ascontiguousarray(a if a.size else np.full(1, pad, dt))

        def csr(counts):
            c = np.concatenate(counts) if counts else np.zeros(0, np.int64)
            return np.ascontiguousarray(np.concatenate(([0], np.cumsum(c))).astype(i32))
        arrs = dict(prev_action=cat(acts, i32, -1), t_now=cat(ts, f64, 0.0), veh_off=csr(veh_cnt), pos_off=csr(pos_cnt),
                    veh_radius=cat(rad, f64, 0.0), veh_vel=cat(vel, f64, 0.0), pos_x=cat(px, f64, 0.0), pos_y=cat(py, f64, 0.0),
                    zone_off=csr(zcnt), zone_gid=cat(zg, i32, 0))
        pi = PlannerPathsIn()
        for k, a in arrs.items():
            setattr(pi, k, a.ctypes.data)
        v = [cat(c, f64, 0.0) for c in vcols]
        em = cat(emerg, i32, 0)
        vi = PlannerVelIn()
        for name, a in zip(("pos_est_x", "pos_est_y", "vel_est", "vel_max", "gg_scale", "gg_ax", "gg_ay", "safety_d"), v):
            setattr(vi, name, a.ctypes.data)
        vi.incl_emerg_traj = em.ctypes.data
        vi.gg_row_off, vi.gg_rows = None, None
        # machine limits: the call's table, or -- a fleet of different cars -- a table per group (key "ax_max_machines" of the group)
        tables, tab_idx, keep_t = [], [], []
        for cnt, g in groups:
            t = np.asarray(g.get("ax_max_machines", ax_max_machines), f64).reshape(-1, 2)
            k = next((i for i, u in enumerate(tables) if u.shape == t.shape and np.array_equal(u, t)), None)
            if k is None:
                tables.append(t); k = len(tables) - 1
            tab_idx.append(np.full(cnt, k, i32))
        Fleet._machine_tables(vi, tables, np.concatenate(tab_idx), keep_t)
        return pi, vi, (arrs, v, em, keep_t)

    def pack_arrays(self, prev_action, t_now, veh_off, pos_off, veh_radius, veh_vel, pos_x, pos_y, zone_off, zone_gid,
                    pos_est, vel_est, vel_max=100.0, gg_scale=1.0, local_gg=(5.0, 5.0), safety_d=30.0, incl_emerg_traj=False,
                    ax_max_machines=((100.0, 5.0),), ax_tables=None, ax_table_idx=None, gg_row_off=None, gg_rows=None):
        """Input structs of one tick from the caller's own arrays (a simulator that holds its vehicles as arrays): the layout of
        ``ltpl_planner_paths_in`` / ``ltpl_planner_vel_in`` (include/ltpl_hip.h) -- ``prev_action`` action ids (LTPL_ACT_*) per planner,
        CSR offsets ``veh_off`` [n + 1] / ``pos_off`` [n_veh + 1] / ``zone_off`` [n + 1], own position of a vehicle first. Scalars are
        broadcast; ``vel_max`` may be an array (one value per planner). Different cars: ``ax_tables`` = list of machine tables and
        ``ax_table_idx`` = the table of every planner (instead of the one table ``ax_max_machines``). Location dependent friction (local_gg as a
        dict, OTH.py:649-666): ``gg_rows`` (rows, 2) = [ax, ay] per path coordinate and ``gg_row_off`` [n * 4 + 1] = the rows of planner p's
        k-th path key are gg_row_off[4 p + k] .. gg_row_off[4 p + k + 1] (none: that key drives with the constant ``local_gg``). Returns (paths struct, velocity struct,
        keep-alive) like ``pack_groups``."""
        n, i32, f64 = self.n_scen, np.int32, np.float64

        def arr(a, dt, size=None, pad=None):
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dt), (size,)) if size is not None else np.asarray(a, dt).reshape(-1))
            return a if a.size else np.full(1, pad if pad is not None else 0, dt)
        pe = np.asarray(pos_est, f64).reshape(-1, 2)
        if pe.shape[0] == 1:
            pe = np.broadcast_to(pe, (n, 2))
        if pe.shape[0] != n:
            raise ValueError("pos_est: one (x, y) per planner expected")
        arrs = dict(prev_action=arr(prev_action, i32, n), t_now=arr(t_now, f64, n), veh_off=arr(veh_off, i32), pos_off=arr(pos_off, i32),
                    veh_radius=arr(veh_radius, f64), veh_vel=arr(veh_vel, f64), pos_x=arr(pos_x, f64), pos_y=arr(pos_y, f64),
                    zone_off=arr(zone_off, i32), zone_gid=arr(zone_gid, i32))
        if arrs["veh_off"].size != n + 1 or arrs["zone_off"].size != n + 1 or arrs["pos_off"].size != int(arrs["veh_off"][-1]) + 1:
            raise ValueError("pack_arrays: veh_off / zone_off need n + 1 entries, pos_off one more than the number of vehicles")
        pi = PlannerPathsIn()
        for k, a in arrs.items():
            setattr(pi, k, a.ctypes.data)
        if type(local_gg) not in (tuple, list) or len(local_gg) != 2:
            raise ValueError("Provided local_gg does not satisfy requested format! Read parameter documentation.")
        v = [np.ascontiguousarray(pe[:, 0]), np.ascontiguousarray(pe[:, 1]), arr(vel_est, f64, n), arr(vel_max, f64, n), arr(gg_scale, f64, n),
             arr(local_gg[0], f64, n), arr(local_gg[1], f64, n), arr(safety_d, f64, n)]
        em = arr(np.asarray(incl_emerg_traj).astype(i32), i32, n)
        vi = PlannerVelIn()
        for name, a in zip(("pos_est_x", "pos_est_y", "vel_est", "vel_max", "gg_scale", "gg_ax", "gg_ay", "safety_d"), v):
            setattr(vi, name, a.ctypes.data)
        vi.incl_emerg_traj = em.ctypes.data
        vi.gg_row_off, vi.gg_rows = None, None
        keep_t = []
        if gg_row_off is not None or gg_rows is not None:
            go = np.ascontiguousarray(np.asarray(gg_row_off, i32).reshape(-1))
            gr = np.ascontiguousarray(np.asarray(gg_rows, f64).reshape(-1, 2))
            if go.size != n * _capi.PLANNER_MAX_KEYS + 1 or gr.shape[0] < int(go[-1]):
                raise ValueError("pack_arrays: gg_row_off needs n * %d + 1 entries and gg_rows gg_row_off[-1] rows" % _capi.PLANNER_MAX_KEYS)
            if gr.shape[0] == 0:
                gr = np.zeros((1, 2))
            vi.gg_row_off, vi.gg_rows = go.ctypes.data, gr.ctypes.data
            keep_t += [go, gr]
        if ax_tables is not None:
            if ax_table_idx is None or len(np.asarray(ax_table_idx).reshape(-1)) != n:
                raise ValueError("pack_arrays: ax_table_idx needs one entry per planner")
            Fleet._machine_tables(vi, list(ax_tables), ax_table_idx, keep_t)
        else:
            Fleet._machine_tables(vi, [ax_max_machines], None, keep_t)
        return pi, vi, (arrs, v, em, keep_t)

    def calc_paths_packed(self, pi):
        """``calc_paths`` on an input struct of ``pack_groups`` (a caller that already holds its fleet's inputs as arrays pays no packing)."""
        self._check(self._fn("calc_paths")(self.handle, C.byref(pi)))

    def calc_vel_profile_packed(self, vi):
        self._check(self._fn("calc_vel_profile")(self.handle, C.byref(vi)))

    def tape_append_groups(self, groups, ax_max_machines=((100.0, 5.0),)):
        """Inputs of one tick for planners that come in groups with identical inputs (see ``pack_groups``)."""
        pi, vi, keep = self.pack_groups(groups, ax_max_machines)
        self._check(self._fn("tape_append")(self.handle, C.byref(pi), C.byref(vi)))

    def tape_append_packed(self, pi, vi):
        """Append the input structs of ``pack_groups`` / ``pack_arrays`` (both calls of one tick) to the tape."""
        self._check(self._fn("tape_append")(self.handle, C.byref(pi), C.byref(vi)))

    DIGEST_DOUBLES = 8 + 9 * _capi.PLANNER_MAX_KEYS

    def digest(self):
        """Digest of EVERY planner's last tick, computed on the device (ltpl_fleet_digest): array [n_planners, DIGEST_DOUBLES] --
        [0] error word, [1] cut_index_pos, [2] cut_layer, [3] n_keys, [4] n_ids, [5] vel_plan, [6] n_vel_course, [7] acc_plan, per key k:
        [8 + 7 k ..] key id, trajectory id, rows, s_end, vx[0], vx[-1], sum(vx); per id k: [8 + 7 K + 2 k ..] key id, id value.
        ``tick_replay.check_digests`` compares it with a tick of a recording for all planners at once."""
        out = np.zeros((self.n_scen, self.DIGEST_DOUBLES), np.float64)
        self._check(self._fn("digest")(self.handle, out.ctypes.data_as(C.POINTER(C.c_double)), int(self.DIGEST_DOUBLES)))
        return out

    def tape_run(self, first, count):
        """Advance all planners through ticks [first, first + count) of the tape; returns the device time in ms."""
        ms = C.c_float(0.0)
        self._check(self._fn("tape_run")(self.handle, int(first), int(count), C.byref(ms)))
        return float(ms.value)

    # ---- closed-loop simulation on the device -------------------------------------------------------------------------------------
    def sim_setup(self, race, planners, t0=1.0e6, tic0=None, dt=0.05, n_export=115):
        """The example driver's loop around every planner (ltpl_fleet_sim_setup). ``race``: ``sim.RaceLineTable`` (or its [n, 5] rows).
        ``planners``: one dict per planner -- ``opponents`` [(s0, vel_scale, length)], ``static`` [(x, y, theta, v, length)],
        ``pref`` action names in order of preference (1 .. 5, 'emergency' allowed), ``pos_est`` (x, y), ``vel_est``, ``zone_gids``.
        The opponents' previous call is at ``tic0`` (default ``t0``)."""
        if len(planners) != self.n_scen:
            raise ValueError("sim_setup: one entry per planner expected")
        f64, i32 = np.float64, np.int32
        rows = np.ascontiguousarray(np.asarray(race.rows() if hasattr(race, "rows") else race, f64).reshape(-1, 5))

        def csr(lists):
            return np.ascontiguousarray(np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(i32))

        def col(lists, c, dt_=f64):
            a = np.array([row[c] for x in lists for row in x], dt_)
            return np.ascontiguousarray(a if a.size else np.zeros(1, dt_))
        opp = [list(p.get("opponents", ())) for p in planners]
        sta = [list(p.get("static", ())) for p in planners]
        pref = [[KEY_IDS[a] if isinstance(a, str) else int(a) for a in p["pref"]] for p in planners]
        zones = [sorted(set(int(g) for g in (p.get("zone_gids") or ()))) for p in planners]
        arrs = dict(race=rows, opp_off=csr(opp), opp_s0=col(opp, 0), opp_vel_scale=col(opp, 1), opp_length=col(opp, 2),
                    static_off=csr(sta), static_x=col(sta, 0), static_y=col(sta, 1), static_theta=col(sta, 2), static_v=col(sta, 3),
                    static_length=col(sta, 4), pref_off=csr(pref),
                    pref_action=np.ascontiguousarray(np.array([a for x in pref for a in x] or [0], i32)),
                    pos_est_x=np.ascontiguousarray(np.array([float(p["pos_est"][0]) for p in planners], f64)),
                    pos_est_y=np.ascontiguousarray(np.array([float(p["pos_est"][1]) for p in planners], f64)),
                    vel_est=np.ascontiguousarray(np.array([float(p.get("vel_est", 0.0)) for p in planners], f64)),
                    zone_off=csr(zones), zone_gid=np.ascontiguousarray(np.array([g for z in zones for g in z] or [0], i32)))
        si = SimIn()
        for k, a in arrs.items():
            setattr(si, k, a.ctypes.data)
        si.n_rl, si.t0, si.tic0, si.dt, si.n_export = rows.shape[0], float(t0), float(t0 if tic0 is None else tic0), float(dt), int(n_export)
        self._check(self._fn("sim_setup")(self.handle, C.byref(si)))
        self._sim_opp, self._sim_export = int(arrs["opp_off"][-1]), int(n_export)
        self._sim_pref_off = arrs["pref_off"].astype(np.int64)      # (sim_selector_read sizes and splits the ordered lists with it)
        self._sim_event_order = np.zeros(0, np.int64)       # (sim_setup switches the events off)

    def sim_vel(self, ax_tables=None, ax_table_idx=None, **vel_kwargs):
        """Velocity arguments of the following ``sim_run`` calls (keywords of ``calc_vel_profile`` without pos_est / vel_est, scalars or one
        value per planner; ``ax_tables`` + ``ax_table_idx``: a machine table per planner). local_gg as a dict is not supported: location dependent grip comes from a map
        on the device (``friction``)."""
        vi, keep = self._pack_vel_in([(0.0, 0.0)] * self.n_scen, 0.0, **vel_kwargs)
        if ax_tables is not None:
            keep = [keep]
            Fleet._machine_tables(vi, ax_tables, ax_table_idx, keep)
        self._check(self._fn("sim_vel")(self.handle, C.byref(vi)))

    def sim_run(self, n_ticks, trace=True):
        """``n_ticks`` closed-loop ticks back to back on the device (ltpl_fleet_sim_run). Returns (trace, ms): trace [n_ticks, n_planners,
        SIM_TRACE_DOUBLES] -- sel action, t_now, pos_est x / y, vel_est, on-track vehicles, first vehicle X / Y, then the tick's digest row
        (``digest``) -- or None with ``trace=False``. A failing planner raises BackendError after the run (``last_trace`` keeps the trace)."""
        out = np.zeros((int(n_ticks), self.n_scen, SIM_TRACE_DOUBLES), np.float64) if trace else None
        ms = C.c_float(0.0)
        rc = self._fn("sim_run")(self.handle, int(n_ticks), None if out is None else out.ctypes.data, SIM_TRACE_DOUBLES, C.byref(ms))
        self.last_trace, self.last_ms = out, float(ms.value)
        self._check(rc)
        return out, float(ms.value)

    def sim_race(self, races, length=5.0, heading0=None):
        """Planners that see one another (ltpl_fleet_sim_race; after ``sim_setup``, refused after the first ``sim_run``). ``races``: sizes
        summing to the number of planners, or ranges of consecutive planners covering them all in order. Every other planner of a race
        is an object of a planner's list, behind its opponents and statics: the pose, speed and heading its tracker wrote this tick, with
        ``length`` (scalar or one per planner). ``heading0`` (scalar or one per planner; default: the heading given to ``set_start``) is a
        planner's heading until its first trajectory."""
        n = self.n_scen
        races = list(races)
        if races and all(isinstance(r, range) for r in races):
            if [q for r in races for q in r] != list(range(n)) or any(r.step != 1 for r in races):
                raise ValueError("sim_race: the ranges must cover the planners 0 .. n - 1 in order")
            sizes = [len(r) for r in races]
        else:
            sizes = [int(r) for r in races]
        self._set("sim_race", SimRaceIn, (("race_off", _offsets(sizes), np.int32, len(sizes) + 1), ("length", length, np.float64),
                                          ("heading0", self._start_heading() if heading0 is None else heading0, np.float64)), n_races=len(sizes))

    def sim_heading(self):
        """[n] heading of every planner's tracked pose (``sim_race``'s heading0 until its first trajectory)."""
        out = np.zeros(self.n_scen, np.float64)
        self._check(self._fn("sim_heading")(self.handle, out.ctypes.data))
        return out

    # ---- race telemetry on the device ---------------------------------------------------------------------------------------------
    def sim_telemetry(self, radius=2.5, grid_s=None):
        """(Re)starts the race telemetry of the following ``sim_run`` calls (ltpl_fleet_sim_telemetry; after ``sim_setup``, between runs
        at any time): a record per planner, accumulated on the device in every tick the planner is live. ``radius``: contact radius
        (scalar or one per planner; None switches the telemetry off); ``grid_s``: progress offset of every planner (default: s of its
        first live tick; hand it in for grids that straddle the start line)."""
        if radius is None:
            return self._set("sim_telemetry")
        self._set("sim_telemetry", SimTeleIn, (("radius", radius, np.float64), ("grid_s", grid_s, np.float64))[:1 if grid_s is None else 2])

    def sim_telemetry_read(self):
        """The records as they stand (ltpl_fleet_sim_telemetry_read; accumulation goes on): dict of named arrays, one entry per planner
        (``TELEMETRY_FIELDS``: counts as int64, ``act`` [n, 5] in the order straight, follow, left, right, emergency), plus
        ``track_length``, the closed length of the race line. BackendError while the telemetry is off."""
        length = C.c_double(0.0)
        return telemetry_dict(self._read("sim_telemetry_read", TELEMETRY_DOUBLES, C.byref(length)), float(length.value))

    # ---- flight recorder on the device ----------------------------------------------------------------------------------------------
    def sim_record(self, planners, depth=1):
        """(Re)starts the flight recorder of the following ``sim_run`` calls (ltpl_fleet_sim_record; after ``sim_setup``, between runs at
        any time): for the ``planners`` (distinct indices, any order) the device keeps a full record of each of the last ``depth`` ticks.
        ``planners=None`` switches the recorder off. Tick indices count from this call on."""
        if planners is None:
            self._check(self._fn("sim_record")(self.handle, None, 0, int(depth)))
            return
        idx = np.ascontiguousarray(np.asarray(list(planners), np.int64).reshape(-1).astype(np.int32))
        self._check(self._fn("sim_record")(self.handle, idx.ctypes.data if idx.size else None, int(idx.size), int(depth)))

    def sim_record_info(self):
        """dict(n_planners, depth, first_tick, n_ticks): the ring holds the fleet ticks first_tick .. first_tick + n_ticks - 1."""
        v = [C.c_int32(0) for _ in range(4)]
        self._check(self._fn("sim_record_info")(self.handle, *[C.byref(x) for x in v]))
        return dict(zip(("n_planners", "depth", "first_tick", "n_ticks"), (int(x.value) for x in v)))

    def sim_record_read(self, first=None, count=None):
        """The held ticks (``first`` .. ``first + count - 1``; default: all of them), oldest first: a list over ticks of lists over the
        recorded planners in the order given to ``sim_record``. Every element is a dict -- ``tick``, ``planner``, ``error`` (error word, 0:
        none), ``sel`` (action name), ``t_now``, ``pos_est``, ``vel_est``, ``heading``, ``vehicles`` [(radius, vel, positions (2, 2))] as
        ``calc_paths`` takes them, ``paths`` (``start_node``, ``keys``, ``nodes``, ``n_rows``, ``red_len``, ``const_rows``,
        ``closest_obj_index`` named as by ``paths()``, plus ``const_path_seg``: (const_rows, 2) array or None), taken between the tick's
        calc_paths and its velocity stage, and ``traj``: the triple of ``trajectories()`` with rows trimmed to n_export and no vel_course.
        ``TickLogWriter.write_sim_record`` turns such a dict into a row of the reference's tick log."""
        info = self.sim_record_info()
        first = info["first_tick"] if first is None else int(first)
        count = info["first_tick"] + info["n_ticks"] - first if count is None else int(count)
        head, pv, tv = SimRecordHead(), PathsView(), self._tv
        obj = np.zeros((SIM_RECORD_OBJECTS, 6))
        cxy = np.zeros((self.cap_rows, 2))
        for k in range(_capi.PLANNER_MAX_KEYS):
            pv.nodes[k] = self._pv.nodes[k]                # (path_param, coeff and node_idx are not recorded: no buffers)
        vc, tv.vel_course = tv.vel_course, None
        get = self._fn("sim_record_get")
        out = []
        try:
            for t in range(first, first + count):
                row = []
                for m in range(info["n_planners"]):
                    self._check(get(self.handle, t, m, C.byref(head), obj.ctypes.data, C.byref(pv), cxy.ctypes.data, C.byref(tv)))
                    row.append(self._record_dict(head, obj, pv, cxy, tv))
                out.append(row)
        finally:
            tv.vel_course = vc
        return out

    def _record_dict(self, head, obj, pv, cxy, tv):
        nk = pv.n_keys
        key_id, n_rows, n_nodes, red = pv.key_id[:nk], pv.n_rows[:nk], pv.n_nodes[:nk], pv.red_len[:nk]
        coi = pv.closest_obj_index
        paths = {"keys": [], "nodes": {}, "n_rows": {}, "red_len": {}, "start_node": pv.start_node[:2], "const_rows": pv.const_rows,
                 "closest_obj_index": None if coi < 0 else coi, "const_path_seg": None}
        for k in range(nk):
            name = KEY_NAMES[key_id[k]]
            nodes = self._nd[k][:n_nodes[k]].tolist()
            if nodes and nodes[0][0] < 0:                   # the start spline's pseudo node [None, None] (OTH.py:267)
                nodes = [[None if a < 0 else a, None if b < 0 else b] for a, b in nodes]
            paths["keys"].append(name)
            paths["nodes"][name], paths["n_rows"][name], paths["red_len"][name] = nodes, n_rows[k], bool(red[k])
        if pv.const_rows >= 0 and nk:
            paths["const_path_seg"] = cxy[:min(pv.const_rows, n_rows[0])].copy()
        nb, ni, ne = tv.n_keys, tv.n_ids, self._sim_export
        traj = {KEY_NAMES[tv.key_id[k]]: [self._tr[k][:min(tv.n_rows[k], ne)].copy()] for k in range(nb)}
        ids = {KEY_NAMES[tv.id_key[k]]: tv.id_val[k] for k in range(ni)}
        ref = {"cut_index_pos": tv.cut_index_pos, "cut_layer": tv.cut_layer, "vel_plan": tv.vel_plan, "acc_plan": tv.acc_plan,
               "vel_course": np.zeros(0)}
        veh = [(float(obj[i, 0]), float(obj[i, 1]), obj[i, 2:6].reshape(2, 2).copy()) for i in range(head.n_objects)]
        return {"tick": head.tick, "planner": head.planner, "error": head.error, "sel": KEY_NAMES.get(head.sel_action),
                "t_now": head.t_now, "pos_est": [head.pos_x, head.pos_y], "vel_est": head.vel_est, "heading": head.heading,
                "vehicles": veh, "paths": paths, "traj": (traj, ids, ref)}

    # ---- snapshot and branch on the device ------------------------------------------------------------------------------------------
    def sim_snapshot(self, slot=0, planners=None):
        """Copies the simulation state of the ``planners`` (distinct indices; default: all) into snapshot slot ``slot`` (0 ..
        SIM_SNAPSHOTS - 1) on the device, replacing what the slot held (ltpl_fleet_sim_snapshot; after ``sim_setup``, before or after
        runs). State is what the tick kernels write: a planner's memory with its error word, its friction-row window, clock, action,
        tracked pose, speed and heading, its opponents' positions, with telemetry on its record and with ``sim_tracker`` set its track
        table and next id (the tracker's parameters and statistics stay the destination's). What the caller set
        (preference lists, opponents' speeds, statics, zones, ``sim_vel`` arguments, friction maps, races, the recorder) is no part of it.
        ``sim_setup`` drops every snapshot; ``sim_telemetry`` invalidates their telemetry part."""
        if planners is None:
            self._check(self._fn("sim_snapshot")(self.handle, int(slot), None, 0))
            return
        idx = np.ascontiguousarray(np.asarray(list(planners), np.int64).reshape(-1).astype(np.int32))
        if idx.size == 0:
            raise ValueError("sim_snapshot: an empty planner list (None: all planners)")
        self._check(self._fn("sim_snapshot")(self.handle, int(slot), idx.ctypes.data, int(idx.size)))

    def sim_snapshot_info(self, slot):
        """dict(planners: int32 array in the order given to ``sim_snapshot``, bytes: device memory of the slot), or None for an empty slot."""
        n, b = C.c_int32(0), C.c_uint64(0)
        self._check(self._fn("sim_snapshot_info")(self.handle, int(slot), C.byref(n), None, 0, C.byref(b)))
        if n.value == 0:
            return None
        idx = np.zeros(n.value, np.int32)
        self._check(self._fn("sim_snapshot_info")(self.handle, int(slot), C.byref(n), idx.ctypes.data, int(idx.size), None))
        return dict(planners=idx, bytes=int(b.value))

    def sim_snapshot_drop(self, slot):
        """Frees snapshot slot ``slot`` (ltpl_fleet_sim_snapshot_drop)."""
        self._check(self._fn("sim_snapshot_drop")(self.handle, int(slot)))

    def sim_branch(self, src, dst, snapshot=None):
        """Planner ``dst[k]`` of the live fleet takes the state of planner ``src[k]`` (ltpl_fleet_sim_branch) -- of the live fleet, or of
        snapshot slot ``snapshot``, which must hold it. A scalar ``src`` is broadcast over ``dst`` (fan-out of one situation into a bank
        of planners with other ``vel_max`` / grip / machine tables). The configuration stays the destination's own (``sim_snapshot``), so
        both planners of a pair need the same number of opponents; ``dst`` entries are distinct; with the live fleet as source no planner
        is both a source and a destination (a pair ``src == dst`` is skipped). The error word travels: a healthy source revives a
        failed planner. Returns the device time of the copy in ms."""
        d = np.ascontiguousarray(np.asarray(dst, np.int64).reshape(-1).astype(np.int32))
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(src, np.int64).reshape(-1), d.shape).astype(np.int32))
        ms = C.c_float(0.0)
        self._check(self._fn("sim_branch")(self.handle, -1 if snapshot is None else int(snapshot), s.ctypes.data if s.size else None,
                                           d.ctypes.data if d.size else None, int(d.size), C.byref(ms)))
        return float(ms.value)

    def sim_restore(self, slot):
        """Every planner of snapshot ``slot`` back to the state the snapshot holds (``sim_branch`` with src == dst == the slot's planners).
        Returns the device time of the copy in ms."""
        info = self.sim_snapshot_info(slot)
        if info is None:
            raise ValueError("sim_restore: snapshot slot %d is empty" % int(slot))
        return self.sim_branch(info["planners"], info["planners"], snapshot=slot)

    # ---- scripted events on the device ----------------------------------------------------------------------------------------------
    def sim_events(self, events):
        """Sets the event list of the following ``sim_run`` calls (ltpl_fleet_sim_events; after ``sim_setup``, between runs at any time):
        a list of ``sim.Event`` -- a condition (a schedule tick, an opponent within a distance, the speed below / above a value, a delay
        after another event) and one write into the planner's configuration (an opponent's vel_scale / length, a static object, an entry
        of the preference list, an argument of ``sim_vel``, the grip factor on the friction map). Executed on the device at the head of
        every tick, each event at most once; the schedule tick counts the ticks run since this call. ``None`` (or an empty list)
        switches the events off, and so does ``sim_setup``."""
        events = list(events) if events is not None else []
        if not events:
            self._check(self._fn("sim_events")(self.handle, None))
            self._sim_event_order = np.zeros(0, np.int64)
            return
        a = sim_pack_events(events, self.n_scen)
        ei = SimEventsIn()
        ei.n_events = len(events)
        for k in ("ev_off", "when_kind", "when_index", "when_value", "set_kind", "set_index", "set_value"):
            setattr(ei, k, a[k].ctypes.data)
        self._check(self._fn("sim_events")(self.handle, C.byref(ei)))
        self._sim_event_order = a["order"]

    def sim_events_read(self):
        """dict(fired_tick: int32 array, one entry per event in the order of the list given to ``sim_events`` -- the schedule tick in
        which it fired, -1: not yet; tick: the schedule tick, i.e. the ticks run since ``sim_events``)."""
        n, tick = C.c_int32(0), C.c_int32(0)
        self._check(self._fn("sim_events_read")(self.handle, None, C.byref(n), C.byref(tick)))
        packed = np.full(max(n.value, 1), -1, np.int32)
        if n.value:
            self._check(self._fn("sim_events_read")(self.handle, packed.ctypes.data, None, None))
        order = getattr(self, "_sim_event_order", np.zeros(0, np.int64))
        if len(order) != n.value:                          # (a list set through the C entry point itself: the library's order, planner by planner)
            order = np.arange(n.value)
        out = np.full(n.value, -1, np.int32)
        if n.value:
            out[order] = packed[:n.value]
        return dict(fired_tick=out, tick=int(tick.value))

    # ---- seeded sensor noise on the device --------------------------------------------------------------------------------------------
    def sim_noise(self, seed=None, pos=0.0, vel=0.0, obj_pos=0.0, obj_theta=0.0, obj_vel=0.0, tick0=0):
        """Localisation and perception errors of the following ``sim_run`` calls (ltpl_fleet_sim_noise; after ``sim_setup``, between runs
        at any time). ``seed``: 64-bit seed (scalar or one per planner; None switches the noise off); standard deviations, scalars or one
        per planner: ``pos`` [m] and ``vel`` [m/s] of the planner's own estimate, ``obj_pos`` [m], ``obj_theta`` [rad], ``obj_vel`` [m/s]
        of every opponent, static object and mate it perceives. A sigma of 0 draws nothing. ``tick0``: the noise tick of the next tick
        to run (draws depend on seed, tick, object and component only: ``sim.noise_gauss``, ``sim.NoiseModel``)."""
        if seed is None:
            return self._set("sim_noise")
        sigmas = (("sigma_pos", pos), ("sigma_vel", vel), ("sigma_obj_pos", obj_pos), ("sigma_obj_theta", obj_theta), ("sigma_obj_vel", obj_vel))
        self._set("sim_noise", SimNoiseIn, (("seed", seed, np.uint64),) + tuple((k, v, np.float64) for k, v in sigmas), tick0=int(tick0))

    def sim_estimate(self):
        """dict(pos_est [n, 2], vel_est [n]): what every planner was handed as its pose and speed in the last tick
        (ltpl_fleet_sim_estimate); the true state of ``sim_state`` while the noise is off."""
        x, y, v = (np.zeros(self.n_scen, np.float64) for _ in range(3))
        self._check(self._fn("sim_estimate")(self.handle, x.ctypes.data, y.ctypes.data, v.ctypes.data))
        return dict(pos_est=np.column_stack((x, y)), vel_est=v)

    def sim_noise_draws(self, seed, tick, obj, comp, words=False):
        """g(seed, tick, obj, comp) for arrays of tuples (they broadcast), evaluated on the device (ltpl_fleet_sim_noise_draws); equals
        ``sim.noise_gauss`` bit for bit. ``words=True``: returns (g, [n, 12] uint32 output words of the generator)."""
        a = np.broadcast_arrays(np.asarray(seed, np.uint64), np.asarray(tick, np.uint32), np.asarray(obj, np.uint32), np.asarray(comp, np.uint32))
        sd, tk, ob, cp = (np.ascontiguousarray(v.reshape(-1)) for v in a)
        n = int(sd.size)
        g = np.zeros(n, np.float64)
        w = _zeros(n, 12, dtype=np.uint32) if words else None
        self._check(self._fn("sim_noise_draws")(self.handle, sd.ctypes.data, tk.ctypes.data, ob.ctypes.data, cp.ctypes.data, n, g.ctypes.data,
                                                None if w is None else w.ctypes.data))
        return (g, w[:n]) if words else g

    # ---- vehicle model on the device ------------------------------------------------------------------------------------------------
    def sim_vehicle(self, model=1, keep_state=False, **params):
        """A car between the planned trajectory and the pose of the next tick (ltpl_fleet_sim_vehicle; after ``sim_setup`` -- and after
        ``sim_race`` where its heading0 matters --, between runs at any time). ``model``: 0 the ideal tracker, 1 the vehicle model (scalar
        or one per planner; None switches the model off); ``params``: keywords of ``sim.VEHICLE_DEFAULTS`` (scalars or one per planner;
        ``ctl_steps``: one integer). The state of every planner with model 1 starts from its present true pose, speed and heading with
        a = kappa = 0 and cleared statistics; ``keep_state=True``: planners that already drove the model keep state and statistics and
        only the parameters change (a grip that drops between two runs). Host mirror: ``sim.VehicleModel``."""
        if model is None:
            return self._set("sim_vehicle")
        unknown = set(params) - set(VEHICLE_DEFAULTS)
        if unknown:
            raise TypeError("sim_vehicle: unknown parameter(s) %s" % sorted(unknown))
        par = dict(VEHICLE_DEFAULTS, **params)
        self._set("sim_vehicle", SimVehicleIn, (("model", model, np.int32),) + tuple((k, par[k], np.float64) for k in VEHICLE_PARAMS),
                  ctl_steps=int(par["ctl_steps"]), flags=1 if keep_state else 0)

    def sim_vehicle_read(self, raw=False):
        """dict of named arrays (``sim.VEHICLE_FIELDS``): state x, y, c, s, v, a, kappa and statistics e, e_max, e2_sum, dv_max, ctl_steps,
        sat_lat, sat_lon, off_track_ticks of every planner (ltpl_fleet_sim_vehicle_read). A planner on the ideal tracker holds NaN (its
        counters read -1). ``raw=True``: the [n, 15] records."""
        out = self._read("sim_vehicle_read", VEHICLE_DOUBLES)
        return out if raw else vehicle_dict(out)

    def sim_vehicle_step(self, state, params, rows, dt, ctl_steps):
        """The model's test hook (ltpl_fleet_sim_vehicle_step): one tick of independent cases on the device, one wave each. ``state``
        [m, 7]; ``params`` [m, 9] in the order of ``sim.VEHICLE_PARAMS``; ``rows``: a list of m arrays [n_q, 5] = s, x, y, vx, ax
        (0 .. 256 rows); ``dt``, ``ctl_steps``: scalars or one per case. Returns (records [m, 15]: the state after the tick and the
        tick's statistics, theta [m]); equals ``sim.VehicleModel.tick`` bit for bit."""
        state = np.ascontiguousarray(np.asarray(state, np.float64).reshape(-1, 7))
        m = state.shape[0]
        params = _per(params, np.float64, (m, len(VEHICLE_PARAMS)))
        off, flat = _ragged(rows, 5)
        if len(off) - 1 != m:
            raise ValueError("sim_vehicle_step: one row table per case expected")
        dts, ctl = _per(dt, np.float64, m), _per(ctl_steps, np.int32, m)
        out, theta = _zeros(m, VEHICLE_DOUBLES), _zeros(m)
        self._check(self._fn("sim_vehicle_step")(self.handle, m, state.ctypes.data, params.ctypes.data, off.ctypes.data, flat.ctypes.data,
                                                 dts.ctypes.data, ctl.ctypes.data, out.ctypes.data, VEHICLE_DOUBLES, theta.ctypes.data))
        return out[:m], theta[:m]

    # ---- sensor model on the device ---------------------------------------------------------------------------------------------------
    def sim_sensor(self, range=float("inf"), fov_deg=360.0, r_near=0.0, occl=0.0, p_drop=0.0, seed=None, tick0=0):
        """Which of the tick's on-track objects every planner is shown (ltpl_fleet_sim_sensor; after ``sim_setup``, between runs at any
        time): a ``range`` [m], a forward cone of the FULL opening angle ``fov_deg`` (exactly 360: no cone), an all-round near field
        ``r_near`` inside which cone and occlusion do not apply, occlusion by nearer objects with their radii scaled by ``occl`` (0: off)
        and a dropout probability ``p_drop`` per object and tick drawn from ``seed`` (scalars or one per planner; ``seed=None``: 0).
        ``tick0``: the sensor tick of the next tick. ``range=None`` switches the sensor off. The statistics start anew with every
        call. Host mirror: ``sim.SensorModel``."""
        if range is None:
            return self._set("sim_sensor")
        val = dict(range=range, r_near=r_near, fov_cos=sensor_fov_cos(fov_deg), occl=occl, p_drop=p_drop)
        self._set("sim_sensor", SimSensorIn, tuple((k, val[k], np.float64) for k in SENSOR_PARAMS) + (("seed", 0 if seed is None else seed, np.uint64),),
                  tick0=int(tick0))

    def sim_sensor_read(self, raw=False):
        """dict of named arrays (``sim.SENSOR_FIELDS``): live ticks, objects on the track, seen, lost to range / cone / occlusion / dropout,
        ticks with a lost object, the smallest true clearance to a lost object and its sensor tick, of every planner
        (ltpl_fleet_sim_sensor_read). ``raw=True``: the [n, 10] records."""
        out = self._read("sim_sensor_read", SENSOR_DOUBLES)
        return out if raw else sensor_dict(out)

    def sim_sensor_eval(self, pose, f, params, seed, tick, objs):
        """The sensor's test hook (ltpl_fleet_sim_sensor_eval): independent cases on the device, one wave each. ``pose`` [m, 2]; ``f``
        [m, 2] the forward vector as given; ``params`` [m, 5] in the order of ``sim.SENSOR_PARAMS``; ``seed``, ``tick``: scalars or one
        per case; ``objs``: a list of m arrays [n_q, 3] = x, y, r (0 .. 96 rows). Returns (causes, u): per case an int32 array (0 seen,
        1 .. 4 the cause of loss) and the dropout draws (NaN where none was made); equals ``sim.SensorModel.evaluate`` bit for bit."""
        pose = np.asarray(pose, np.float64).reshape(-1, 2)
        m = pose.shape[0]
        pf = np.ascontiguousarray(np.concatenate((pose, _per(f, np.float64, (m, 2))), axis=1))
        params = _per(params, np.float64, (m, len(SENSOR_PARAMS)))
        seeds, ticks = _per(seed, np.uint64, m), _per(tick, np.uint32, m)
        off, flat = _ragged(objs, 3)
        if len(off) - 1 != m:
            raise ValueError("sim_sensor_eval: one object list per case expected")
        cause, u = np.zeros(flat.shape[0], np.int32), np.zeros(flat.shape[0], np.float64)
        self._check(self._fn("sim_sensor_eval")(self.handle, m, pf.ctypes.data, params.ctypes.data, seeds.ctypes.data, ticks.ctypes.data,
                                                off.ctypes.data, flat.ctypes.data, cause.ctypes.data, u.ctypes.data))
        return _split(cause, off), _split(u, off)

    # ---- object tracker on the device -------------------------------------------------------------------------------------------------
    def sim_tracker(self, gate=TRACKER_DEFAULTS["gate"], w_pos=TRACKER_DEFAULTS["w_pos"], w_vel=TRACKER_DEFAULTS["w_vel"],
                    n_confirm=TRACKER_DEFAULTS["n_confirm"], n_coast=TRACKER_DEFAULTS["n_coast"], tick0=0):
        """A multi-object tracker per planner between the staged object list (behind ``sim_sensor``) and the planner
        (ltpl_fleet_sim_tracker; after ``sim_setup``, between runs at any time): detections are associated with predicted tracks inside
        ``gate`` [m] (greedy nearest neighbour), a matched track is filtered with the prediction's weights ``w_pos`` / ``w_vel`` in
        [0, 1), a new track is handed on from its ``n_confirm``-th detection, a confirmed track that is lost is coasted on for up to
        ``n_coast`` ticks (scalars or one per planner). ``tick0``: the tracker tick of the next tick. ``gate=None`` switches the tracker
        off. Tables and statistics start anew with every call. Host mirror: ``sim.TrackerModel``."""
        if gate is None:
            return self._set("sim_tracker")
        val = dict(gate=gate, w_pos=w_pos, w_vel=w_vel, n_confirm=n_confirm, n_coast=n_coast)
        self._set("sim_tracker", SimTrackerIn, tuple((k, val[k], np.int32 if k.startswith("n_") else np.float64) for k in TRACKER_PARAMS),
                  tick0=int(tick0))

    def sim_tracker_read(self, planners=None, raw=False):
        """The tracker's statistics of every planner as a dict of named arrays (``sim.TRACKER_FIELDS``; ``raw=True``: the [n, 12] records)
        (ltpl_fleet_sim_tracker_read). With ``planners`` (a list of indices): (records, tables, counts) -- their track tables
        [len(planners), 96, 10] in the order of ``sim.TRACK_FIELDS``, unused rows NaN, and their track counts."""
        if planners is None:
            out = self._read("sim_tracker_read", TRACKER_DOUBLES, 0, None, None, None)
            return out if raw else tracker_dict(out)
        sel = np.ascontiguousarray(np.asarray(planners, np.int32).reshape(-1))
        tabs, cnt = _zeros(len(sel), TRACK_CAP, TRACK_DOUBLES), _zeros(len(sel), dtype=np.int32)
        out = self._read("sim_tracker_read", TRACKER_DOUBLES, len(sel), sel.ctypes.data, tabs.ctypes.data, cnt.ctypes.data)
        return (out if raw else tracker_dict(out)), tabs[:len(sel)], cnt[:len(sel)]

    def sim_tracker_eval(self, params, adv, tick, cap, slots, tracks, next_id, dets):
        """The tracker's test hook (ltpl_fleet_sim_tracker_eval): independent cases on the device, one wave each, one tick each.
        ``params`` [m, 5] in the order of ``sim.TRACKER_PARAMS``; ``adv``, ``tick``, ``cap``, ``slots``, ``next_id``: scalars or one per
        case; ``tracks``: a list of m arrays [T_q, 10]; ``dets``: a list of m arrays [K_q, 6] = x, y, px, py, r, v. Returns a dict:
        ``tables`` [m, 96, 10] (unused rows NaN), ``n_tracks`` [m], ``next_id`` [m], ``out`` (a list of [n_out_q, 6] arrays), ``assign`` (a
        list of int32 arrays: matched id, -1 born, -2 overflow), ``rec`` [m, 12]; equals ``sim.TrackerModel.step`` bit for bit."""
        (toff, tflat), (doff, dflat) = _ragged(tracks, TRACK_DOUBLES), _ragged(dets, 6)
        m = len(toff) - 1
        if len(doff) - 1 != m:
            raise ValueError("sim_tracker_eval: one table and one detection list per case expected")
        params = _per(params, np.float64, (m, len(TRACKER_PARAMS)))
        adv, tick, nid = _per(adv, np.float64, m), _per(tick, np.uint32, m), _per(next_id, np.float64, m)
        cs = np.ascontiguousarray(np.stack((_per(cap, np.int32, m), _per(slots, np.int32, m)), axis=1))
        tabs, ntr, nid_out = _zeros(m, TRACK_CAP, TRACK_DOUBLES), _zeros(m, dtype=np.int32), _zeros(m)
        out, n_out, rec = _zeros(m, TRACK_CAP, 6), _zeros(m, dtype=np.int32), _zeros(m, TRACKER_DOUBLES)
        assign = np.zeros(dflat.shape[0], np.int32)
        self._check(self._fn("sim_tracker_eval")(self.handle, m, params.ctypes.data, adv.ctypes.data, tick.ctypes.data, cs.ctypes.data, toff.ctypes.data,
                                                 tflat.ctypes.data, nid.ctypes.data, doff.ctypes.data, dflat.ctypes.data, tabs.ctypes.data,
                                                 ntr.ctypes.data, nid_out.ctypes.data, out.ctypes.data, n_out.ctypes.data, assign.ctypes.data,
                                                 rec.ctypes.data))
        return dict(tables=tabs[:m], n_tracks=ntr[:m], next_id=nid_out[:m], out=[out[q, :n_out[q]].copy() for q in range(m)],
                    assign=_split(assign, doff), rec=rec[:m])

    # ---- prediction model on the device -----------------------------------------------------------------------------------------------
    def sim_predictor(self, n_points=PREDICTOR_DEFAULTS["n_points"], mode=PREDICTOR_DEFAULTS["mode"], horizon=PREDICTOR_DEFAULTS["horizon"],
                      relax=PREDICTOR_DEFAULTS["relax"], d_max=PREDICTOR_DEFAULTS["d_max"]):
        """A multi-point prediction of every object a planner is handed, behind ``sim_sensor`` and ``sim_tracker`` and in front of the
        path kernel (ltpl_fleet_sim_predictor; after ``sim_setup``, between runs at any time): every object reaches the planner with its
        own position and ``n_points`` (1 .. 8, fleet-wide) predicted points over ``horizon`` [s] instead of the ingestion's single 0.2 s
        point. ``mode`` 0: as ingested (the planner computes what it computes without a predictor), 1: straight line, 2: along the race
        line at the object's lateral offset, of which the share ``relax`` in [0, 1] is given up by the last point; an object further than
        ``d_max`` [m] from the race line, or moving against it, is predicted straight (scalars or one per planner). The planner takes its
        closest object from a vehicle's LAST position, so with a long horizon a ``follow`` job may follow another car. Refused
        (LTPL_ERR_CAPACITY) unless (opponents + statics + mates) (1 + n_points) <= 192 for every planner. ``n_points=None`` switches the
        predictor off. The statistics start anew with every call. Host mirror: ``sim.PredictorModel``."""
        if n_points is None:
            return self._set("sim_predictor")
        val = dict(mode=mode, horizon=horizon, relax=relax, d_max=d_max)
        self._set("sim_predictor", SimPredictorIn, tuple((k, val[k], np.int32 if k == "mode" else np.float64) for k in PREDICTOR_PARAMS),
                  n_points=int(n_points))

    def sim_predictor_read(self, raw=False):
        """dict of named arrays (``sim.PREDICTOR_FIELDS``): live ticks, objects predicted, a count per outcome (as ingested, still,
        straight by mode / ``d_max`` / direction / without a segment, along the track), the largest lateral offset used and the points
        that wrapped (ltpl_fleet_sim_predictor_read). ``raw=True``: the [n, 11] records."""
        out = self._read("sim_predictor_read", PREDICTOR_DOUBLES)
        return out if raw else predictor_dict(out)

    def sim_predictor_eval(self, n_points, params, objs):
        """The predictor's test hook (ltpl_fleet_sim_predictor_eval): independent cases on the device, one wave each, on the race-line
        table of ``sim_setup``. ``params`` [m, 4] in the order of ``sim.PREDICTOR_PARAMS``; ``objs``: a list of m arrays [n_q, 5] = x, y,
        px, py, v (at most 96 rows). Returns (positions, outcomes, rec): per case the [n_q, 1 + n_points, 2] positions (own, then the
        points) and the int32 outcomes, and the [m, 11] counters; equals ``sim.PredictorModel`` bit for bit."""
        off, flat = _ragged(objs, 5)
        m, K = len(off) - 1, int(n_points)
        params = _per(params, np.float64, (m, len(PREDICTOR_PARAMS)))
        pts = np.zeros((flat.shape[0], 1 + max(K, 1), 2))
        oc, rec = np.zeros(flat.shape[0], np.int32), _zeros(m, PREDICTOR_DOUBLES)
        self._check(self._fn("sim_predictor_eval")(self.handle, m, K, params.ctypes.data, off.ctypes.data, flat.ctypes.data, pts.ctypes.data,
                                                   oc.ctypes.data, rec.ctypes.data))
        return _split(pts, off), _split(oc, off), rec[:m]

    # ---- behaviour selector on the device ---------------------------------------------------------------------------------------------
    def sim_selector(self, on=True, **params):
        """A behaviour selector per planner (ltpl_fleet_sim_selector; after ``sim_setup``, between runs at any time): at the head of every
        tick the trajectories of the previous exported set are scored against the objects the planner was handed -- pace over ``horizon``
        [s], minus ``w_clear`` per metre of clearance (ego radius ``r_ego``) under ``c_soft``, minus ``w_switch`` for leaving the previous
        action; an action whose clearance falls below ``c_hard`` is unsafe -- and the step walks the ORDERED list: safe actions by score,
        emergency if listed, unsafe ones by clearance, the rest. The user's preference list stays the allowed set and the tie order and
        is never written. Parameters (``sim.SELECTOR_PARAMS``, defaults ``sim.SELECTOR_DEFAULTS``) and ``on``: scalars or one per planner.
        ``on=None`` switches the selector off. The statistics start anew with every call. Host mirror: ``sim.SelectorModel``."""
        if on is None:
            return self._set("sim_selector")
        unknown = set(params) - set(SELECTOR_PARAMS)
        if unknown:
            raise ValueError("sim_selector: unknown parameter %s" % sorted(unknown))
        val = dict(SELECTOR_DEFAULTS, **params)
        self._set("sim_selector", SimSelectorIn, (("on", on, np.int32),) + tuple((k, val[k], np.float64) for k in SELECTOR_PARAMS))

    def sim_selector_read(self, raw=False):
        """(records, ordered): the dict of named arrays (``sim.SELECTOR_FIELDS``; ``raw=True``: the [n, 12] records) and the current
        ordered list of every planner, a list of int32 arrays in the order of the preference lists of ``sim_setup``
        (ltpl_fleet_sim_selector_read)."""
        off = getattr(self, "_sim_pref_off", np.zeros(self.n_scen + 1, np.int64))
        order = _zeros(off[-1], dtype=np.int32)
        out = self._read("sim_selector_read", SELECTOR_DOUBLES, order.ctypes.data, int(off[-1]))
        return (out if raw else selector_dict(out)), _split(order, off)

    def sim_selector_eval(self, params, users, sel_prev, actions, objs, emergency=None, rec=None):
        """The selector's test hook (ltpl_fleet_sim_selector_eval): independent cases on the device, one wave each. ``params`` [m, 6] in
        the order of ``sim.SELECTOR_PARAMS``; per case: ``users`` the preference list, ``sel_prev``, ``actions`` four entries (None: not
        exported, else rows [n, 4] = s, x, y, vx), ``objs`` [n_q, 5] = x, y, px, py, r, ``emergency`` exported or not; ``rec`` [m, 12]: the
        records before (default: fresh ones). Returns (ordered lists, act_d [m, 4, 3] = vbar, clear, J, act_i [m, 4, 2] = clear_obj, flags,
        records after); equals ``sim.SelectorModel.evaluate`` bit for bit."""
        m = len(users)
        R = SELECTOR_MAX_ROWS
        params = _per(params, np.float64, (m, len(SELECTOR_PARAMS)))
        lists = _zeros(m, 8, dtype=np.int32)
        n_rows = np.full((max(m, 1), 4), -1, np.int32)
        rows = _zeros(m, 4, 4, R)
        off, flat = _ragged(objs, 5)
        for q in range(m):
            u = [int(a) for a in users[q]]
            lists[q, 0], lists[q, 1], lists[q, 2] = len(u), int(sel_prev[q]), int(bool(emergency[q])) if emergency is not None else 0
            lists[q, 3:3 + min(len(u), 5)] = u[:5]
            for a in range(4):
                if actions[q][a] is None:
                    continue
                t = np.asarray(actions[q][a], np.float64).reshape(-1, 4)
                n_rows[q, a] = t.shape[0]
                rows[q, a, :, :min(t.shape[0], R)] = t[:R].T
        order, act_d, act_i = _zeros(m, 5, dtype=np.int32), _zeros(m, 4, 3), _zeros(m, 4, 2, dtype=np.int32)
        if rec is None:
            rec = _zeros(m, SELECTOR_DOUBLES)
            rec[:, 10] = np.inf
        rec = np.ascontiguousarray(np.asarray(rec, np.float64).reshape(max(m, 1), SELECTOR_DOUBLES).copy())
        self._check(self._fn("sim_selector_eval")(self.handle, m, params.ctypes.data, lists.ctypes.data, n_rows.ctypes.data, rows.ctypes.data,
                                                  off.ctypes.data, flat.ctypes.data, order.ctypes.data, act_d.ctypes.data, act_i.ctypes.data,
                                                  rec.ctypes.data))
        return [order[q, :lists[q, 0]].copy() for q in range(m)], act_d[:m], act_i[:m], rec[:m]

    # ---- safety monitor on the device -------------------------------------------------------------------------------------------------
    def sim_safety(self, on=True, tick0=0, keep_state=False, **params):
        """A safety monitor per planner (ltpl_fleet_sim_safety; after ``sim_setup``, between runs at any time): every live tick the staged
        objects -- in front of sensor and tracker, at their true positions -- are measured against the true pose and its displacement since
        the previous live tick: time to collision, required deceleration, time headway, gap and closing speed, accumulated into a 31-double
        record (``sim.SAFETY_FIELDS``) and a ring of the last 8 incidents (``sim.INCIDENT_FIELDS``; an incident: consecutive evaluated ticks
        with TTC under ``ttc_thr``). Measurement only: the run is bit-identical with and without it. Parameters (``sim.SAFETY_PARAMS``,
        defaults ``sim.SAFETY_DEFAULTS``) and ``on``: scalars or one per planner; ``tick0``: the monitor's tick of the next fleet tick.
        ``keep_state=True`` changes parameters, mask and tick0 and keeps records and rings. ``on=None`` clears the monitor. Host mirror:
        ``sim.SafetyModel``."""
        if on is None:
            return self._set("sim_safety")
        unknown = set(params) - set(SAFETY_PARAMS)
        if unknown:
            raise ValueError("sim_safety: unknown parameter %s" % sorted(unknown))
        val = dict(SAFETY_DEFAULTS, **params)
        self._set("sim_safety", SimSafetyIn, (("on", on, np.int32),) + tuple((k, val[k], np.float64) for k in SAFETY_PARAMS),
                  tick0=int(tick0), flags=SAFETY_KEEP_STATE if keep_state else 0)

    def sim_safety_read(self, raw=False):
        """(records, incidents): the dict of named arrays (``sim.SAFETY_FIELDS``; ``raw=True``: the [n, 31] records) and the incident rings
        [n, 8, 6] (``sim.INCIDENT_FIELDS``; NaN: unwritten; ``sim.safety_incidents`` orders a ring) (ltpl_fleet_sim_safety_read)."""
        inc = np.zeros((self.n_scen, SAFETY_INCIDENTS, INCIDENT_DOUBLES), np.float64)
        out = self._read("sim_safety_read", SAFETY_DOUBLES, inc.ctypes.data, INCIDENT_DOUBLES)
        return (out if raw else safety_dict(out)), inc

    def sim_safety_eval(self, pose, dt, tick, params, objs, rec=None, inc=None):
        """The monitor's test hook (ltpl_fleet_sim_safety_eval): independent cases on the device, one wave and one live tick each.
        ``pose`` [m, 2], ``dt`` [m], ``tick`` [m], ``params`` [m, 5] in the order of ``sim.SAFETY_PARAMS``; per case ``objs`` [n_q, 5] = x,
        y, px, py, r; ``rec`` [m, 31] and ``inc`` [m, 8, 6]: records and rings before (default: the start state). Returns (records after,
        rings after, per_obj: a list of [n_q, 6] = ttc, drac, thw, gap, closing, flags, per_tick [m, 8]); equals ``sim.safety_tick`` bit
        for bit."""
        off, flat = _ragged(objs, 5)
        m = len(off) - 1
        k = max(m, 1)
        pose, dt, tick = _per(pose, np.float64, (m, 2)), _per(dt, np.float64, m), _per(tick, np.int32, m)
        params = _per(params, np.float64, (m, len(SAFETY_PARAMS)))
        r0, i0 = safety_start(k)
        rec = r0 if rec is None else np.ascontiguousarray(np.asarray(rec, np.float64).reshape(k, SAFETY_DOUBLES).copy())
        inc = i0 if inc is None else np.ascontiguousarray(np.asarray(inc, np.float64).reshape(k, SAFETY_INCIDENTS, INCIDENT_DOUBLES).copy())
        per_obj, per_tick = np.zeros((flat.shape[0], 6)), np.zeros((k, 8))
        self._check(self._fn("sim_safety_eval")(self.handle, m, pose.ctypes.data, dt.ctypes.data, tick.ctypes.data, params.ctypes.data,
                                                off.ctypes.data, flat.ctypes.data, rec.ctypes.data, inc.ctypes.data, per_obj.ctypes.data,
                                                per_tick.ctypes.data))
        return rec[:m], inc[:m], _split(per_obj, off), per_tick[:m]

    # ---- reactive opponents on the device ----------------------------------------------------------------------------------------------
    def sim_react(self, on=True, tick0=0, keep_state=False, **params):
        """Opponents that react to the car ahead (ltpl_fleet_sim_react; after ``sim_setup``, between runs at any time): at the head of
        every tick each race-line opponent gets an EFFECTIVE vel_scale in [0, its configured one] from the car ahead of it on the race
        line -- another opponent of the planner or the ego (its TRUE pose and speed, within ``lat_gate`` of the line) -- by the
        car-following rule of csrc/fleet_react.hpp, and the tick integrates the race-line speed times that scale. Parameters
        (``sim.REACT_PARAMS`` without ``on``, defaults ``sim.REACT_DEFAULTS``) and ``on``: scalars or one per planner; ``tick0``: the
        model's tick of the next fleet tick. A call starts from the configured scales and fresh records; ``keep_state=True`` changes
        parameters and tick0 and keeps scales and records. ``on=None`` (or 0 for every planner) switches the model off. A field whose
        opponents never find a leader drives the run without the model bit for bit. Host mirror: ``sim.ReactModel``."""
        if on is None:
            return self._set("sim_react")
        names = REACT_PARAMS[1:]                           # (``on`` travels apart, as int32)
        unknown = set(params) - set(names)
        if unknown:
            raise ValueError("sim_react: unknown parameter %s" % sorted(unknown))
        val = dict(REACT_DEFAULTS, **params)
        self._set("sim_react", SimReactIn, (("on", on, np.int32),) + tuple((k, val[k], np.float64) for k in names),
                  tick0=int(tick0), flags=REACT_KEEP_STATE if keep_state else 0)

    def sim_react_read(self, raw=False):
        """(records, eff_scale): the dict of named arrays (``sim.REACT_FIELDS``; ``raw=True``: the [n, 16] records) and the effective
        scales of all opponents in the order of ``sim_state()['opp_s']`` (ltpl_fleet_sim_react_read)."""
        no = getattr(self, "_sim_opp", 0)
        eff = _zeros(no)
        out = self._read("sim_react_read", REACT_DOUBLES, eff.ctypes.data)
        return (out if raw else react_dict(out)), eff[:no]

    def sim_react_eval(self, params, ego, dt, tick, opp, rec=None):
        """The rule's test hook (ltpl_fleet_sim_react_eval; needs ``sim_setup``, for the race table): independent cases on the device,
        one wave and one tick each. ``params`` [m, 9] in the order of ``sim.REACT_PARAMS``, ``ego`` [m, 3] = x, y, v, ``dt`` [m],
        ``tick`` [m]; per case ``opp`` [n_q, 4] = s, c, e, length (0 .. 96); ``rec`` [m, 16]: the records before (default: the start
        state). Returns (records after, e_new: a list of [n_q], per_opp: a list of [n_q, 4] = leader, delta, gap, acc, ego_out [m, 3] =
        s_e, d_e, has); equals ``sim.react_tick`` bit for bit."""
        off, flat = _ragged(opp, 4)
        m = len(off) - 1
        k = max(m, 1)
        params, ego = _per(params, np.float64, (m, len(REACT_PARAMS))), _per(ego, np.float64, (m, 3))
        dt, tick = _per(dt, np.float64, m), _per(tick, np.int32, m)
        rec = react_start(k) if rec is None else np.ascontiguousarray(np.asarray(rec, np.float64).reshape(k, REACT_DOUBLES).copy())
        e_out, per_opp, ego_out = np.zeros(flat.shape[0]), np.zeros((flat.shape[0], 4)), np.zeros((k, 3))
        self._check(self._fn("sim_react_eval")(self.handle, m, params.ctypes.data, ego.ctypes.data, dt.ctypes.data, tick.ctypes.data,
                                               off.ctypes.data, flat.ctypes.data, rec.ctypes.data, e_out.ctypes.data, per_opp.ctypes.data,
                                               ego_out.ctypes.data))
        return rec[:m], _split(e_out, off), _split(per_opp, off), ego_out[:m]

    # ---- campaign statistics on the device ---------------------------------------------------------------------------------------------
    def sim_stats(self, groups, measures=None, top_k=0, period=0, depth=0, tick0=0, keep_series=False, n_groups=None):
        """A statistics plan (ltpl_fleet_sim_stats; after ``sim_setup``, between runs at any time): ``groups`` [n] gives every planner its
        group, -1 .. G - 1 (-1: none; G = ``n_groups`` or the largest index + 1); ``measures``: a list of (family, field, lo, hi, bins,
        top_dir) -- a family of ``sim.STATS_FAMILIES`` whose module is on (or ``"state"`` with its field ``"failed"``), a field of the
        family's ``*_FIELDS`` table (``"act[2]"`` for an element; or the column), the histogram's range and 1 .. 16 cells, and -1 / 0 / +1
        for a list of the ``top_k`` (0 .. 8) smallest / no / largest planners. ``sim_stats_reduce`` reduces on demand; with ``period`` > 0
        ``sim_run`` reduces at the tail of every tick with (tick0 + ticks since this call + 1) % period == 0 into a ring of ``depth``
        rows (``sim_stats_series``). ``keep_series=True`` keeps the ring of a plan with the same G, number of measures and depth.
        ``groups=None`` clears the plan. Measurement only: the run is bit-identical with and without it. Host mirror: ``sim.StatsModel``."""
        if groups is None:
            self._set("sim_stats")
            self._sim_stats = None
            return
        i32, f64 = np.int32, np.float64
        group = _per(groups, i32, self.n_scen)
        G = (int(group.max()) + 1 if group.size else 0) if n_groups is None else int(n_groups)
        cols = [stats_column(m[0], m[1]) for m in measures]
        M = len(cols)
        per_measure = (("family", [c[0] for c in cols], i32), ("column", [c[1] for c in cols], i32), ("lo", [m[2] for m in measures], f64),
                       ("hi", [m[3] for m in measures], f64), ("bins", [m[4] for m in measures], i32), ("top_dir", [m[5] for m in measures], i32))
        self._set("sim_stats", SimStatsIn, (("group", group, i32),) + tuple(c + (M,) for c in per_measure), n_groups=G, n_measures=M,
                  top_k=int(top_k), period=int(period), depth=int(depth), tick0=int(tick0), flags=STATS_KEEP_SERIES if keep_series else 0)
        self._sim_stats = (G, M, int(top_k), int(depth) if int(period) > 0 else 0)

    def _stats_shape(self):
        shape = getattr(self, "_sim_stats", None)
        return shape if shape is not None else (1, 1, 0, 0)      # (no plan: the call below refuses)

    def sim_stats_reduce(self, raw=True):
        """(rows [G, M, 27], tops [G, M, top_k, 2] = value, planner) of the plan, reduced now on the device from the planners' records
        (ltpl_fleet_sim_stats_reduce; ``sim.STATS_FIELDS``; ``raw=False``: the rows as ``sim.stats_dict``). Unused list entries are
        (NaN, -1)."""
        G, M, K, _ = self._stats_shape()
        tops = np.zeros((G, M, max(K, 1), 2), np.float64)
        rows = self._read("sim_stats_reduce", STATS_DOUBLES, tops.ctypes.data if K else None, K, rows=(G, M))
        return (rows if raw else stats_dict(rows)), tops[:, :, :K]

    def sim_stats_series(self):
        """(ticks [held], rows [held, G, M, 27], rows ever written): the ring of the plan's series, oldest first
        (ltpl_fleet_sim_stats_series)."""
        G, M, _, depth = self._stats_shape()
        ticks, rows = _zeros(depth, dtype=np.int32), _zeros(depth, G, M, STATS_DOUBLES)
        held, total = C.c_int32(0), C.c_int64(0)
        self._check(self._fn("sim_stats_series")(self.handle, ticks.ctypes.data, rows.ctypes.data, STATS_DOUBLES, C.byref(held), C.byref(total)))
        return ticks[:held.value].copy(), rows[:held.value].copy(), int(total.value)

    def sim_stats_eval(self, values, spec, planners=None):
        """The rule's test hook (ltpl_fleet_sim_stats_eval): independent cases on the device, each one group and one measure on raw values.
        Per case ``values`` [n_q] and ``spec`` = (lo, hi, bins, top_dir, top_k); ``planners`` (or None: the positions): per case the
        planner index of every value. Returns (rows [m, 27], tops [m, 8, 2]); equals ``sim.stats_reduce`` bit for bit."""
        off, flat = _ragged(values)
        m = len(off) - 1
        spec = np.ascontiguousarray(np.asarray(spec, np.float64).reshape(m, 5))
        idx = None if planners is None else _ragged(planners)[1].astype(np.int32)
        rows, tops = _zeros(m, STATS_DOUBLES), _zeros(m, STATS_MAX_TOP, 2)
        self._check(self._fn("sim_stats_eval")(self.handle, m, off.ctypes.data, flat.ctypes.data, None if idx is None else idx.ctypes.data,
                                               spec.ctypes.data, rows.ctypes.data, tops.ctypes.data))
        return rows[:m], tops[:m]

    # ---- friction maps on the device ------------------------------------------------------------------------------------------------
    def friction(self, maps, map_idx=None, scale=1.0):
        """Location dependent grip from maps resident on the device (ltpl_fleet_friction; local_gg as a dict, OTH.py:633-666). ``maps``:
        a ``friction.FrictionGrid`` or a list of them (empty / None: clears the maps); ``map_idx``: the map of every planner (scalar or one
        per planner, -1: the planner keeps its constant ``local_gg`` tuple; default: map 0 for all); ``scale``: grip factor per planner.
        A planner with a map takes the rows of every offered key from the map on every route of the velocity stage
        (``calc_vel_profile``, ``tape_run``, ``sim_run`` with or without races); between ticks or runs at any time."""
        f64, i32 = np.float64, np.int32
        if maps is None:
            maps = []
        elif hasattr(maps, "rows"):
            maps = [maps]
        maps = list(maps)
        cols = ()
        if maps:
            k = len(maps)
            nodes = np.concatenate([m.nodes() for m in maps])
            cols = tuple((a, [getattr(m, a) for m in maps], f64, k) for a in ("x0", "y0", "dx", "dy"))
            cols += tuple((a, [getattr(m, a) for m in maps], i32, k) for a in ("nx", "ny"))
            cols += (("node_off", _offsets([m.nx * m.ny for m in maps]), i32, k + 1), ("nodes", nodes, f64, nodes.shape),
                     ("map_idx", 0 if map_idx is None else map_idx, i32), ("scale", scale, f64))
        self._set("friction", FrictionIn, cols, n_maps=len(maps))

    def friction_scale(self, scale):
        """New grip factors (scalar or one per planner) on the maps set by ``friction`` (ltpl_fleet_friction_scale)."""
        sc = _per(scale, np.float64, self.n_scen)
        self._check(self._fn("friction_scale")(self.handle, sc.ctypes.data))

    def friction_rows(self, map, xy, scale=1.0):
        """[n, 2] = [ax, ay] of map ``map`` at the points ``xy`` [n, 2] times ``scale``, evaluated on the device
        (ltpl_fleet_friction_rows); equals ``FrictionGrid.rows`` bit for bit."""
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        x, y = np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])
        out = np.zeros((xy.shape[0], 2), np.float64)
        self._check(self._fn("friction_rows")(self.handle, int(map), x.ctypes.data, y.ctypes.data, int(xy.shape[0]), float(scale),
                                              out.ctypes.data))
        return out

    def sim_state(self):
        """Simulation state: dict of pos_est [n, 2], vel_est, sel_action (ids), now, opponent s / tic (all opponents in planner order)."""
        n, no = self.n_scen, getattr(self, "_sim_opp", 0)
        px, py, v, now = (np.zeros(n, np.float64) for _ in range(4))
        sel = np.zeros(n, np.int32)
        os_, ot = _zeros(no), _zeros(no)
        self._check(self._fn("sim_state")(self.handle, px.ctypes.data, py.ctypes.data, v.ctypes.data, sel.ctypes.data, now.ctypes.data,
                                          os_.ctypes.data, ot.ctypes.data))
        return dict(pos_est=np.column_stack((px, py)), vel_est=v, sel_action=sel, now=now, opp_s=os_[:no], opp_tic=ot[:no])
