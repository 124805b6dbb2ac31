"""
TEST INFRASTRUCTURE (no test functions): the fleet's closed-loop simulation (ltpl_fleet_sim_setup / _race / _vel / _run,
csrc/fleet_sim.hpp) restated as a plain host loop for ARBITRARY scenarios, out of parts the project already pins to the reference:

  opponents, ego tracker, heading, mates   graphbasedlocaltrajectoryplanner_amd/sim.py (bit for bit against the recordings:
                                           tests/test_sim_host.py, tests/test_sim_race_host.py)
  object ingestion                         OracleBackend.process_objects (the oracle's plain C)
  the planner                              passed in: anything with the interface of planner.Planner and ONE planner per object
                                           (oracle/planner_host.py: the host state machine over the oracle's arithmetic)

``HostSimLoop`` takes the ``planners`` dicts of ``Fleet.sim_setup`` and the ``races`` of ``Fleet.sim_race``. A tick has two halves, in
the order of the device (k_fleet_sim_step for every planner, then k_fleet_sim_mates, then the fleet's tick):

  ``step_sim()``    per planner: clock; action = first preferred key of the previous exported set ('straight' before the first tick);
                    opponents; statics appended; ingestion (survivors in list order); tracker on the previous trajectory of the selected
                    action trimmed to n_export rows; heading
  ``step_plan()``   per planner of a race, after EVERY tracker: the mates through the same ingestion, behind the own survivors; then
                    calc_paths / calc_vel_profile (``want_paths``: the planner's paths as they stand after BOTH calls, i.e. with the
                    memory already trimmed to the tick's cut layer -- a device fleet's tick cannot be read in between)

Failure semantics of the device: a planner without a matching action fails alone, takes no objects, keeps its state and stays in its
mates' lists there; a planner whose calc_paths / calc_vel_profile raises stays failed from that tick on.

Free running, the loop carries its own state (``tick()``). Seated, one tick is computed from a state handed in (``seat()`` before
``step_sim()``: clock, pose, speed, heading, the opponents' s / tic and the trajectories of the tick before; ``step_plan(post=...)``:
the state AFTER the step, so that mates and planner see exactly what the other side's planner sees).

Further down: the digest row of a tick computed on the host (``trace_rows``: what ``Fleet.sim_run`` returns as its trace) and the seeded
scenario classes shared by tests/test_sim_loop_host.py (which asserts that they reach their edges) and
tests/test_gpu_sim_differential.py (which runs the device through them).
"""
import math

import numpy as np

from graphbasedlocaltrajectoryplanner_amd import _capi, sim
from graphbasedlocaltrajectoryplanner_amd._capi import BackendError
from graphbasedlocaltrajectoryplanner_amd.fleet import SIM_TRACE_DOUBLES
from graphbasedlocaltrajectoryplanner_amd.planner import KEY_IDS

PRED_DT = 0.2                 # ObjectListInterface.py:121
K = _capi.PLANNER_MAX_KEYS


class HostSimLoop(object):
    def __init__(self, lat, race, planners, planner_objs, oracle=None, t0=1.0e6, tic0=None, dt=0.05, n_export=115):
        """``race``: sim.RaceLineTable; ``planners``: the dicts of ``Fleet.sim_setup``; ``planner_objs``: one planner object (n_scen = 1)
        per entry; ``oracle``: OracleBackend of ``lat`` (made here if not given)."""
        if oracle is None:
            from oracle.oracle_lib import OracleBackend
            oracle = OracleBackend(lat)
        assert len(planners) == len(planner_objs)
        self.lat, self.oracle, self.tab, self.lists = lat, oracle, race, race.lists()
        self.dt, self.n_export = float(dt), int(n_export)
        self.n = len(planners)
        self.pl = list(planner_objs)
        tic0 = t0 if tic0 is None else tic0
        self.cfg = []
        for e in planners:
            pref = [a if isinstance(a, str) else _capi.ACTION_NAMES[a] for a in e["pref"]]
            self.cfg.append(dict(opp=[tuple(float(v) for v in o) for o in e.get("opponents", ())],
                                 static=[tuple(float(v) for v in s) for s in e.get("static", ())], pref=pref,
                                 zones=sorted(set(int(g) for g in (e.get("zone_gids") or ())))))
        self.now = [float(t0)] * self.n
        self.sel = [None] * self.n
        self.started = [False] * self.n
        self.pos = [[float(e["pos_est"][0]), float(e["pos_est"][1])] for e in planners]
        self.vel = [float(e.get("vel_est", 0.0)) for e in planners]
        self.theta = [0.0] * self.n                      # (sim_setup: zero until sim_race hands in heading0)
        self.opp_s = [[o[0] for o in c["opp"]] for c in self.cfg]
        self.opp_tic = [[float(tic0)] * len(c["opp"]) for c in self.cfg]
        self.traj = [None] * self.n                      # previous exported set {key: [rows]}
        self.failed = [False] * self.n
        self.velkw = [dict() for _ in range(self.n)]
        self.race_of = [[h] for h in range(self.n)]
        self.length = [5.0] * self.n
        self._heading = [0.0] * self.n
        self._live, self._rec = [False] * self.n, [None] * self.n

    # ---- setup ------------------------------------------------------------------------------------------------------------------
    def set_start(self, h, pos, heading, vel=0.0, max_heading_offset=math.pi / 4):
        self._heading[h] = float(heading)
        return self.pl[h].set_start(0, pos, heading, vel, max_heading_offset)

    def sim_race(self, races, length=5.0, heading0=None):
        """``races``: sizes summing to the number of planners (Fleet.sim_race)."""
        sizes = [len(r) if isinstance(r, range) else int(r) for r in races]
        assert sum(sizes) == self.n
        a = 0
        for s in sizes:
            for h in range(a, a + s):
                self.race_of[h] = list(range(a, a + s))
            a += s
        self.length = [float(v) for v in np.broadcast_to(np.asarray(length, float), (self.n,))]
        h0 = self._heading if heading0 is None else np.broadcast_to(np.asarray(heading0, float), (self.n,))
        self.theta = [float(v) for v in h0]

    def sim_vel(self, h=None, **kw):
        """Velocity arguments (keywords of calc_vel_profile without pos_est / vel_est) of planner ``h`` (None: of all)."""
        for q in (range(self.n) if h is None else [h]):
            self.velkw[q] = dict(kw)

    def seat(self, h, now, pos, vel, theta, opp_s, opp_tic, traj):
        """State of planner ``h`` before a tick: ``traj`` = the exported set of the tick before ({key: [rows]}; None or empty before the
        first tick)."""
        self.now[h], self.pos[h], self.vel[h], self.theta[h] = float(now), [float(pos[0]), float(pos[1])], float(vel), float(theta)
        self.opp_s[h], self.opp_tic[h] = [float(v) for v in opp_s], [float(v) for v in opp_tic]
        self.traj[h] = traj if traj else None
        self.started[h] = bool(traj)

    # ---- a tick -----------------------------------------------------------------------------------------------------------------
    def ingest(self, rows):
        """``rows``: [x, y, theta, v, length] -> (keep mask, vehicles of calc_paths for the survivors in list order)."""
        if not rows:
            return np.zeros(0, bool), []
        a = np.asarray(rows, float).reshape(-1, 5)
        o = self.oracle.process_objects(a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4], PRED_DT)
        keep = o["on_track"].astype(bool)
        veh = [(float(o["radius"][k]), float(a[k, 3]), np.array([[a[k, 0], a[k, 1]], [o["pred_x"][k], o["pred_y"][k]]]))
               for k in range(len(rows)) if keep[k]]
        return keep, veh

    def step_sim(self):
        """First half of a tick for every planner; returns the records (dicts) the second half completes."""
        for h in range(self.n):
            c = self.cfg[h]
            rec = dict(failed=True, action_failed=False, sel=self.sel[h], now=self.now[h], objects=[], keep=np.zeros(0, bool), veh=[])
            self._rec[h], self._live[h] = rec, False
            if self.failed[h]:
                continue
            now = self.now[h] + self.dt
            keys = list(self.traj[h].keys()) if self.started[h] else ['straight']
            sel = next((a for a in c["pref"] if a in keys), None)
            if sel is None:
                self.failed[h] = True
                rec.update(action_failed=True, sel=c["pref"][-1], now=now)
                continue
            rows = []
            for q, (_, scale, length) in enumerate(c["opp"]):
                s, tic, x, y, psi, v = sim.opponent_step(self.tab, self.opp_s[h][q], self.opp_tic[h][q], now, scale, self.lists)
                self.opp_s[h][q], self.opp_tic[h][q] = s, tic
                rows.append((x, y, psi, v, length))
            rows += c["static"]
            keep, veh = self.ingest(rows)
            if self.started[h]:
                tr = np.asarray(self.traj[h][sel][0], float)[:self.n_export]
                pos, vel, s, j = sim.vdc_track(self.pos[h], tr, self.dt)
                if s is not None:
                    self.theta[h] = sim.peer_heading(s, j, tr[:, 0].tolist(), tr[:, 3].tolist())
                self.pos[h], self.vel[h] = pos, vel
                rec["traj_rows"] = int(np.asarray(self.traj[h][sel][0]).shape[0])
            self.now[h], self.sel[h], self.started[h] = now, sel, True
            self._live[h] = True
            rec.update(failed=False, sel=sel, now=now, objects=rows, keep=keep, veh=veh)
        for h in range(self.n):
            self._rec[h].update(pos=list(self.pos[h]), vel=self.vel[h], theta=self.theta[h], opp_s=list(self.opp_s[h]),
                                opp_tic=list(self.opp_tic[h]))
        return self._rec

    def step_plan(self, post=None, want_paths=False):
        """Second half. ``post``: {planner: dict(sel, now, pos, vel, theta)} replaces the state the first half left (seated runs: the
        other side's state after its own step). Returns the completed records."""
        for h, st in (post or {}).items():
            self.pos[h], self.vel[h], self.theta[h] = [float(st["pos"][0]), float(st["pos"][1])], float(st["vel"]), float(st["theta"])
            if self._live[h]:
                self.now[h], self.sel[h] = float(st["now"]), st["sel"]
        for h in range(self.n):
            rec = self._rec[h]
            rec.update(cnt=0, first=(float("nan"), float("nan")), n_mates_kept=0)
            if not self._live[h]:
                continue
            veh = list(rec["veh"])
            if len(self.race_of[h]) > 1:
                mates = sim.race_objects(h, self.race_of[h], self.pos, self.vel, self.theta, self.length)
                rows = [(o['X'], o['Y'], o['theta'], o['v'], o['length']) for o in mates]
                keep, mv = self.ingest(rows)
                rec["mates"], rec["mates_keep"], rec["n_mates_kept"] = rows, keep, len(mv)
                veh += mv
            rec["veh"], rec["cnt"] = veh, len(veh)
            if veh:
                rec["first"] = (float(veh[0][2][0, 0]), float(veh[0][2][0, 1]))
        for h in range(self.n):
            rec = self._rec[h]
            if not self._live[h]:
                continue
            pl = self.pl[h]
            try:
                pl.calc_paths([self.sel[h]], [self.now[h]], [rec["veh"]], [self.cfg[h]["zones"]])
                pl.calc_vel_profile([self.pos[h]], self.vel[h], **self.velkw[h])
                rec["traj"] = pl.trajectories(0)
                if want_paths:
                    # read BEHIND the velocity stage, which trims the path memory to the cut layer: the only place where a fleet that runs
                    # whole ticks on the device can be read, and the same state on both sides
                    rec["paths"] = pl.paths(0)
                self.traj[h] = rec["traj"][0]
            except BackendError as e:
                self.failed[h] = True
                rec.update(failed=True, error=str(e))
        return self._rec

    def tick(self, want_paths=False):
        self.step_sim()
        return [dict(r) for r in self.step_plan(want_paths=want_paths)]


def digest_row(rec):
    """``Fleet.digest()``'s row of a host record (k_fleet_digest, csrc/fleet_dev.hpp)."""
    o = np.zeros(SIM_TRACE_DOUBLES - 8)
    if rec["failed"] or "traj" not in rec:
        o[0] = 1.0
        return o
    traj, ids, ref = rec["traj"]
    o[1], o[2], o[3], o[4] = ref["cut_index_pos"], ref["cut_layer"], len(traj), len(ids)
    o[5], o[6], o[7] = ref["vel_plan"], ref["vel_course"].shape[0], ref["acc_plan"]
    for i, (k, v) in enumerate(list(traj.items())[:K]):
        r = v[0]
        n = r.shape[0]
        o[8 + 7 * i: 8 + 7 * i + 7] = [KEY_IDS[k], ids.get(k, 0), n, r[-1, 0] if n else 0.0, r[0, 5] if n else 0.0, r[-1, 5] if n else 0.0,
                                       float(np.sum(r[:, 5]))]
    for i, (k, v) in enumerate(list(ids.items())[:K]):
        o[8 + 7 * K + 2 * i], o[8 + 7 * K + 2 * i + 1] = KEY_IDS[k], v
    return o


def trace_rows(recs):
    """[n_planners, SIM_TRACE_DOUBLES]: the records of one tick in the layout of ``Fleet.sim_run``'s trace."""
    out = np.zeros((len(recs), SIM_TRACE_DOUBLES))
    for p, r in enumerate(recs):
        out[p, :8] = [KEY_IDS.get(r["sel"], _capi.ACT_NONE), r["now"], r["pos"][0], r["pos"][1], r["vel"], r["cnt"], r["first"][0], r["first"][1]]
        out[p, 8:] = digest_row(r)
    return out


# ---- seeded scenario classes ------------------------------------------------------------------------------------------------------
C2_VEL = dict(vel_max=100.0, gg_scale=1.0, local_gg=(5.0, 5.0), ax_max_machines=((100.0, 5.0),), safety_d=30.0, incl_emerg_traj=False)
DEFAULT_PREF = ("right", "left", "straight", "follow")


def race_line_pose(tab, s):
    """(pos, heading) of the race-line row nearest to arc length ``s`` (heading in (-pi, pi])."""
    i = int(np.argmin(np.abs(tab.s_rl - s)))
    psi = float(tab.psi[i])
    return (float(tab.x[i]), float(tab.y[i])), (psi - 2 * np.pi if psi > np.pi else psi)


def crowded_statics(track, n, seed, first_row=250, every=8, off_every=3, off_phase=0):
    """``n`` static objects on every ``every``-th reference-line row from ``first_row`` on: every ``off_every``-th (from ``off_phase``)
    pushed 40 m off the track along the normal, the others within +-2 m; seeded headings and speeds 0 .. 8 m/s; rows
    (x, y, theta, v, length)."""
    rng = np.random.default_rng(seed)
    ref, nv = np.asarray(track['refline'], float), np.asarray(track['normvec'], float)
    out = []
    for k in range(n):
        i = (first_row + every * k) % ref.shape[0]
        off = 40.0 if k % off_every == off_phase else float(rng.uniform(-2.0, 2.0))
        out.append((float(ref[i, 0] + nv[i, 0] * off), float(ref[i, 1] + nv[i, 1] * off), float(rng.uniform(-np.pi, np.pi)),
                    float(rng.uniform(0.0, 8.0)), 4.0))
    return out


def monteblanco_classes(tab, track, start_pos):
    """{name: dict(entry (Fleet.sim_setup), vel (calc_vel_profile keywords), ticks[, start_vel (set_start)])} on Monteblanco, every ego at ``start_pos`` (the c2
    recording's start). See tests/test_sim_loop_host.py for what each class must reach."""
    lap = float(tab.s_rl[-1])
    movers = [(250.0, 0.35, 5.0), (lap - 1.0, 0.5, 5.0)]

    def parked(n):
        return [(600.0 + 40.0 * k, (0.0, 0.02, 0.05)[k % 3], 5.0) for k in range(n)]

    def entry(**kw):
        return dict(dict(opponents=[], static=[], pref=DEFAULT_PREF, pos_est=start_pos, vel_est=0.0, zone_gids=[]), **kw)
    return {
        "empty": dict(entry=entry(), vel=C2_VEL, ticks=200),
        "one": dict(entry=entry(opponents=[(250.0, 0.35, 5.0)]), vel=C2_VEL, ticks=200),
        "crowded": dict(entry=entry(opponents=movers + parked(38), static=crowded_statics(track, 56, 11)), vel=C2_VEL, ticks=200),
        "crowded70": dict(entry=entry(opponents=movers + parked(68), static=crowded_statics(track, 26, 12)), vel=C2_VEL, ticks=200),
        "statics": dict(entry=entry(static=crowded_statics(track, 26, 13)), vel=C2_VEL, ticks=200),
        "emerg_first": dict(entry=entry(opponents=[(140.0, 0.4, 5.0)], pref=("emergency", "straight", "follow")),
                            vel=dict(C2_VEL, incl_emerg_traj=True), ticks=200),
        # (a flying start at 15 m/s: the car brakes to standstill ON the emergency trajectory; from rest it would never leave it)
        "emerg_second": dict(entry=entry(opponents=[(140.0, 0.4, 5.0)], pref=("left", "emergency", "follow", "straight"), vel_est=15.0),
                             vel=dict(C2_VEL, incl_emerg_traj=True), ticks=300, start_vel=15.0),
        "failing": dict(entry=entry(opponents=[(250.0, 0.35, 5.0)], pref=("right",)), vel=C2_VEL, ticks=200),
    }


def lap_end_class(tab):
    """A class for any closed track: the ego started 60 m before the end of the lap, three opponents (one 20 m before the line)."""
    lap = float(tab.s_rl[-1])
    pos, heading = race_line_pose(tab, lap - 60.0)
    return dict(entry=dict(opponents=[(lap - 20.0, 0.3, 5.0), (40.0, 0.2, 5.0), (lap / 2.0, 0.5, 5.0)], static=[],
                           pref=("left", "right", "straight", "follow"), pos_est=pos, vel_est=0.0, zone_gids=[]),
                vel=C2_VEL, ticks=400, heading=heading)


def big_race(tab, n_cars, s0=50.0, gap=33.0, own=()):
    """One race of ``n_cars`` cars ``gap`` m apart from ``s0`` on, preference lists rotating over three orders; ``own``: opponents every
    car carries besides. Returns (entries, [(pos, heading)])."""
    orders = (("straight", "follow", "right", "left"), ("left", "right", "straight", "follow"), ("right", "left", "straight", "follow"))
    entries, poses = [], []
    for k in range(n_cars):
        pos, heading = race_line_pose(tab, s0 + gap * k)
        poses.append((pos, heading))
        entries.append(dict(opponents=list(own), static=[], pref=orders[k % 3], pos_est=pos, vel_est=0.0, zone_gids=[]))
    return entries, poses


BIG_RACE_TICKS = 120
CAP_RACE_CARS = 20


def cap_race_own(tab, n=96 - (CAP_RACE_CARS - 1), s0=760.0, gap=20.0):
    """Own opponents of every car of the race at the cap: parked or crawling on the race line ahead of the cars, so that all of them and
    all mates are on the track: own + mates = 96 exactly."""
    return [(s0 + gap * k, (0.0, 0.02)[k % 2], 5.0) for k in range(n)]


OTHER_TRACKS = ("berlin", "lvms")      # berlin: runtime LDS plan (its lattice is rebuilt by the offline build); lvms: the long oval


THREE_ROWS = ((0.0, 7.0), (40.0, 5.0), (100.0, 2.0))
VEL_VARIANTS = (dict(C2_VEL, vel_max=60.0, gg_scale=0.8), dict(C2_VEL, safety_d=15.0, local_gg=(4.0, 6.0), ax_max_machines=THREE_ROWS),
                dict(C2_VEL, vel_max=35.0, local_gg=(3.5, 3.5), incl_emerg_traj=True), dict(C2_VEL, ax_max_machines=THREE_ROWS, gg_scale=0.9))


def variant_pairs(n):
    """[(class name, variant, calc_vel_profile keywords)] for ``n`` planners: classes 'one', 'crowded', 'statics', 'emerg_second' crossed with
    velocity arguments (vel_max, gg_scale, safety_d, local_gg, machine table) that differ within one fleet."""
    out = []
    for i in range(n):
        name, v = ("one", "crowded", "statics", "emerg_second", "one")[i % 5], i % 4
        out.append((name, v, dict(VEL_VARIANTS[v], incl_emerg_traj=True) if name == "emerg_second" else dict(VEL_VARIANTS[v])))
    return out
