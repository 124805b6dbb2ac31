"""
TEST INFRASTRUCTURE (no test functions): scripted events of the fleet simulation (ltpl_fleet_sim_events, csrc/fleet_events.hpp) on the
host loop of tests/sim_loop.py. ``sim.EventScript`` decides which events fire in front of a tick; ``apply_writes`` carries their writes
into a ``HostSimLoop`` from outside (its ``cfg`` and ``velkw`` are plain attributes), ``loop_state`` hands the loop's state to the
script. Further down: the seeded event scenarios shared by tests/test_sim_events_host.py (which shows on the CPU that they are not
vacuous) and tests/test_gpu_sim_events.py (which runs the device through them).
"""
import numpy as np

import sim_loop as sl
from graphbasedlocaltrajectoryplanner_amd.sim import Event

VEL_KEYS = {"vel_max": "vel_max", "gg_scale": "gg_scale", "safety_d": "safety_d", "incl_emerg": "incl_emerg_traj"}
OPP_COL = {"opp_vel_scale": 1, "opp_length": 2}
STATIC_COL = {"static_x": 0, "static_y": 1, "static_theta": 2, "static_v": 3, "static_length": 4}


def apply_writes(loop, fired, host_of=None):
    """``fired``: what ``EventScript.before_tick`` returned; ``host_of``: {fleet planner: planner of ``loop``} (default: the same index;
    planners the loop does not hold are skipped)."""
    for _, p, (kind, idx, val) in fired:
        h = p if host_of is None else host_of.get(p)
        if h is None:
            continue
        cfg, kw = loop.cfg[h], loop.velkw[h]
        if kind in OPP_COL:
            o = list(cfg["opp"][idx])
            o[OPP_COL[kind]] = float(val)
            cfg["opp"][idx] = tuple(o)
        elif kind in STATIC_COL:
            s = list(cfg["static"][idx])
            s[STATIC_COL[kind]] = float(val)
            cfg["static"][idx] = tuple(s)
        elif kind == "pref":
            cfg["pref"][idx] = val
        elif kind in ("gg_ax", "gg_ay"):
            g = list(kw.get("local_gg", (5.0, 5.0)))
            g[0 if kind == "gg_ax" else 1] = float(val)
            kw["local_gg"] = tuple(g)
        elif kind in VEL_KEYS:
            kw[VEL_KEYS[kind]] = val
        else:
            raise ValueError("the host loop has no target for %r" % kind)


def loop_state(loop):
    """The state a free-running ``HostSimLoop`` hands to ``EventScript.before_tick``."""
    return dict(pos=loop.pos, vel=loop.vel, opp_s=loop.opp_s, failed=loop.failed)


def fleet_state(fleet, opp_off, failed=None):
    """The same from the device (``Fleet.sim_state``); ``failed``: error flags of the tick before (trace field [8] != 0)."""
    st = fleet.sim_state()
    return dict(pos=st["pos_est"], vel=st["vel_est"], opp_s=st["opp_s"], opp_off=opp_off, failed=failed)


# ---- seeded event scenarios ---------------------------------------------------------------------------------------------------------
EVENT_TICKS = 54          # ticks of the differential runs
SPLIT = 20                # timed events at SPLIT - 1 and SPLIT: the last tick of one call and the first of the next where a run is split there
BRAKE_SCALE0, BRAKE_TICKS = 0.3, 24   # the braking unit's opponent: vel_scale before and after the brake (0.2 in between), ticks it lasts
BRAKE_START_VEL = 15.0    # flying start of the braking unit (set_start and vel_est)


def entry(start_pos, opponents, static=(), pref=sl.DEFAULT_PREF):
    return dict(opponents=list(opponents), static=list(static), pref=tuple(pref), pos_est=start_pos, vel_est=0.0, zone_gids=[])


def braking_unit(start_pos):
    """One planner with a flying start (15 m/s) closing in on an opponent 100 m ahead: the opponent brakes (vel_scale 0.3 -> 0.2) when
    the ego is within 97 m and accelerates again 24 ticks later; a speed trigger with a chain of two, one that never fires, timed events
    at tick 0 and on both sides of SPLIT."""
    e = dict(entry(start_pos, [(100.0, BRAKE_SCALE0, 5.0)]), vel_est=BRAKE_START_VEL)
    ev = [Event(0, when=("opp_within", 0, 97.0), set=("opp_vel_scale", 0, 0.2)),
          Event(0, when=("after", 0, BRAKE_TICKS), set=("opp_vel_scale", 0, BRAKE_SCALE0)),
          Event(0, when=("vel_above", 17.0), set=("safety_d", 25.0)),
          Event(0, when=("after", 2, 4), set=("gg_scale", 0.9)),
          Event(0, when=("after", 3, 3), set=("vel_max", 60.0)),
          Event(0, when=("vel_below", -1.0), set=("vel_max", 50.0)),               # never fires
          Event(0, when=("tick", 0), set=("opp_length", 0, 4.0)),
          Event(0, when=("tick", SPLIT - 1), set=("gg_ax", 4.5)),
          Event(0, when=("tick", SPLIT), set=("gg_ay", 4.0))]
    return e, ev


def statics_unit(start_pos, track, n_static, n_opp, seed):
    """A planner with ``n_opp`` parked opponents and ``n_static`` statics: a static set up off the track is moved onto it at a tick, one
    starts to move, the preference list changes at a tick; a trigger on the LAST opponent (a wrong local -> global index reads a
    neighbour's)."""
    opp = [(150.0 + 35.0 * k, (0.0, 0.02, 0.05)[k % 3], 5.0) for k in range(n_opp)]
    st = sl.crowded_statics(track, n_static, seed, first_row=40, every=6)
    e = entry(start_pos, opp, st)
    ref, nv = np.asarray(track['refline'], float), np.asarray(track['normvec'], float)
    ev = []
    if n_static:
        off_k = next(k for k in range(n_static) if k % 3 == 0)                     # (crowded_statics: 40 m off the track)
        i = (40 + 6 * off_k) % ref.shape[0]
        ev += [Event(0, when=("tick", 5), set=("static_x", off_k, float(ref[i, 0] + 0.5 * nv[i, 0]))),
               Event(0, when=("tick", 5), set=("static_y", off_k, float(ref[i, 1] + 0.5 * nv[i, 1]))),
               Event(0, when=("tick", 7), set=("static_v", n_static - 1, 3.0)),
               Event(0, when=("tick", 7), set=("static_theta", n_static - 1, 0.3)),
               Event(0, when=("tick", 9), set=("static_length", n_static - 1, 6.0))]
    if n_opp:
        ev += [Event(0, when=("opp_within", n_opp - 1, 400.0), set=("opp_vel_scale", n_opp - 1, 0.3)),
               Event(0, when=("after", len(ev), 2), set=("opp_length", n_opp - 1, 3.0))]
    ev.append(Event(0, when=("tick", 12), set=("pref", 1, "straight")))
    return e, ev


def many_unit(start_pos):
    """70 opponents, a trigger on opponent 66, and 16 triggers in all (the cap): speed thresholds that fire one after the other while the
    car accelerates, the same target written by several (the later of the list wins when two fire in one tick)."""
    opp = [(250.0, 0.35, 5.0)] + [(600.0 + 12.0 * k, (0.0, 0.02, 0.05)[k % 3], 5.0) for k in range(69)]
    e = entry(start_pos, opp)
    ev = [Event(0, when=("opp_within", 66, 1.0e4), set=("opp_vel_scale", 66, 0.1))]
    ev += [Event(0, when=("vel_above", 0.5 * k), set=("safety_d", 30.0 - k)) for k in range(1, 14)]
    ev += [Event(0, when=("vel_above", 1.0), set=("safety_d", 12.0)),                # fires with k = 2's: the later one wins
           Event(0, when=("after", 0, 1), set=("opp_length", 66, 4.5))]
    assert len(ev) == 16
    return e, ev


def scenario(start_pos, track, n):
    """(entries, events, classes, start speeds) of a fleet of ``n`` planners: units of different opponent / static counts dealt round robin, so that
    neighbours' offsets differ; planner 0 always the braking unit. ``classes[p]``: the unit kind of planner p. The last planner carries
    no trigger. Every planner has one timed event in tick 3 (n = 65: two blocks of the timed kernel); planners of one kind are identical."""
    kinds = ["brake", "statics", "many", "statics2", "plain"]
    entries, events, classes = [], [], []
    for p in range(n):
        kind = kinds[p % len(kinds)] if p < n - 1 or n == 1 else "plain"
        if kind == "brake":
            e, ev = braking_unit(start_pos)
        elif kind == "statics":
            e, ev = statics_unit(start_pos, track, 7, 3, 21)
        elif kind == "statics2":
            e, ev = statics_unit(start_pos, track, 4, 0, 22)
        elif kind == "many":
            e, ev = many_unit(start_pos)
        else:
            e, ev = entry(start_pos, [(250.0, 0.35, 5.0), (400.0, 0.3, 5.0)]), []
        entries.append(e)
        classes.append(kind)
        events += [Event(p, when=x.when, set=x.set) for x in ev]
        events.append(Event(p, when=("tick", 3), set=("vel_max", 90.0 - kinds.index(kind))))
    return entries, events, classes, [BRAKE_START_VEL if k == "brake" else 0.0 for k in classes]
