"""Copy rate of SNAPSHOT AND BRANCH of the fleet simulation (ltpl_fleet_sim_snapshot / ltpl_fleet_sim_branch, csrc/fleet_branch.hpp:
k_fleet_sim_branch) on the fleet of tools/sim_rate.py.   tools/sim_branch_rate.py [--planners 32768] [--ticks 5] [--reps 3] [--friction-map]
[--lib PATH] [--out FILE.json]. After a few ticks of sim_run (so that every planner holds trajectories) the best of ``--reps`` runs of
  snapshot   a snapshot of every planner (wall time of the call: allocation of the slot included; the copy alone is what restore times)
  restore    every planner back from the slot (device time of the copy)
  fan-out    8 sources into all other planners
  scattered  4 096 pairs spread over the fleet (a seeded permutation)
in milliseconds and bytes moved (read + written) per second; the bytes of a pair are the planner block plus, with --friction-map, its
window of friction rows -- the scalars, opponents and telemetry record of a pair are a few hundred bytes and left out. For orientation
only: a float4 copy kernel moves 6.29 TB/s on the same device (read + written). Prints the memory of the full snapshot (info.bytes) and the
kernel's register / scratch / LDS figures. LTPL_SIM_BRANCH_NT=1 with --lib pointing at the experiment build times the non-temporal store
form."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                                            # noqa: E402
import planner_replay as pr                                                   # noqa: E402
from graphbasedlocaltrajectoryplanner_amd import _capi                        # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.fleet import Fleet                  # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.lattice import Lattice              # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.sim import RaceLineTable            # noqa: E402

FLOAT4_COPY_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planners", type=int, default=32768)
    ap.add_argument("--ticks", type=int, default=5, help="ticks of sim_run in front of the copies")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--friction-map", action="store_true", help="every planner on the friction grid: row windows exist and are copied")
    ap.add_argument("--lib", default=None, help="path of the library to load (default: the in-tree build)")
    ap.add_argument("--out", default=None, help="write the figures as JSON")
    a = ap.parse_args()
    lat = Lattice.load(os.path.join(ROOT, "tests", "golden", "monteblanco_lattice.npz"))
    race = RaceLineTable.from_track(np.load(os.path.join(ROOT, "tests", "golden", "monteblanco_track.npz")))
    hip = _capi.HipBackend(lat, lib_path=a.lib) if a.lib else _capi.HipBackend(lat)
    ticks = pr.load_ticks("c2")
    st, va = ticks[0]['start'], ticks[0]['vel_args']
    zones = pr.zone_gids_of_tick(lat, ticks[0])
    n = a.planners
    entries = [dict(opponents=[(250.0 + 280.0 * k + 10.0 * (p % 16), 0.30 + 0.05 * (k % 4), 5.0) for k in range(8)],
                    pref=("right", "left", "straight", "follow"), pos_est=st['pos'], vel_est=0.0, zone_gids=zones) for p in range(n)]
    fleet = Fleet(hip, n)
    fleet.set_start_range(0, n, st['pos'], st['heading'], st['vel'], st['max_heading_offset'])
    fleet.sim_setup(race, entries)
    if a.friction_map:
        from graphbasedlocaltrajectoryplanner_amd.friction import FrictionGrid
        fleet.friction(FrictionGrid.load(os.path.join(ROOT, "tests", "golden", "friction_grid.npz")), scale=1.0 - 0.3 * (np.arange(n) % 16) / 15.0)
    fleet.sim_vel(vel_max=va['vel_max'], gg_scale=va['gg_scale'], local_gg=tuple(va['local_gg']), safety_d=va['safety_d'],
                  ax_max_machines=va['ax_max_machines'])
    fleet.sim_run(a.ticks, trace=False)
    before = fleet.digest()

    walls = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fleet.sim_snapshot(0)
        walls.append((time.perf_counter() - t0) * 1e3)
    info = fleet.sim_snapshot_info(0)
    per_pair = info["bytes"] // n // 256 * 256          # planner block (+ row window): the small parts are below 256 bytes per planner ...
    small = info["bytes"] - per_pair * n
    assert 0 <= small < 1024 * n, (info["bytes"], per_pair)
    src8 = [int(q) for q in np.linspace(0, n - 1, 8).round()] if n >= 16 else [0]
    fan_dst = np.setdiff1d(np.arange(n), src8).astype(np.int32)
    fan_src = np.array(src8, np.int32)[np.arange(fan_dst.size) % len(src8)]
    rng = np.random.default_rng(7)
    perm = rng.permutation(n)
    m = min(4096, n // 2)
    sc_src, sc_dst = perm[:m].astype(np.int32), perm[m:2 * m].astype(np.int32)
    cases = [("restore", lambda: fleet.sim_restore(0), n), ("fan-out of %d" % len(src8), lambda: fleet.sim_branch(fan_src, fan_dst), int(fan_dst.size)),
             ("%d scattered pairs" % m, lambda: fleet.sim_branch(sc_src, sc_dst), m)]
    out = {"planners": n, "friction_map": bool(a.friction_map), "snapshot_bytes": info["bytes"], "bytes_per_pair": per_pair,
           "float4_copy_TBs_for_orientation": FLOAT4_COPY_TBS, "nontemporal": os.environ.get("LTPL_SIM_BRANCH_NT", "0") not in ("", "0"), "cases": {}}
    ms = min(walls)
    print("full snapshot: %d planners, %d bytes (%.1f KB per planner): best wall time of the call %.3f ms (all: %s)" % (
        n, info["bytes"], info["bytes"] / n / 1024.0, ms, ", ".join("%.3f" % w for w in walls)))
    out["cases"]["snapshot (wall, allocation included)"] = {"ms": ms, "all_ms": walls, "pairs": n, "TBs": 2.0 * per_pair * n / ms / 1e9}
    for name, fn, pairs in cases:
        t = [fn() for _ in range(a.reps)]
        ms = min(t)
        tbs = 2.0 * per_pair * pairs / ms / 1e9
        out["cases"][name] = {"ms": ms, "all_ms": t, "pairs": pairs, "TBs": tbs}
        print("%-22s %6d pairs: best %.3f ms (all: %s) = %.2f TB/s read + written   [float4 copy, for orientation: %.2f TB/s]" % (
            name, pairs, ms, ", ".join("%.3f" % x for x in t), tbs, FLOAT4_COPY_TBS))
    # the restore brought every planner back before the branches scattered states about: the fleet still runs
    fleet.sim_restore(0)
    assert np.array_equal(fleet.digest(), before, equal_nan=True)
    fleet.sim_run(2, trace=False)
    import __graft_entry__ as ge
    res = {k: v for k, v in ge.kernel_resources(a.lib or ge.HIP_LIB).items() if "k_fleet_sim_branch" in k}
    for k, v in res.items():
        print("%s: %d VGPRs, %d SGPRs, %d B scratch, %d B LDS, %d spilled" % (k, v.get("vgpr_count", -1), v.get("sgpr_count", -1),
              v.get("private_segment_fixed_size", -1), v.get("group_segment_fixed_size", -1), v.get("vgpr_spill_count", -1)))
    out["kernel_resources"] = res
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
    fleet.close()


if __name__ == "__main__":
    main()
