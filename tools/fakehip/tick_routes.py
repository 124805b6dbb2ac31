"""TEST TOOL: "every tick has a route". The library's host code built against the stand-in runtime without sanitizers
(FAKEHIP_SAN=none tools/fakehip/build.sh; it reports 256 compute units and 160 KiB of LDS, as an MI355X does), run with the product's
route thresholds (no LTPL_PIPELINE_MIN_SCEN / LTPL_FOLLOW_EMIT_MIN_SCEN in the environment). ltpl_tick_batch is called on lattices whose
fused tick fits, does not fit although the plan does (C5 at 120 .. 190 m: the band served by the pipeline at every batch size), and
whose plan does not fit (long-horizon mode), at batch sizes around every switch: no call may be refused. Kernels do nothing here, so
results are not looked at. Then LTPL_FORCE_FUSED=1 (forces the fused kernel at every size): a lattice whose fused tick does not fit
must come back as LTPL_ERR_CAPACITY with a message, Monteblanco must still run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from graphbasedlocaltrajectoryplanner_amd import _capi                      # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.lattice import Lattice            # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.scenario_gen import random_scenarios   # noqa: E402
from graphbasedlocaltrajectoryplanner_amd.synthetic_lattice import c5_lattice    # noqa: E402

FAKE = os.path.join(ROOT, "tools", "fakehip", "build_plain", "libltpl_hip_fake.so")
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 512, 513)

for name in ("LTPL_PIPELINE_MIN_SCEN", "LTPL_FOLLOW_EMIT_MIN_SCEN", "LTPL_FORCE_FUSED", "LTPL_FORCE_LONG_HORIZON"):
    assert name not in os.environ, "%s is set: this check is about the product defaults" % name


def inputs(lat, n):
    scen, vels = random_scenarios(lat, n, seed=n, n_veh=4)
    rng = np.random.default_rng(n)
    vplan = rng.uniform(0.0, 40.0, n)
    pos = np.array([lat.node_pos[lat.layer_off[s['start_node'][0]] + s['start_node'][1]] for s in scen])
    vel = _capi.TickVelBatch(_capi.VelParamSet(len_veh=lat.veh_length), n, vplan, vplan, pos, np.concatenate(vels))
    return _capi.PathsBatch(scen, w_last_edges=[0.0, 0.5, 0.8]), vel


def refusals(hip, lat, sizes):
    out = {}
    for n in sizes:
        try:
            hip.tick_batch(*inputs(lat, n))
        except _capi.BackendError as e:
            out[n] = str(e)
    return out


lattices = [("c5 %d m" % h, c5_lattice(horizon=float(h))) for h in (115, 120, 150, 190, 195)]
lattices.append(("monteblanco", Lattice.load(os.path.join(ROOT, "tests", "golden", "monteblanco_lattice.npz"))))
failed = []
for name, lat in lattices:
    hip = _capi.HipBackend(lat, lib_path=FAKE)
    bad = refusals(hip, lat, SIZES)
    hip.close()
    print("%-12s max_path_nodes %4d max_path_pts %4d: %s" % (name, hip.caps.max_path_nodes, hip.caps.max_path_pts,
                                                              "every size runs" if not bad else "REFUSED %s" % sorted(bad)))
    for n, msg in sorted(bad.items()):
        print("    n = %d: %s" % (n, msg[:140]))
    failed += [(name, n) for n in bad]
assert not failed, "ticks refused on the default routes: %s" % failed

os.environ["LTPL_FORCE_FUSED"] = "1"                             # (read by ltpl_create)
band = dict(lattices)["c5 150 m"]
hip = _capi.HipBackend(band, lib_path=FAKE)
bad = refusals(hip, band, (1, 64, 513))
hip.close()
assert sorted(bad) == [1, 64, 513], bad
for n, msg in sorted(bad.items()):
    assert "capacity exceeded" in msg and "fused tick exceeds the LDS budget" in msg, (n, msg)
print("forced fused tick on c5 150 m: refused at n = %s (%s)" % (sorted(bad), bad[1][:100]))
mb = dict(lattices)["monteblanco"]
hip = _capi.HipBackend(mb, lib_path=FAKE)
bad = refusals(hip, mb, (1, 64, 513))
hip.close()
assert not bad, bad
print("forced fused tick on monteblanco: every size runs")
print("tick routes OK")
