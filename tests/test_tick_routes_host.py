"""CPU: which route serves a tick (fused kernel or batch pipeline) with the product's thresholds -- no call may be refused.

The library's host code decides the route; it is built against the stand-in runtime (tools/fakehip, no sanitizers: it reports the
256 compute units and 160 KiB of LDS of an MI355X) and driven by tools/fakehip/tick_routes.py in a child process whose environment
does NOT carry the suite's LTPL_PIPELINE_MIN_SCEN / LTPL_FOLLOW_EMIT_MIN_SCEN pins (tests/conftest.py). C5 lattices with a 120 .. 190 m
horizon hold a four-wave plan that fits in LDS but a fused tick (plan + velocity scratch) that does not: the pipeline must serve them
at every batch size, single ticks included. Results are looked at by tests/test_gpu_default_routes.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_tick_size_has_a_route_with_the_default_thresholds():
    env = dict(os.environ, FAKEHIP_SAN="none", LTPL_NO_SELFTEST="1")
    for name in ("LTPL_PIPELINE_MIN_SCEN", "LTPL_FOLLOW_EMIT_MIN_SCEN", "LTPL_FORCE_FUSED", "LTPL_FORCE_LONG_HORIZON"):
        env.pop(name, None)
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=900)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "tick_routes.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and "tick routes OK" in p.stdout, p.stdout[-3000:]
    assert "c5 150 m" in p.stdout and "forced fused tick on c5 150 m: refused" in p.stdout, p.stdout[-3000:]
