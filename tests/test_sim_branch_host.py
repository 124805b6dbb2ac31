"""
CPU: snapshot and branch of the fleet simulation's planner state (ltpl_fleet_sim_snapshot / _snapshot_info / _snapshot_drop /
ltpl_fleet_sim_branch, include/ltpl_hip.h; csrc/fleet_branch.hpp) on the host -- the argument checks, the bookkeeping of the slots and the
number of launches on the stand-in runtime (tools/fakehip/sim_branch_args.py, plain build). The copies themselves are tested on the
device: tests/test_gpu_sim_branch.py.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_snapshot_and_branch_entry_points_check_their_arguments_without_a_device():
    env = dict(os.environ, FAKEHIP_SAN="none", LTPL_NO_SELFTEST="1")
    subprocess.run([os.path.join(ROOT, "tools", "fakehip", "build.sh")], check=True, env=env, stdout=subprocess.DEVNULL, timeout=1500)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fakehip", "sim_branch_args.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and "sim branch args OK" in p.stdout, p.stdout[-3000:]
    assert "launches per tick" in p.stdout and p.stdout.count("previous snapshot kept") == 2, p.stdout[-3000:]
    assert p.stdout.count("each part kernel once, 1 allocation in front of them") == 2 and "nothing launched, the slot as it was" in p.stdout, p.stdout[-3000:]


def test_python_binding_declares_the_four_entry_points():
    from graphbasedlocaltrajectoryplanner_amd import fleet
    assert fleet.SIM_SNAPSHOTS == 8
    for name in ("sim_snapshot", "sim_snapshot_info", "sim_snapshot_drop", "sim_branch", "sim_restore"):
        assert callable(getattr(fleet.Fleet, name)), name
    with open(os.path.join(ROOT, "include", "ltpl_hip.h")) as fh:
        hdr = fh.read()
    assert "#define LTPL_FLEET_SIM_SNAPSHOTS 8" in hdr
    for name in ("ltpl_fleet_sim_snapshot(", "ltpl_fleet_sim_snapshot_info(", "ltpl_fleet_sim_snapshot_drop(", "ltpl_fleet_sim_branch("):
        assert name in hdr, name
