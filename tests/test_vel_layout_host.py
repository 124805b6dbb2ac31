"""
CPU: the buffer layouts of the velocity stage (csrc/vel_layout.hpp), compiled with the host compiler alone (tests/vel_layout_shim.cpp) --

  1. the per-wave LDS scratch (carve_vel_scratch / vel_scratch_bytes): every array cap + 2 doubles, chunk and axm 128 doubles, sections
     disjoint and 8-byte aligned, arrays absent in a mode null, the run-start flags (cap + 16 bytes) inside the size, the size a multiple of
     16 and EQUAL TO THE FORMULA THE HOST USED BEFORE THE CARVE BECAME THE ONE DEFINITION (occupancy depends on this number);
  2. the fused tick's LDS: team block + 3 scratches + the fourth wave's flag row, that row inside the total and behind wave 2's scratch;
  3. the tiled planes in HBM (vel_planes_layout): order, disjointness, alignment, the total equal to the expression tick_prepare used
     before, zero when the tick is not the pipeline;
  4. with_vel_variant: variants 0 - 5 reach (EM, AXM1) = (0,f) (0,t) (1,f) (1,t) (2,f) (2,t), any other value the last one.
"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from graphbasedlocaltrajectoryplanner_amd.lattice import Lattice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ACTIONS = 3
SCRATCH = ("w", "kabs", "el", "s", "wb", "wc", "gax", "gay", "igay", "px", "py", "chunk", "axm")
PLANES = ("KE", "P0", "P1", "P2", "P3", "XY", "flags", "job_slot", "job_cnt", "fseg")


def align(x, a):
    return (x + a - 1) // a * a


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vel_layout") / "vel_layout_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "vel_layout_shim.cpp")], check=True)
    lib = ctypes.CDLL(so)
    P = ctypes.c_void_p
    lib.vel_scratch_layout_host.argtypes = [ctypes.c_int] * 4 + [P]
    lib.fused_tick_layout_host.argtypes = [ctypes.c_int, ctypes.c_int, P]
    lib.vel_planes_layout_host.argtypes = [ctypes.c_int] * 3 + [P]
    lib.vel_variant_reached_host.argtypes = [ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def caps():
    """1, 2, 14, 16, 17, 254, 256 and the lattice's max_path_pts (the longest path of any start layer, rounded up to 16 as ltpl_create does)"""
    lat = Lattice.load(os.path.join(ROOT, "tests", "golden", "monteblanco_lattice.npz"))
    pts = align(int(lat.max_horizon()[2]), 16)
    assert pts > 16
    return [1, 2, 14, 16, 17, 254, 256, pts]


def scratch(shim, cap, gg, xy, lite):
    out = np.zeros(16, np.int64)
    shim.vel_scratch_layout_host(cap, int(gg), int(xy), int(lite), out.ctypes.data)
    off = dict(zip(SCRATCH, (int(v) for v in out[:13])))
    return off, int(out[13]), int(out[14]), int(out[15])


def test_velocity_scratch(shim, caps):
    for cap, gg, xy, lite in itertools.product(caps, (False, True), (False, True), (False, True)):
        off, start, nbytes, vs_cap = scratch(shim, cap, gg, xy, lite)
        what = "cap %d gg %d xy %d lite %d" % (cap, gg, xy, lite)
        assert vs_cap == cap, what
        # arrays absent in a mode are null, the others are there
        absent = set()
        if lite:
            absent |= {"s", "wb", "wc", "chunk"}
        if not gg:
            absent |= {"gax", "gay", "igay"}
        if not xy:
            absent |= {"px", "py"}
        assert {k for k, o in off.items() if o < 0} == absent, what
        # sections: every array cap + 2 doubles, chunk and axm 128 doubles, the flags cap + 16 bytes; disjoint, 8-byte aligned, inside the size
        size = {k: 8 * (128 if k in ("chunk", "axm") else cap + 2) for k in SCRATCH}
        sec = sorted((o, o + size[k], k) for k, o in off.items() if o >= 0) + [(start, start + cap + 16, "start")]
        assert sec[0][0] == 0, what
        for (a0, a1, ka), (b0, b1, kb) in zip(sec, sec[1:]):
            assert a1 == b0, (what, ka, kb)             # (disjoint and no gap: each array is exactly its size)
        assert all(a0 % 8 == 0 for a0, _, _ in sec), what
        assert start + cap + 16 <= nbytes and nbytes % 16 == 0, what
        # the size formula of the host side before the carve sized the launch
        arrays = (3 if lite else 6) + (3 if gg else 0) + (2 if xy else 0)
        b = 8 * (arrays * (cap + 2) + (128 if lite else 256)) + cap + 16
        assert nbytes == (b + 15) // 16 * 16, what


def test_fused_tick_lds(shim, caps):
    for cap, lp4 in itertools.product(caps, (0, 16, 4096, 70000)):
        out = np.zeros(4, np.int64)
        shim.fused_tick_layout_host(lp4, cap, out.ctypes.data)
        total, flags_off, stride, n_act = (int(v) for v in out)
        assert n_act == MAX_ACTIONS
        assert stride == scratch(shim, cap, False, True, False)[2]
        assert total == lp4 + 3 * stride + align(cap + 16, 16), (cap, lp4)
        # the fourth wave's flag row: behind wave 2's scratch, inside the total
        assert flags_off >= lp4 + MAX_ACTIONS * stride and flags_off + cap + 16 <= total, (cap, lp4)


def planes(shim, n_scen, cap_pts, pipeline=True):
    out = np.zeros(14, np.int64)
    shim.vel_planes_layout_host(n_scen, cap_pts, int(pipeline), out.ctypes.data)
    v = [int(x) for x in out]
    return dict(zip(PLANES, v[:10])), v[10], v[11], v[12], v[13]


def test_velocity_planes(shim):
    for n_scen, cap_pts in itertools.product((1, 63, 64, 65, 128, 129), (1, 7, 8, 9, 64)):
        off, n_slots_pad, n_scen_pad, plane_rows, nbytes = planes(shim, n_scen, cap_pts)
        what = "n_scen %d cap_pts %d" % (n_scen, cap_pts)
        assert n_slots_pad == align(MAX_ACTIONS * n_scen, 64) and n_scen_pad == align(n_scen, 64) and plane_rows == align(cap_pts, 8), what
        tiles = n_slots_pad + n_scen_pad
        # the operand plane: two doubles per row and tile
        size = {"KE": 16 * plane_rows * tiles, "P0": 8 * cap_pts * tiles, "P1": 8 * cap_pts * n_scen_pad, "P2": 8 * cap_pts * n_scen_pad,
                "P3": 8 * cap_pts * n_scen_pad, "XY": 16 * plane_rows * n_scen_pad, "flags": 4 * tiles, "job_slot": 8 * tiles, "job_cnt": 4 * 16,
                "fseg": 8 * n_scen_pad}
        # sections in the order KE, P0 .. P3, XY, flags, job_slot, job_cnt, fseg; disjoint; the last one ends inside the block
        assert off["KE"] == 0, what
        for a, b in zip(PLANES, PLANES[1:]):
            assert off[a] + size[a] == off[b], (what, a, b)
        assert off["fseg"] + size["fseg"] == nbytes, what
        assert off["KE"] % 16 == 0 and off["XY"] % 16 == 0, what
        assert all(off[k] % 8 == 0 for k in ("P0", "P1", "P2", "P3", "job_slot")), what
        assert all(off[k] % 4 == 0 for k in ("flags", "job_cnt", "fseg")), what
        # the expression tick_prepare sized the block with before the layout was the one definition
        assert nbytes == 8 * (2 * plane_rows * tiles + cap_pts * (tiles + 3 * n_scen_pad) + 2 * plane_rows * n_scen_pad) \
            + 4 * (3 * tiles + 16 + 2 * n_scen_pad), what
        # not the pipeline: no planes
        off0, sp0, cp0, pr0, nbytes0 = planes(shim, n_scen, cap_pts, pipeline=False)
        assert nbytes0 == 0 and (sp0, cp0, pr0) == (n_slots_pad, n_scen_pad, plane_rows), what


def test_with_vel_variant(shim):
    # 2 * EM + AXM1: (0,f) (0,t) (1,f) (1,t) (2,f) (2,t)
    assert [shim.vel_variant_reached_host(v) for v in range(6)] == [0, 1, 2, 3, 4, 5]
    for v in (-1, 6, 7, 8, 100, -(2 ** 31), 2 ** 31 - 1):
        assert shim.vel_variant_reached_host(v) == 5, v
