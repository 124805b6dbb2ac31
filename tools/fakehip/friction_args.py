"""TEST TOOL: argument checks of ltpl_fleet_friction / ltpl_fleet_friction_scale / ltpl_fleet_friction_rows (the fleet's friction maps in
device memory) without a device. The library's host code built against the stand-in runtime (FAKEHIP_SAN=none tools/fakehip/build.sh, or
the ASan + UBSan build with ``--san``: run it with the sanitizer run-time preloaded like tools/fakehip/run.sh); kernels do nothing, so
results are not looked at -- only the return codes, the messages and the kernels a tick launches:
  - every invalid argument is refused before any device allocation (an allocation failure armed for the next hipMalloc is still pending
    after the refused call): null pointers, nx < 2, non-finite or non-positive values, map_idx out of range, node offsets that do not match;
  - a fleet with a map launches the rows form of the velocity stage (one more launch per tick for a small fleet: the forward-backward jobs with rows),
    clearing the maps brings back the number of launches of a fleet that never had one (the brake / emergency launches keep their rows form);
  - an allocation failing at any point of ltpl_fleet_friction leaves the fleet with its previous maps: LTPL_ERR_HIP, and the lookup on the
    old map still works."""
import ctypes
import sys

import numpy as np

import sim_args_common as common
from sim_args_common import launches_per_tick, msg, no_allocation
from graphbasedlocaltrajectoryplanner_amd.fleet import FrictionIn
from graphbasedlocaltrajectoryplanner_amd.friction import FrictionGrid

N = 4
lib, fleet, table = common.start(N, "build" if "--san" in sys.argv else "build_plain")
lib.ltpl_fleet_friction.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.ltpl_fleet_friction_scale.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.ltpl_fleet_friction_rows.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_void_p]
h = fleet.handle
GRIDS = [FrictionGrid(0.0, 0.0, 10.0, 10.0, np.full((3, 4), 4.0), np.full((3, 4), 3.0)),
         FrictionGrid(-5.0, 2.0, 1.0, 2.0, np.full((2, 2), 5.0), np.full((2, 2), 6.0))]


def call(drop=(), **over):
    """ltpl_fleet_friction with the two maps above; ``over`` replaces arrays, ``drop`` names members left null."""
    f64, i32 = np.float64, np.int32
    a = dict(x0=np.array([g.x0 for g in GRIDS], f64), y0=np.array([g.y0 for g in GRIDS], f64), dx=np.array([g.dx for g in GRIDS], f64),
             dy=np.array([g.dy for g in GRIDS], f64), nx=np.array([g.nx for g in GRIDS], i32), ny=np.array([g.ny for g in GRIDS], i32),
             node_off=np.array([0, 12, 16], i32), nodes=np.concatenate([g.nodes() for g in GRIDS]), map_idx=np.array([0, 1, -1, 0], i32),
             scale=np.array([1.0, 0.7, 1.0, 0.5], f64))
    n_maps = over.pop("n_maps", 2)
    for k, v in over.items():
        a[k] = np.ascontiguousarray(np.asarray(v, a[k].dtype))
    fi = FrictionIn()
    fi.n_maps = n_maps
    for k, v in a.items():
        if k not in drop:
            setattr(fi, k, v.ctypes.data)
    return lib.ltpl_fleet_friction(h, ctypes.byref(fi))


def refused(code, text, **kw):
    rc = no_allocation(lambda: call(**kw))
    assert rc == code and text in msg(), (rc, msg(), code, text, kw)
    print("refused (%d): %s" % (rc, msg()))


def nodes_with(i, v):
    n = np.concatenate([g.nodes() for g in GRIDS])
    n.reshape(-1)[i] = v
    return n


# ---- refused before any allocation ----------------------------------------------------------------------------------------------
assert lib.ltpl_fleet_friction(None, None) == 1 and lib.ltpl_fleet_friction(h, None) == 1
assert lib.ltpl_fleet_friction_scale(None, None) == 1 and lib.ltpl_fleet_friction_scale(h, None) == 1
assert lib.ltpl_fleet_friction_rows(None, 0, None, None, 0, 1.0, None) == 1
one = np.ones(N)
assert no_allocation(lambda: lib.ltpl_fleet_friction_scale(h, one.ctypes.data)) == 1 and "ltpl_fleet_friction first" in msg()
xy = np.zeros(3)
assert no_allocation(lambda: lib.ltpl_fleet_friction_rows(h, 0, xy.ctypes.data, xy.ctypes.data, 3, 1.0, np.zeros(6).ctypes.data)) == 1 and "map out of range" in msg()
for member in ("x0", "y0", "dx", "dy", "nx", "ny", "node_off", "nodes"):
    refused(1, "map arrays missing", drop=(member,))
for member in ("map_idx", "scale"):
    refused(1, "map_idx / scale missing", drop=(member,))
refused(1, "n_maps must not be negative", n_maps=-1)
refused(1, "at least 2 x 2 nodes", nx=[1, 2], node_off=[0, 3, 7])
refused(1, "at least 2 x 2 nodes", ny=[3, 1], node_off=[0, 12, 14])
refused(1, "at least 2 x 2 nodes", nx=[4, 0])
for bad in (np.nan, np.inf, -np.inf):
    refused(1, "x0 / y0 must be finite", x0=[0.0, bad])
    refused(1, "x0 / y0 must be finite", y0=[bad, 0.0])
for bad in (0.0, -1.0, np.nan, np.inf):
    refused(1, "dx / dy must be finite and positive", dx=[bad, 1.0])
    refused(1, "dx / dy must be finite and positive", dy=[10.0, bad])
refused(1, "node_off must start at 0", node_off=[1, 13, 17])
refused(1, "must be nx[m] * ny[m]", node_off=[0, 12, 15])
refused(1, "must be nx[m] * ny[m]", node_off=[0, 11, 16])
for bad in (0.0, -4.0, np.nan, np.inf):
    refused(1, "node values must be finite and positive", nodes=nodes_with(5, bad))
    refused(1, "node values must be finite and positive", nodes=nodes_with(31, bad))
    refused(1, "a scale must be finite and positive", scale=[1.0, 1.0, bad, 1.0])
refused(1, "map_idx out of range", map_idx=[0, 2, 0, 0])
refused(1, "map_idx out of range", map_idx=[0, 1, -2, 0])

# ---- launches of a tick with and without a map -------------------------------------------------------------------------------------
good = dict(opponents=[(250.0, 0.3, 5.0)], pref=("right", "straight"), pos_est=(0.0, 0.0), zone_gids=[3])


fleet.sim_setup(table, [good] * N)
fleet.sim_vel()
plain = launches_per_tick()
assert call() == 0, msg()
assert launches_per_tick() == plain + 1                     # + k_vel_profile SEL 3: forward-backward jobs with rows (a small fleet's follow jobs run wave per job either way)
assert call(map_idx=[-1] * N) == 0                          # maps set, no planner on one: the launches of before
assert launches_per_tick() == plain
assert call() == 0
fleet.friction_scale([1.0, 0.3, 1.0, 1.0])                  # after a run, between runs
for bad in (0.0, -1.0, np.nan, np.inf):
    s = np.array([1.0, bad, 1.0, 1.0])
    assert lib.ltpl_fleet_friction_scale(h, s.ctypes.data) == 1 and "finite and positive" in msg()
assert launches_per_tick() == plain + 1
pts = np.array([[3.0, 4.0], [-100.0, 50.0], [35.0, 25.0]])
assert fleet.friction_rows(0, pts).shape == (3, 2) and fleet.friction_rows(1, pts, 0.5).shape == (3, 2)
assert fleet.friction_rows(0, np.zeros((0, 2))).shape == (0, 2)
out = np.zeros(6)
x, y = np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1])
assert no_allocation(lambda: lib.ltpl_fleet_friction_rows(h, 2, x.ctypes.data, y.ctypes.data, 3, 1.0, out.ctypes.data)) == 1 and "map out of range" in msg()
assert no_allocation(lambda: lib.ltpl_fleet_friction_rows(h, -1, x.ctypes.data, y.ctypes.data, 3, 1.0, out.ctypes.data)) == 1
assert no_allocation(lambda: lib.ltpl_fleet_friction_rows(h, 0, None, y.ctypes.data, 3, 1.0, out.ctypes.data)) == 1 and "missing" in msg()
assert no_allocation(lambda: lib.ltpl_fleet_friction_rows(h, 0, x.ctypes.data, y.ctypes.data, 3, 1.0, None)) == 1
assert no_allocation(lambda: lib.ltpl_fleet_friction_rows(h, 0, x.ctypes.data, y.ctypes.data, -3, 1.0, out.ctypes.data)) == 1
assert no_allocation(lambda: lib.ltpl_fleet_friction_rows(h, 0, x.ctypes.data, y.ctypes.data, 3, np.nan, out.ctypes.data)) == 1
fleet.friction(None)                                        # n_maps = 0 clears
assert launches_per_tick() == plain
assert lib.ltpl_fleet_friction_rows(h, 0, x.ctypes.data, y.ctypes.data, 3, 1.0, out.ctypes.data) == 1 and "map out of range" in msg()
fleet.friction(GRIDS, map_idx=[0, 1, -1, 1], scale=[1.0, 0.8, 1.0, 0.6])     # (the Python form)
assert launches_per_tick() == plain + 1

# ---- an allocation failing at every point of ltpl_fleet_friction: the previous maps stay -------------------------------------------------
fresh = common.Fleet(common.hip, N)                         # (a fleet whose rows array does not exist yet: one allocation more)
h_old, h = h, fresh.handle
common.use_handle(h)
one_map = [GRIDS[0]]


def no_map_0(k, _):
    """The cleared state is still in place."""
    assert lib.ltpl_fleet_friction_rows(h, 0, x.ctypes.data, y.ctypes.data, 3, 1.0, out.ctypes.data) == 1


failures = common.alloc_sweep("ltpl_fleet_friction", lambda: (call(), msg()), 32, no_map_0)
assert failures == 5, failures                             # maps, nodes, map_idx, scale, the planners' rows
fresh.friction(one_map)
for k in range(1, 5):                                       # (the rows array exists by now)
    lib.fakehip_fail_malloc_after(k)
    rc = call()
    lib.fakehip_fail_malloc_after(0)
    assert rc == 3, (k, rc)
    assert fresh.friction_rows(0, pts).shape == (3, 2)                # the old map 0 serves lookups ...
    assert lib.ltpl_fleet_friction_rows(h, 1, x.ctypes.data, y.ctypes.data, 3, 1.0, out.ctypes.data) == 1      # ... and there is no map 1
print("allocation failure at each of the %d allocations of ltpl_fleet_friction: previous maps kept" % failures)
print("launches per tick: %d without a map, %d with" % (plain, plain + 1))
h = h_old
common.use_handle(h)
fresh.close()
common.finish("friction args OK")
