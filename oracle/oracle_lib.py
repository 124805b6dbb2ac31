"""
ORACLE / TEST INFRASTRUCTURE ONLY -- never imported by the product path.

ctypes binding of oracle/libltpl_oracle.so (the plain-C restatement in oracle/ltpl_oracle.c). It exposes the same
method surface as ``graphbasedlocaltrajectoryplanner_amd._capi.HipBackend`` so that tests can (a) compare the HIP
path against it on identical packed inputs and (b) drive the host-side mirror with it on machines without a GPU in
order to check the HOST logic against the real reference. bench.py uses it for the ``cpu_baseline`` leg only.
"""
import ctypes as C
import os
import subprocess

from graphbasedlocaltrajectoryplanner_amd import _capi
from graphbasedlocaltrajectoryplanner_amd.lattice import Lattice

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libltpl_oracle.so")


def build(force=False):
    src = os.path.join(HERE, "ltpl_oracle.c")
    hdr = os.path.join(os.path.dirname(HERE), "include", "ltpl_hip.h")
    if (not force and os.path.isfile(LIB)
            and os.path.getmtime(LIB) >= max(os.path.getmtime(src), os.path.getmtime(hdr))):
        return LIB
    # (two processes -- the ranks of a gloo test, pytest-xdist workers -- may find the library stale at the same time: one builds, the
    #  other waits on the lock and finds it fresh)
    import fcntl
    with open(os.path.join(HERE, ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if force or not (os.path.isfile(LIB) and os.path.getmtime(LIB) >= max(os.path.getmtime(src), os.path.getmtime(hdr))):
            subprocess.check_call(["make", "-s", "-C", HERE, "-B", "libltpl_oracle.so"])
    return LIB


def _project(lib_path, entry, x, y, s, closed, qx, qy):
    import numpy as np
    x, y, s, qx, qy = (np.ascontiguousarray(a, np.float64) for a in (x, y, s, qx, qy))
    assert x.shape == y.shape == s.shape and x.ndim == 1 and qx.shape == qy.shape and qx.ndim == 1
    fn = getattr(C.CDLL(lib_path), entry)
    fn.argtypes = [C.c_int32, _capi._pf64, _capi._pf64, _capi._pf64, C.c_int32, C.c_int32, _capi._pf64, _capi._pf64, _capi._pf64, _capi._pi32]
    s_out, idx = np.empty(qx.size, np.float64), np.empty((qx.size, 2), np.int32)
    pd = lambda a: a.ctypes.data_as(_capi._pf64)
    rc = fn(x.size, pd(x), pd(y), pd(s), int(bool(closed)), qx.size, pd(qx), pd(qy), pd(s_out), idx.ctypes.data_as(_capi._pi32))
    if rc != 0:
        raise _capi.BackendError("%s: status %d" % (entry, rc))
    return s_out, idx


def get_s_coord(x, y, s, closed, qx, qy):
    """The oracle's get_s_coord (oracle_get_s_coord) for arrays of queries on a caller's polyline: (s [nq], index pair [nq, 2])."""
    return _project(build(), "oracle_get_s_coord", x, y, s, closed, qx, qy)


def project_host(form, x, y, s, closed, qx, qy):
    """The host instantiation of project_on_polyline of csrc/planner_core.hpp (``form`` "planner_core") or csrc/fleet_core.hpp ("fleet_core")
    through oracle/planner_host_shim.cpp: (s [nq], index pair [nq, 2])."""
    from oracle import planner_host
    return _project(planner_host.build(), {"planner_core": "oracle_project_planner_core", "fleet_core": "oracle_project_fleet_core"}[form],
                    x, y, s, closed, qx, qy)


class OracleBackend(object):
    def __init__(self, lattice: Lattice):
        build()
        self.lib = C.CDLL(LIB)
        self.lib.oracle_plan_paths.argtypes = [C.POINTER(_capi.LatticeDesc), C.POINTER(_capi.PathsIn),
                                               C.POINTER(_capi.PathsOut)]
        self.lib.oracle_vel_profile.argtypes = [C.POINTER(_capi.LatticeDesc), C.POINTER(_capi.VelParams), C.c_int,
                                                C.POINTER(_capi.VelJob), C.POINTER(_capi.VelResult)]
        self.lib.oracle_process_objects.argtypes = [C.POINTER(_capi.LatticeDesc), C.POINTER(_capi.ObjectsIn),
                                                    C.POINTER(_capi.ObjectsOut)]
        self.has_tick = hasattr(self.lib, "oracle_tick_batch")
        if self.has_tick:
            self.lib.oracle_tick_batch.argtypes = [C.POINTER(_capi.LatticeDesc), C.POINTER(_capi.PathsIn),
                                                   C.POINTER(_capi.TickVelIn), C.POINTER(_capi.PathsOut),
                                                   C.POINTER(_capi.TickVelOut)]
        self.lattice = lattice
        self.binding = _capi.LatticeBinding(lattice)
        layers, edges, pts = lattice.max_horizon()
        self.caps = _capi.Caps(max_path_nodes=layers, max_path_pts=pts, max_horizon_edges=edges, device=-1,
                               num_cus=0, lds_bytes_paths=0)

    @staticmethod
    def _check(rc):
        if rc != 0:
            raise _capi.BackendError("oracle: status %d" % rc)

    def new_paths_result(self, n_scen):
        return _capi.PathsResult(n_scen, self.caps.max_path_nodes, self.caps.max_path_pts)

    def plan_paths(self, batch, result=None):
        if result is None:
            result = self.new_paths_result(batch.n_scen)
        self._check(self.lib.oracle_plan_paths(C.byref(self.binding.desc), C.byref(batch.struct),
                                               C.byref(result.struct)))
        return result

    def plan_paths_mask(self, batch, team_waves=0):
        """Checker of HipBackend.plan_paths_mask: blocked edges of every scenario (uint8 [n_scen, num_edges])."""
        import numpy as np
        self.lib.oracle_plan_paths_mask.argtypes = [C.POINTER(_capi.LatticeDesc), C.POINTER(_capi.PathsIn),
                                                    C.POINTER(_capi.PathsOut), C.c_void_p]
        result = self.new_paths_result(batch.n_scen)
        blocked = np.zeros((batch.n_scen, self.lattice.num_edges), np.uint8)
        self._check(self.lib.oracle_plan_paths_mask(C.byref(self.binding.desc), C.byref(batch.struct), C.byref(result.struct),
                                                    blocked.ctypes.data))
        return result, blocked

    def vel_profile(self, params, jobs):
        jarr, rarr, outs, keep = _capi.make_vel_jobs(jobs)
        self._check(self.lib.oracle_vel_profile(C.byref(self.binding.desc), C.byref(params.struct), len(jobs), jarr,
                                                rarr))
        return [(outs[i], bool(rarr[i].too_close), bool(rarr[i].vel_bound)) for i in range(len(jobs))]

    def _host(self):
        from oracle import planner_host
        if not hasattr(self, "_host_lib"):
            planner_host.build()
            self._host_lib = C.CDLL(planner_host.LIB)
            self._host_lib.oracle_const_segment_test.argtypes = [
                C.POINTER(_capi.LatticeDesc), _capi._pf64, C.c_int32, _capi._pf64, C.c_int32, _capi._pf64, _capi._pf64,
                _capi._pf64, _capi._pi32, _capi._pi32]
            self._host_lib.oracle_raceline_s.argtypes = [C.POINTER(_capi.LatticeDesc), C.c_double, C.c_double,
                                                         C.POINTER(C.c_double)]
        return self._host_lib

    def raceline_s(self, pos):
        s = C.c_double(0.0)
        self._check(self._host().oracle_raceline_s(C.byref(self.binding.desc), float(pos[0]), float(pos[1]), C.byref(s)))
        return float(s.value)

    def const_segment_test(self, const_path_seg, pos_est, vehicles):
        """Host logic of the product (csrc/planner_core.hpp) through the test harness library; no device arithmetic involved."""
        self._host()
        args = _capi.pack_const_segment_args(const_path_seg, pos_est, vehicles)
        flags, closest = C.c_int32(0), C.c_int32(-1)
        self._check(self._host_lib.oracle_const_segment_test(C.byref(self.binding.desc), *args[:7], C.byref(flags),
                                                             C.byref(closest)))
        return (bool(flags.value & _capi.FLAG_OBJ_IN_CONST), bool(flags.value & _capi.FLAG_OBJ_BESIDES),
                None if closest.value < 0 else int(closest.value))

    def process_objects(self, x, y, theta, v, length, dt=0.2):
        i, o, arrays, keep = _capi.make_objects(x, y, theta, v, length, dt)
        if i.n_obj > 0:
            self._check(self.lib.oracle_process_objects(C.byref(self.binding.desc), C.byref(i), C.byref(o)))
        return arrays

    def tick_batch(self, batch, vel, result=None, vresult=None):
        if not self.has_tick:
            raise _capi.BackendError("oracle_tick_batch not built")
        if result is None:
            result = self.new_paths_result(batch.n_scen)
        if vresult is None:
            vresult = _capi.TickVelResult(batch.n_scen, result.cap_pts)
        self._check(self.lib.oracle_tick_batch(C.byref(self.binding.desc), C.byref(batch.struct),
                                               C.byref(vel.struct), C.byref(result.struct), C.byref(vresult.struct)))
        return result, vresult
