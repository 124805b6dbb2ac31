"""
GPU: the resident single-tick kernel (k_tick_persistent, ltpl_create_ex(LTPL_CREATE_PERSISTENT_TICK)) next to MANY other handles of the
process. The kernel never completes, so a kernel launched on a stream that shares its hardware queue waits until it idles out, and the
next persistent tick has to start it again. The runtime maps the streams of a process onto a few hardware queues (four by
default) per stream priority; the resident kernel's stream is created at the highest priority, which nothing else in the library uses by
default, so no other stream shares its queue however many there are. Here six other handles -- more streams than hardware queues, so
every normal-priority queue carries some of them -- each launch a tick between any two persistent ticks: one start, the kernel stays
resident, results identical.
"""
import pytest

import test_gpu_persistent_tick as pt
from graphbasedlocaltrajectoryplanner_amd import _capi

pytestmark = pytest.mark.gpu

N_OTHERS = 6
N_TICKS = 10


def test_resident_kernel_is_started_once_with_more_handles_open_than_hardware_queues(monteblanco, monkeypatch):
    monkeypatch.setenv("LTPL_PERSIST_IDLE_MS", "100")
    others = [_capi.HipBackend(monteblanco) for _ in range(N_OTHERS)]
    pers = _capi.HipBackend(monteblanco, persistent_tick=True)
    try:
        for i, (b, v) in enumerate(pt.single_ticks(monteblanco, N_TICKS, seed=21)):
            got = pers.tick_batch(b, v)
            for k, other in enumerate(others):
                pt.assert_same_tick(got, other.tick_batch(b, v), "tick %d handle %d" % (i, k))
        st = pers.persistent_stats()
        assert st["ticks"] == N_TICKS and st["launches"] == 1 and st["resident"] == 1, st
    finally:
        pers.close()
        for other in others:
            other.close()
    pt.device_synchronize()
