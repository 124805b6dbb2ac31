"""GPU: the velocity kernels against the long-double reference tests/vel_ref.py, at their decision boundaries.

SEAM (k_vel_profile, the wave form of csrc/vel_wave.hpp): ltpl_vel_profile on every family of tests/vel_cases.py at each of the six
variants -- too_close and vel_bound exact, vx within the derived bound of vel_cases.BOUNDS (class = exponent, part = the row's radicand)
and exactly 0 where the reference is 0; a failure names the job and the row. One call per group (jobs of both gg forms, all lengths and
modes mixed; the family `chunk` holds the chunk-edge lengths and the longest accepted job) and one call with a single job per group; an
opponent that never stops within a lap on an 80 m oval with a handle of its own.

TICK ROUTES (k_tick; k_follow_prep + k_vel_lanes + k_vel_final; k_tick_persistent): the twelve batches of vel_cases.tick_inputs at the
smallest sizes that take each route -- 5 and 48 scenarios fused, 96 through k_vel_final, 255 / 256 on either side of LTPL_EMIT_MIN_SCEN,
256 with the follow jobs finished by the lane kernel (the suite's handle) and by two waves (a handle of its own), six single ticks on the
resident kernel. The reference is evaluated on the DEVICE'S OWN path_param columns (held to 1e-10 by the assembly tests), once per batch
on the 256-scenario run; every route's path_param is asserted bit-identical to it. Flags, n_pts, the positions of zeros and of -5 exact;
vx and ax within bound on every decision-stable slot (fp64 and long-double traces of vel_ref equal); unstable slots keep the comparison
with the oracle at the project's 1e-5, and their share is asserted <= 2 % again on the device's paths.

What one run on an MI355X measured is in the comment block below (every test prints its lines; run with `pytest -s`).
"""
# MEASURED (one run on an MI355X): worst element-wise deviation from the long-double reference, relative with the floors 1 m/s / 0.5 m/s^2.
# Seam, per variant and family (the bounds: vel_cases.BOUNDS; the standstill and radicand families hold the ill-conditioned rows):
#   exp1-1rows-PD      table 2.7e-15  runs 2.1e-15  vmax 2.9e-16  radicand 7.4e-13  standstill 1.2e-09  follow 2.9e-13  chunk 3.7e-14
#   exp1-5rows-PD      table 4.3e-16  runs 2.4e-16  vmax 1.9e-16  radicand 7.4e-13  standstill 1.2e-09  follow 2.9e-13  chunk 8.4e-14
#   exp2-1rows-PDtan   table 5.0e-16  runs 3.2e-16  vmax 2.9e-16  radicand 3.4e-07  standstill 1.7e-09  follow 4.7e-14  chunk 1.1e-07
#   exp2-3rows-PD      table 6.6e-16  runs 4.1e-16  vmax 1.9e-16  radicand 3.4e-07  standstill 1.7e-09  follow 4.7e-14  chunk 9.8e-08
#   exp1.5-1rows-PD    table 5.1e-16  runs 3.4e-16  vmax 3.1e-16  radicand 2.9e-09  standstill 2.2e-10  follow 4.7e-14  chunk 4.7e-10
#   exp1.5-2rows-PDtan table 4.3e-16  runs 3.2e-16  vmax 2.1e-16  radicand 2.9e-09  standstill 2.2e-10  follow 4.7e-14  chunk 6.1e-11
#   exp1-1rows-PD      short lap: worst 5.8e-16
#   exp1-5rows-PD      short lap: worst 2.9e-16
#   exp2-1rows-PDtan   short lap: worst 2.9e-16
#   exp2-3rows-PD      short lap: worst 2.9e-16
#   exp1.5-1rows-PD    short lap: worst 2.8e-16
#   exp1.5-2rows-PDtan short lap: worst 2.9e-16
# Tick, per parameter set and route, both generators together (valid slots compared / decision-unstable among them):
#   exp1_row     k_tick (5, 48)               vx 2.4e-13 ax 4.3e-13    130 slots, 0 unstable
#   exp1_row     k_vel_final (96)             vx 2.1e-12 ax 1.8e-12    237 slots, 0 unstable
#   exp1_row     k_vel_final (255)            vx 2.1e-12 ax 1.8e-12    641 slots, 0 unstable
#   exp1_row     lanes emit (256)             vx 2.1e-12 ax 1.8e-12    645 slots, 0 unstable
#   exp1_table   k_tick (5, 48)               vx 1.4e-13 ax 4.3e-13    130 slots, 0 unstable
#   exp1_table   k_vel_final (96)             vx 6.2e-13 ax 1.4e-12    237 slots, 0 unstable
#   exp1_table   k_vel_final (255)            vx 1.1e-12 ax 1.4e-12    641 slots, 0 unstable
#   exp1_table   lanes emit (256)             vx 1.1e-12 ax 1.4e-12    645 slots, 0 unstable
#   exp1p5_row   k_tick (5, 48)               vx 1.5e-12 ax 1.4e-10    130 slots, 0 unstable
#   exp1p5_row   k_vel_final (96)             vx 2.4e-12 ax 7.3e-10    237 slots, 0 unstable
#   exp1p5_row   k_vel_final (255)            vx 4.7e-12 ax 1.1e-09    641 slots, 0 unstable
#   exp1p5_row   lanes emit (256)             vx 4.7e-12 ax 1.1e-09    645 slots, 0 unstable
#   exp1p5_table k_tick (5, 48)               vx 4.1e-12 ax 3.7e-10    130 slots, 0 unstable
#   exp1p5_table k_vel_final (96)             vx 6.5e-12 ax 1.9e-09    237 slots, 0 unstable
#   exp1p5_table k_vel_final (255)            vx 1.2e-11 ax 2.8e-09    641 slots, 0 unstable
#   exp1p5_table lanes emit (256)             vx 1.2e-11 ax 2.8e-09    645 slots, 0 unstable
#   exp2_row     k_tick (5, 48)               vx 5.1e-08 ax 4.9e-06    130 slots, 0 unstable
#   exp2_row     k_vel_final (96)             vx 3.5e-08 ax 4.9e-06    237 slots, 0 unstable
#   exp2_row     k_vel_final (255)            vx 9.8e-08 ax 6.5e-06    641 slots, 0 unstable
#   exp2_row     lanes emit (256)             vx 9.8e-08 ax 6.5e-06    645 slots, 0 unstable
#   exp2_table   k_tick (5, 48)               vx 2.2e-09 ax 1.5e-07    130 slots, 0 unstable
#   exp2_table   k_vel_final (96)             vx 3.0e-09 ax 3.9e-07    237 slots, 0 unstable
#   exp2_table   k_vel_final (255)            vx 5.0e-09 ax 5.4e-07    641 slots, 0 unstable
#   exp2_table   lanes emit (256)             vx 5.0e-09 ax 5.4e-07    645 slots, 0 unstable
#   exp1_row     two-wave follow (256)        vx 2.1e-12 ax 1.8e-12    645 slots, 0 unstable
#   exp1_table   two-wave follow (256)        vx 1.1e-12 ax 1.4e-12    645 slots, 0 unstable
#   exp1p5_row   two-wave follow (256)        vx 4.7e-12 ax 1.1e-09    645 slots, 0 unstable
#   exp1p5_table two-wave follow (256)        vx 1.2e-11 ax 2.8e-09    645 slots, 0 unstable
#   exp2_row     two-wave follow (256)        vx 9.8e-08 ax 6.5e-06    645 slots, 0 unstable
#   exp2_table   two-wave follow (256)        vx 5.0e-09 ax 5.4e-07    645 slots, 0 unstable
#   exp1_row     k_tick_persistent (6 ticks)  vx 2.4e-15 ax 3.0e-14      7 slots, 0 unstable
#   exp1_table   k_tick_persistent (6 ticks)  vx 1.4e-14 ax 1.2e-13      7 slots, 0 unstable
#   exp1p5_row   k_tick_persistent (6 ticks)  vx 2.1e-14 ax 1.4e-12      7 slots, 0 unstable
#   exp1p5_table k_tick_persistent (6 ticks)  vx 3.2e-14 ax 3.6e-12      7 slots, 0 unstable
#   exp2_row     k_tick_persistent (6 ticks)  vx 1.9e-09 ax 2.7e-07      7 slots, 0 unstable
#   exp2_table   k_tick_persistent (6 ticks)  vx 2.4e-11 ax 4.7e-09      7 slots, 0 unstable
# Every slot of every batch was decision-stable on the device's paths. Exponent 2: the kernels stand 9.8e-8 (vx) / 6.5e-6 (ax) from long
# double on the ill-conditioned rows, the oracle 3.5e-8 / 1.9e-6 on the same batches (tests/test_vel_cases_host.py): both are the model's
# conditioning at the friction limit, the oracle about three times nearer; on the regular rows both are below 5e-12.
import numpy as np
import pytest

import vel_ref as R
import vel_cases as C
from helpers import assert_vx_elementwise, assert_ax_elementwise
from vel_jobs import VARIANT_IDS
from test_gpu_vel import largest_accepted_n
from test_gpu_vel_variants import SETS, NAMES
from test_gpu_default_routes import default_backend, sub_batch
from test_gpu_persistent_tick import device_synchronize
from graphbasedlocaltrajectoryplanner_amd import _capi

pytestmark = pytest.mark.gpu
LD = R.LD


# ---------------------------------------------------------------- seam

class SeamRefs(object):
    """Long-double results of every group of a variant, computed once per module."""

    def __init__(self, lat):
        self.lat, self.made = lat, {}

    def of(self, key, vp, jobs):
        if key not in self.made:
            P, idx = R.Params(vp), C.opp_index(self.lat, jobs)
            self.made[key] = [R.run_job(P, jb, self.lat.glob_rl, ix, LD) for jb, ix in zip(jobs, idx)]
        return self.made[key]


@pytest.fixture(scope="module")
def seam_refs(monteblanco):
    return SeamRefs(monteblanco)


def check_seam(k, vp, jobs, got, refs):
    cls, worst = R.exp_class(R.Params(vp).exp), 0.0
    assert len(got) == len(jobs) == len(refs)
    for jb, (vx, tc, vb), ref in zip(jobs, got, refs):
        what = "variant %s job '%s' (mode %d, n %d)" % (VARIANT_IDS[k], jb["name"], jb["mode"], jb["kappa"].size)
        assert tc == ref[1], what + ": too_close %d, reference %d" % (tc, ref[1])
        assert vb == ref[2], what + ": vel_bound %d, reference %d" % (vb, ref[2])
        worst = max(worst, C.check_rows(cls, "vx", vx, ref[0], ref[4], what))
    return worst


@pytest.mark.parametrize("k", range(6), ids=VARIANT_IDS)
def test_vel_profile_matches_long_double_on_the_boundary_families(monteblanco, hip_backend, seam_refs, k):
    worst = {}
    groups = C.families(monteblanco, k)
    for g, (fam, name, vp, jobs) in enumerate(groups):
        assert all(a["kappa"].size != b["kappa"].size or a["mode"] != b["mode"] or not np.array_equal(a["loc_gg"], b["loc_gg"]) for a, b in zip(jobs, jobs[1:]))
        refs = seam_refs.of((k, g), vp, jobs)
        worst[fam] = max(worst.get(fam, 0.0), check_seam(k, vp, jobs, hip_backend.vel_profile(vp, jobs), refs))
        if len(jobs) > 1:                                          # ... and a call with a single job
            check_seam(k, vp, jobs[-1:], hip_backend.vel_profile(vp, jobs[-1:]), refs[-1:])
    print("vel_ref seam: %-18s %s" % (VARIANT_IDS[k], "  ".join("%s %.1e" % (f, worst[f]) for f, _ in C.BUILDERS)))


def test_the_chunk_family_holds_the_longest_accepted_job(monteblanco, hip_backend):
    assert largest_accepted_n(hip_backend, monteblanco) == C.LONGEST_N


@pytest.mark.parametrize("k", range(6), ids=VARIANT_IDS)
def test_vel_profile_on_a_short_lap_behind_an_opponent_that_never_stops(k):
    """vel_cases.short_lap_case on a handle of its own: the opponent's stop scan runs the whole lap of the 80 m oval and ends there."""
    lat, vp, jobs = C.short_lap_case(k)
    P, idx = R.Params(vp), C.opp_index(lat, jobs)
    refs = [R.run_job(P, jb, lat.glob_rl, ix, LD) for jb, ix in zip(jobs, idx)]
    assert refs[0][3][2] == lat.glob_rl.shape[0] - 1
    hip = _capi.HipBackend(lat)
    try:
        worst = check_seam(k, vp, jobs, hip.vel_profile(vp, jobs), refs)
    finally:
        hip.close()
    print("vel_ref seam: %-18s short lap: worst %.1e" % (VARIANT_IDS[k], worst))


# ---------------------------------------------------------------- tick routes

class TickRefs(object):
    """(parameter set, generator) -> the 256-scenario batch, the device's result on the suite's handle and vel_ref's two evaluations on the
    device's paths; made on first use, kept for the module."""

    def __init__(self, lat, hip):
        self.lat, self.hip, self.made = lat, hip, {}

    def get(self, name, gen):
        if (name, gen) not in self.made:
            scen, vels, batch, vel = C.tick_inputs(self.lat, name, gen)
            res, vres = self.hip.tick_batch(batch, vel)
            obj = R.tick_objects(self.lat, batch, vel, res)
            f64 = R.tick_batch_ref(self.lat, batch, vel, res, np.float64, obj)
            ld = R.tick_batch_ref(self.lat, batch, vel, res, LD, obj)
            self.made[name, gen] = (scen, vels, vel, res, vres, f64, ld)
        return self.made[name, gen]


@pytest.fixture(scope="module")
def tick_refs(monteblanco, hip_backend):
    return TickRefs(monteblanco, hip_backend)


def check_tick(name, gen, route, res, vres, full, f64, ld, oracle, lo=0):
    """The slots of ``res`` (scenarios lo .. lo + n_scen - 1 of the batch) against the references of the whole batch."""
    cls = R.exp_class(SETS[name][0])
    wv = wa = 0.0
    n_slots = unstable = 0
    for s in range(res.n_scen):
        assert np.array_equal(res.valid[s], full.valid[lo + s]) and np.array_equal(res.n_pts[s], full.n_pts[lo + s]), (route, s)
        for a in np.flatnonzero(res.valid[s] == 1):
            key, n = (lo + s, int(a)), int(res.n_pts[s, a])
            what = "%s %s %s scenario %d slot %d" % (name, gen, route, lo + s, a)
            assert np.array_equal(res.path_param[s, a, :n], full.path_param[lo + s, a, :n]), what + ": path_param differs between routes"
            n_slots += 1
            vx, ax = vres.vx[s, a, :n], vres.ax[s, a, :n]
            if f64[key].trace != ld[key].trace:
                unstable += 1
                _, ovr = oracle()
                assert (vres.too_close[s, a], vres.vel_bound[s, a]) == (ovr.too_close[lo + s, a], ovr.vel_bound[lo + s, a]), what
                assert_vx_elementwise(vx, ovr.vx[lo + s, a, :n], what)
                assert_ax_elementwise(ax, ovr.ax[lo + s, a, :n], what)
                continue
            b = ld[key]
            assert (vres.too_close[s, a], vres.vel_bound[s, a]) == (b.too_close, b.vel_bound), what + ": flags %r, reference %r" % (
                (vres.too_close[s, a], vres.vel_bound[s, a]), (b.too_close, b.vel_bound))
            still = np.asarray(b.vx == 0)                   # the -5 of standstill (elsewhere an ax of -5 is a deceleration at gg's limit, held by the bound)
            assert np.array_equal((ax == -5.0)[still], np.asarray(b.ax == -5)[still]), what + ": positions of ax = -5"
            wv = max(wv, C.check_rows(cls, "vx", vx, b.vx, b.rad, what))
            wa = max(wa, C.check_rows(cls, "ax", ax, b.ax, C.ax_rad(b.rad), what))
    return n_slots, unstable, wv, wa


def run_routes(lat, hip, tick_refs, name, gen, route, sizes):
    scen, vels, vel, full, _, f64, ld = tick_refs.get(name, gen)
    cache = {}

    def oracle():
        if "o" not in cache:
            from oracle.oracle_lib import OracleBackend
            cache["o"] = OracleBackend(lat).tick_batch(*sub_batch(scen, vels, vel, 0, C.TICK_N))
        return cache["o"]
    for n in sizes:
        batch, v = sub_batch(scen, vels, vel, 0, n)
        res, vres = hip.tick_batch(batch, v)
        n_slots, unstable, wv, wa = check_tick(name, gen, route, res, vres, full, f64, ld, oracle)
        print("vel_ref tick: %-12s %-6s %-22s n %3d  slots %3d unstable %d  vx %.1e ax %.1e" % (name, gen, route, n, n_slots, unstable, wv, wa))
        assert unstable <= C.UNSTABLE_SHARE * n_slots


@pytest.mark.parametrize("gen", C.TICK_GENS)
@pytest.mark.parametrize("name", NAMES)
def test_tick_routes_of_the_suites_handle_match_long_double(monteblanco, hip_backend, tick_refs, name, gen):
    """5 and 48 scenarios: fused k_tick; 96: k_follow_prep + k_vel_lanes + k_vel_final; 255 and 256: generic jobs written by k_vel_final and
    by the lane kernel (LTPL_EMIT_MIN_SCEN = 256); 256: follow jobs finished by the lane kernel (LTPL_FOLLOW_EMIT_MIN_SCEN = 256 in the suite)."""
    run_routes(monteblanco, hip_backend, tick_refs, name, gen, "suite handle", (5, 48, 96, 255, 256))


@pytest.fixture(scope="module")
def two_wave_backend(monteblanco):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("LTPL_FOLLOW_EMIT_MIN_SCEN", "1000000")
        hip = _capi.HipBackend(monteblanco)
    yield hip
    hip.close()


@pytest.mark.parametrize("gen", C.TICK_GENS)
@pytest.mark.parametrize("name", NAMES)
def test_tick_with_two_wave_follow_jobs_matches_long_double(monteblanco, two_wave_backend, tick_refs, name, gen):
    run_routes(monteblanco, two_wave_backend, tick_refs, name, gen, "two-wave follow", (256,))


@pytest.mark.parametrize("name", NAMES)
def test_resident_tick_kernel_matches_long_double(monteblanco, tick_refs, name, monkeypatch):
    """k_tick_persistent: six single ticks (scenarios 0 .. 2 of both batches) on a handle with the resident kernel."""
    monkeypatch.setenv("LTPL_PERSIST_IDLE_MS", "1000")
    pers = default_backend(monteblanco, persistent_tick=True)
    try:
        assert pers.persistent_stats()["enabled"] == 1
        for gen in C.TICK_GENS:
            scen, vels, vel, full, _, f64, ld = tick_refs.get(name, gen)
            for i in range(3):
                batch, v = sub_batch(scen, vels, vel, i, i + 1)
                res, vres = pers.tick_batch(batch, v)
                assert all(f64[i, int(a)].trace == ld[i, int(a)].trace for a in np.flatnonzero(res.valid[0] == 1)), "unstable slot in scenario %d" % i
                n_slots, unstable, wv, wa = check_tick(name, gen, "k_tick_persistent", res, vres, full, f64, ld, None, lo=i)
                print("vel_ref tick: %-12s %-6s %-22s tick %d  slots %3d  vx %.1e ax %.1e" % (name, gen, "k_tick_persistent", i, n_slots, wv, wa))
        assert pers.persistent_stats()["ticks"] == 6
    finally:
        pers.close()
        device_synchronize()
