"""-m gpu: a body in prescribed rigid motion through the C host mirror (NSSetImmersedBoundaryMotion, include/fluca_host.h).

Every NSStep asks the callback for the pose at t + dt, moves the markers (fl_ibm_update; with -ns_ibm_marker_distribution owner fl_ibm_migrate,
reference positions and volumes travelling with a marker that changes rank) and forces with them.  Checked here: the channel of
tests/test_gpu_config5.py with its cylinder oscillating across the y split plane while it turns, eight ranks with both marker distributions
against the undecomposed run; one rank against the CPU oracle's step with the markers moved by the same pose formula in numpy; the error paths."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import inproc
from tests.flow_parity import sphere_markers
from tests.test_gpu_config5 import C5_BC, CH_BOX, Case, _cylinder, _gather
from tests.test_gpu_ibm_owner import _extra_options, _geometry

pytestmark = pytest.mark.gpu

N, RANKS, NSTEPS, DT = (32, 24, 16), (2, 2, 2), 3, 5e-3
CALLBACK_ERROR = 77


# ------------------------------------------------------------------------------------------------ the motion

class Motion:
    """centre(t) = centre0 + (0, A sin(2 pi t / T), 0), turning about z at the rate w: A = 2 h, T = 4 pi dt (the peak speed A 2 pi / T is one h per
    step), w = 0.05 rad per step"""

    def __init__(self, centre0, h, dt):
        self.c0, self.A, self.T, self.w = np.asarray(centre0, dtype=float), 2.0 * h, 4.0 * np.pi * dt, 0.05 / dt

    def pose(self, t):
        ph = 2.0 * np.pi * t / self.T
        return (self.c0 + [0.0, self.A * np.sin(ph), 0.0], np.array([0.0, 0.0, self.w * t]),
                np.array([0.0, self.A * 2.0 * np.pi / self.T * np.cos(ph), 0.0]), np.array([0.0, 0.0, self.w]))

    def markers(self, X0, t):
        """positions and target velocities (3, L) of the markers X0 at time t: Rodrigues' rotation about z"""
        c, rv, vel, om = self.pose(t)
        r0 = np.stack(X0) - self.c0[:, None]
        cs, sn = np.cos(rv[2]), np.sin(rv[2])
        r = np.stack([cs * r0[0] - sn * r0[1], sn * r0[0] + cs * r0[1], r0[2]])
        return [np.ascontiguousarray(a) for a in c[:, None] + r], vel[:, None] + np.cross(om, r, axis=0)

    def callback(self, H, fail_at=None):
        @H.BodyMotionFunc
        def fn(t, centre, rotvec, velocity, omega, ctx):
            if fail_at is not None and t >= fail_at:
                return CALLBACK_ERROR
            for dst, src in zip((centre, rotvec, velocity, omega), self.pose(t)):
                dst[0], dst[1], dst[2] = src
            return 0
        return fn


def _channel_cylinder():
    Lx, Ly, Lz = CH_BOX
    h = Lx / N[0]
    X0 = _cylinder([(0.0, Lx), (0.0, Ly), (0.0, Lz)], h, radius_cells=3.0)
    return h, X0, Motion((0.5 * Lx, 0.5 * Ly, 0.5 * Lz), h, DT)


# ------------------------------------------------------------------------------------------------ the run (tests/test_gpu_config5.py's _mirror_run with a motion)

def _moving_run(R, moving, fail_rank=None, early=False):
    """_mirror_run's channel with its cylinder; moving: the Motion above; fail_rank: that rank's callback (-1: everybody's) fails in the second step;
    early: NSSetImmersedBoundaryMotion is also tried before NSSetImmersedBoundary.  -> this rank's blocks of v, V, p and the return codes."""
    from fluca_amd import capi, hostapi as H
    P = C.c_void_p
    Lx, Ly, Lz = CH_BOX
    n = N
    rank, size = (0, 1) if R is None else (R.rank, R.size)
    rk = RANKS if size > 1 else (1, 1, 1)
    mesh = P()
    assert H.lib.MeshCartCreate3d(0, 0, 1, n[0], n[1], n[2], rk[0], rk[1], rk[2], None, None, None, C.byref(mesh)) == 0
    assert H.lib.MeshSetRank(mesh, rank, size) == 0
    assert H.lib.MeshSetUp(mesh) == 0
    assert H.lib.MeshCartSetUniformCoordinates(mesh, 0., Lx, 0., Ly, 0., Lz) == 0
    ns = P()
    assert H.lib.NSCreate(C.byref(ns)) == 0 and H.lib.NSSetType(ns, b"cnlinear") == 0 and H.lib.NSSetMesh(ns, mesh) == 0
    assert H.lib.NSSetDensity(ns, 1.0) == 0 and H.lib.NSSetViscosity(ns, 0.05) == 0

    @H.BCFunc
    def inlet(dim, t, x, val, ctx):
        val[0], val[1], val[2] = 4.0 * x[1] * (Ly - x[1]) / Ly ** 2 * (1.0 + 0.3 * np.sin(2 * np.pi * x[2] / Lz)), 0.0, 0.0
        return 0

    @H.BCFunc
    def wall(dim, t, x, val, ctx):
        val[0] = val[1] = val[2] = 0.0
        return 0

    @H.BCFunc
    def outlet(dim, t, x, val, ctx):
        val[0] = 0.3 * np.sin(3.0 * t) + 0.1 * x[1]
        return 0

    bcs = [H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=inlet), H.NSBoundaryCondition(type=H.NS_BC_PRESSURE_OUTLET, pressure=outlet),
           H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=wall), H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=wall),
           H.NSBoundaryCondition(type=H.NS_BC_PERIODIC), H.NSBoundaryCondition(type=H.NS_BC_PERIODIC)]
    for b in range(6):
        assert H.lib.NSSetBoundaryCondition(ns, b, bcs[b]) == 0
    argc, av = H.argv("-ns_time_step_size", DT, "-ns_max_steps", NSTEPS, "-ns_ksp_rtol", 1e-10, "-ns_abf_schur_ksp_type", "bcgs",
                      "-ns_abf_schur_ksp_rtol", 1e-12, "-ns_abf_momentum_ksp_rtol", 1e-12)
    assert H.lib.NSSetFromOptions(ns, argc, av) == 0 and H.lib.NSSetUp(ns) == 0
    hp = P()
    assert H.lib.NSGetPoisson(ns, C.byref(hp)) == 0
    if R is not None:
        R.attach(hp)
    h, X, motion = _channel_cylinder()
    L = X[0].size
    keep = []
    for a in X + [np.full(L, h ** 3)]:
        dptr = P()
        capi.check(capi.lib.fl_malloc(0, a.size * 8, C.byref(dptr)))
        capi.check(capi.lib.fl_memcpy_h2d(0, dptr, np.ascontiguousarray(a).ctypes.data_as(C.c_void_p), a.size * 8))
        keep.append(dptr)
    res = {}
    c0 = (C.c_double * 3)(*motion.c0)
    fails = fail_rank is not None and fail_rank in (-1, rank)
    fn = motion.callback(H, fail_at=1.5 * DT if fails else None)
    if early:
        res["early_rc"] = H.lib.NSSetImmersedBoundaryMotion(ns, c0, fn, None)
    assert H.lib.NSSetImmersedBoundary(ns, 0, L, keep[0], keep[1], keep[2], keep[3], None) == 0
    if moving:
        assert H.lib.NSSetImmersedBoundaryMotion(ns, c0, fn, None) == 0
    res["solve_rc"] = H.lib.NSSolve(ns)
    step = C.c_int64(-1)
    assert H.lib.NSGetTimeStep(ns, C.byref(step)) == 0
    res["steps"] = step.value
    sz = (C.c_int64 * 4)()
    assert H.lib.NSGetLocalSizes(ns, sz) == 0
    cc = [C.c_int64() for _ in range(6)]
    assert H.lib.MeshCartGetCorners(mesh, *[C.byref(q) for q in cc]) == 0
    v, p, Vp = P(), P(), (C.c_void_p * 3)()
    assert H.lib.NSGetSolutionArrays(ns, C.byref(v), Vp, C.byref(p)) == 0

    def get(ptr, m):
        out = np.empty(m)
        capi.check(capi.lib.fl_memcpy_d2h(0, out.ctypes.data_as(C.c_void_p), ptr, m * 8))
        return out

    res.update(lo=[q.value for q in cc[:3]], ln=[q.value for q in cc[3:]], v=get(v, 3 * sz[0]), p=get(p, sz[0]), V=[get(C.c_void_p(Vp[d]), sz[1 + d]) for d in range(3)])
    H.lib.NSDestroy(C.byref(ns))
    H.lib.MeshDestroy(C.byref(mesh))
    for dptr in keep:
        capi.lib.fl_free(0, dptr)
    return res


@functools.lru_cache(maxsize=None)
def _one_rank(moving):
    parts = inproc.run_threads(1, lambda R: _moving_run(None, moving, early=moving))
    assert parts[0]["solve_rc"] == 0 and parts[0]["steps"] == NSTEPS
    return parts, _gather(parts, N)


def _eight_ranks_against_one(distribution):
    with _extra_options("-ns_ibm_marker_distribution", distribution):
        parts = inproc.run_threads(8, _moving_run, True)
    assert all(r["solve_rc"] == 0 and r["steps"] == NSTEPS for r in parts)
    v, V, p = _gather(parts, N)
    _, (v1, V1, p1) = _one_rank(True)
    assert np.linalg.norm(v - v1) <= 1e-8 * np.linalg.norm(v1)
    for d in range(3):
        assert np.linalg.norm(V[d] - V1[d]) <= 1e-8 * max(np.linalg.norm(V1[d]), 1e-12), d
    assert np.linalg.norm(p - p1) <= 1e-7 * np.linalg.norm(p1)


# ------------------------------------------------------------------------------------------------ eight ranks against one

def test_the_moving_cylinder_with_owner_rank_markers_on_the_2x2x2_rank_grid():
    """v and V to 1e-8, p to 1e-7 against the undecomposed run: the bounds the resting body is held to.  Markers change rank on the way (counted from
    geometry), so fl_ibm_migrate carries reference positions and volumes across."""
    h, X0, motion = _channel_cylinder()
    Lx, Ly, Lz = CH_BOX
    case = Case(n=N, ranks=RANKS, bc=C5_BC, box=[(0.0, Lx), (0.0, Ly), (0.0, Lz)])
    owners = [_geometry(case, 0, motion.markers(X0, k * DT)[0])[0] for k in range(NSTEPS + 1)]
    changes = [int((a != b).sum()) for a, b in zip(owners, owners[1:])]
    print("markers that change owner rank per step:", changes, "of", X0[0].size)
    assert sum(changes) >= 1
    _eight_ranks_against_one("owner")


def test_the_moving_cylinder_with_replicated_markers_on_the_2x2x2_rank_grid():
    _eight_ranks_against_one("replicated")


def test_the_motion_changes_the_flow():
    _, (v1, _, _) = _one_rank(True)
    _, (vr, _, _) = _one_rank(False)
    assert np.linalg.norm(v1 - vr) >= 1e-3 * np.linalg.norm(vr)


# ------------------------------------------------------------------------------------------------ error paths

def test_a_failing_callback_ends_the_step_with_its_code_on_every_rank():
    """the callback fails in the second step -- everybody's, then rank 3's alone (the others learn of it through the vote: nobody waits in a collective
    call that rank 3 never enters; the wire's time limit would fail the test)"""
    for who in (-1, 3):
        with _extra_options("-ns_ibm_marker_distribution", "owner"):
            parts = inproc.run_threads(8, _moving_run, True, who, wire_timeout=30.0)
        assert [r["solve_rc"] for r in parts] == [CALLBACK_ERROR] * 8, (who, [r["solve_rc"] for r in parts])
        assert [r["steps"] for r in parts] == [1] * 8


def test_a_motion_needs_an_immersed_boundary():
    from fluca_amd import hostapi as H
    parts, _ = _one_rank(True)
    assert parts[0]["early_rc"] == H.ERR_ARG_WRONGSTATE


# ------------------------------------------------------------------------------------------------ one rank against the oracle's step

def test_a_moving_sphere_matches_the_oracle_step():
    """tests/test_gpu_flow_parity.py's channel with the immersed sphere at 32^3, the sphere now oscillating in y and turning about z: the oracle's ibm
    dict receives X and Ut of t + dt from the same pose formula in numpy before every step.  Bounds: those the resting sphere is held to there."""
    from fluca_amd import capi, hostapi as H
    from oracle import fluca_oracle as fo
    P = C.c_void_p
    n, nsteps, Re, D = 32, 2, 100.0, 8
    rho, mu, dt = 1.0, 1.0 / Re, 0.5 / n
    X0, dV = sphere_markers(n, D)
    L = X0[0].size
    motion = Motion((0.5, 0.5, 0.5), 1.0 / n, dt)
    mesh = P()
    assert H.lib.MeshCartCreate3d(0, 0, 1, n, n, n, -1, -1, -1, None, None, None, C.byref(mesh)) == 0
    assert H.lib.MeshSetUp(mesh) == 0
    assert H.lib.MeshCartSetUniformCoordinates(mesh, 0., 1., 0., 1., 0., 1.) == 0
    ns = P()
    assert H.lib.NSCreate(C.byref(ns)) == 0 and H.lib.NSSetType(ns, b"cnlinear") == 0 and H.lib.NSSetMesh(ns, mesh) == 0
    assert H.lib.NSSetDensity(ns, rho) == 0 and H.lib.NSSetViscosity(ns, mu) == 0

    @H.BCFunc
    def inlet(dim, t, x, val, ctx):
        val[0], val[1], val[2] = 4.0 * x[1] * (1.0 - x[1]), 0.0, 0.0
        return 0

    @H.BCFunc
    def zero(dim, t, x, val, ctx):
        val[0] = val[1] = val[2] = 0.0
        return 0

    bcs = [H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=inlet), H.NSBoundaryCondition(type=H.NS_BC_PRESSURE_OUTLET, pressure=zero),
           H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=zero), H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=zero),
           H.NSBoundaryCondition(type=H.NS_BC_PERIODIC), H.NSBoundaryCondition(type=H.NS_BC_PERIODIC)]
    for b in range(6):
        assert H.lib.NSSetBoundaryCondition(ns, b, bcs[b]) == 0
    argc, av = H.argv("-ns_time_step_size", dt, "-ns_max_steps", nsteps, "-ns_ksp_rtol", 1e-9, "-ns_abf_schur_ksp_rtol", 1e-11,
                      "-ns_abf_momentum_ksp_rtol", 1e-11, "-ns_abf_schur_ksp_max_it", 50000)
    assert H.lib.NSSetFromOptions(ns, argc, av) == 0 and H.lib.NSSetUp(ns) == 0
    keep = []
    for a in X0 + [dV]:
        dptr = P()
        capi.check(capi.lib.fl_malloc(0, a.size * 8, C.byref(dptr)))
        capi.check(capi.lib.fl_memcpy_h2d(0, dptr, np.ascontiguousarray(a).ctypes.data_as(C.c_void_p), a.size * 8))
        keep.append(dptr)
    assert H.lib.NSSetImmersedBoundary(ns, 0, L, keep[0], keep[1], keep[2], keep[3], None) == 0
    fn = motion.callback(H)
    assert H.lib.NSSetImmersedBoundaryMotion(ns, (C.c_double * 3)(*motion.c0), fn, None) == 0
    assert H.lib.NSSolve(ns) == 0
    bc = [fo.BC_VELOCITY, fo.BC_PRESSURE_OUTLET, fo.BC_VELOCITY, fo.BC_VELOCITY, fo.BC_PERIODIC, fo.BC_PERIODIC]
    g = fo.Grid.uniform((n, n, n), [(0, 1), (0, 1), (0, 1)], bc, dt / rho)
    v, p, Vp = P(), P(), (C.c_void_p * 3)()
    assert H.lib.NSGetSolutionArrays(ns, C.byref(v), Vp, C.byref(p)) == 0

    def get(ptr, m):
        out = np.empty(m)
        capi.check(capi.lib.fl_memcpy_d2h(0, out.ctypes.data_as(C.c_void_p), ptr, m * 8))
        return out

    vg, pg = get(v, 3 * g.ncell), get(p, g.ncell)
    Vg = [get(C.c_void_p(Vp[d]), g.nface[d]) for d in range(3)]
    H.lib.NSDestroy(C.byref(ns))
    H.lib.MeshDestroy(C.byref(mesh))
    for dptr in keep:
        capi.lib.fl_free(0, dptr)

    def velocity(b, t, Xf):
        if b == 0:
            return np.stack([4.0 * Xf[:, 1] * (1.0 - Xf[:, 1]), np.zeros(len(Xf)), np.zeros(len(Xf))])
        return np.zeros((3, len(Xf)))

    ibm = dict(kind=0, X=X0, dV=dV, Ut=None)
    so = fo.StepOracle(g, dt, rho, mu, velocity, krylov_rtol=1e-4, outer_rtol=1e-9, pressure=lambda b, t, Xf: np.zeros(len(Xf)), ibm=ibm)
    vo, Vo, po = np.zeros(3 * g.ncell), [np.zeros(nf) for nf in g.nface], np.zeros(g.ncell)
    for k in range(nsteps):
        ibm["X"], ibm["Ut"] = motion.markers(X0, (k + 1) * dt)
        vo, Vo, po, _ = so.step_once(vo, Vo, po)
    rel = lambda a, b: float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
    r = dict(v=rel(vg, vo), p=rel(pg, po), V=[rel(Vg[d], Vo[d]) for d in range(3)])
    print("moving sphere, GPU against the oracle's step:", r)
    assert np.abs(vo).max() > 0.5
    assert r["v"] <= 1e-6 and r["p"] <= 1e-5, r
    assert max(r["V"][:2]) <= 1e-6, r
