"""Passive scalars in the host mirror's NSStep (include/fluca_host.h: NSAddScalar ...): the periodic Taylor-Green set-up of the mirror tests at
16^3, four steps.  The scalar equals tests/scalar_reference.py driven by the face velocities read back after each step, to the derived bound of
one step (test_gpu_scalar_step.py); the flow keeps its bits."""
import ctypes as C

import numpy as np
import pytest

from tests import scalar_reference as sr

pytestmark = pytest.mark.gpu
P = C.c_void_p
N, NSTEPS = 16, 4


@pytest.fixture(scope="module")
def H():
    from fluca_amd import build
    build.build()
    from fluca_amd import hostapi
    return hostapi


def phi_start(seed):
    rng = np.random.default_rng(seed)
    k, j, i = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    return np.where((i + 2 * j + k) % 16 < 7, 1.0, 0.0) + 0.1 * rng.uniform(-1.0, 1.0, (N, N, N))


def run(H, scalars=(), opts=()):
    """four NSStep calls; scalars: (gamma, limiter name or None, substeps, start field) each.  -> per step (v, [Vx, Vy, Vz], p, [phi ...]), dt, cfl"""
    L = 2 * np.pi
    rho, mu = 1.0, 0.1
    mesh, ns = P(), P()
    assert H.lib.MeshCartCreate3d(1, 1, 1, N, N, N, -1, -1, -1, None, None, None, C.byref(mesh)) == 0
    assert H.lib.MeshSetUp(mesh) == 0 and H.lib.MeshCartSetUniformCoordinates(mesh, 0., L, 0., L, 0., L) == 0
    assert H.lib.NSCreate(C.byref(ns)) == 0 and H.lib.NSSetType(ns, b"cnlinear") == 0 and H.lib.NSSetMesh(ns, mesh) == 0
    assert H.lib.NSSetDensity(ns, rho) == 0 and H.lib.NSSetViscosity(ns, mu) == 0
    for b in range(6):
        assert H.lib.NSSetBoundaryCondition(ns, b, H.NSBoundaryCondition(type=H.NS_BC_PERIODIC)) == 0
    dt = 0.1
    argc, av = H.argv("-ns_time_step_size", dt, "-ns_ksp_type", "richardson", "-ns_ksp_rtol", 1e-8, "-ns_abf_schur_ksp_rtol", 1e-10,
                      "-ns_abf_momentum_ksp_rtol", 1e-10, *opts)
    assert H.lib.NSSetFromOptions(ns, argc, av) == 0 and H.lib.NSSetUp(ns) == 0
    v, p, V = P(), P(), (C.c_void_p * 3)()
    assert H.lib.NSGetSolutionArrays(ns, C.byref(v), V, C.byref(p)) == 0
    h = L / N
    xc, xf = (np.arange(N) + 0.5) * h, np.arange(N) * h
    Z = np.ones((N, 1, 1))
    ex = lambda xs, ys: (Z * (np.sin(xs)[None, None, :] * np.cos(ys)[None, :, None]), Z * (-np.cos(xs)[None, None, :] * np.sin(ys)[None, :, None]))
    put = lambda ptr, a: H.capi.check(H.capi.lib.fl_memcpy_h2d(0, ptr, np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.c_void_p), a.size * 8))

    def get(ptr, shape):
        out = np.empty(shape)
        H.capi.check(H.capi.lib.fl_memcpy_d2h(0, out.ctypes.data_as(C.c_void_p), ptr, out.size * 8))
        return out
    u0, w0 = ex(xc, xc)
    put(v, np.stack([u0, w0, 0.2 * np.ones_like(u0)]))
    put(C.c_void_p(V[0]), ex(xf, xc)[0])
    put(C.c_void_p(V[1]), ex(xc, xf)[1])
    put(C.c_void_p(V[2]), 0.2 * np.ones((N, N, N)))
    X, Y = np.meshgrid(xc, xc, indexing="xy")
    put(p, Z * (rho / 4 * (np.cos(2 * X) + np.cos(2 * Y)))[None, :, :])
    ids, arrays = [], []
    for gamma, limiter, substeps, start in scalars:
        sid, ptr = C.c_int(-1), P()
        assert H.lib.NSAddScalar(ns, b"dye%d" % len(ids), gamma, None if limiter is None else limiter.encode(), C.byref(sid)) == 0 and sid.value == len(ids)
        assert H.lib.NSSetScalarSubsteps(ns, sid.value, substeps) == 0
        assert H.lib.NSGetScalarArray(ns, sid.value, C.byref(ptr)) == 0 and ptr.value
        assert np.all(get(ptr, (N, N, N)) == 0.0)                       # a new scalar starts at 0
        put(ptr, start)
        ids.append(sid.value)
        arrays.append(ptr)
    if scalars:    # the errors that need a set-up NS
        assert H.lib.NSSetScalarSubsteps(ns, len(ids), 1) == H.ERR_ARG_OUTOFRANGE and H.lib.NSSetScalarSubsteps(ns, 0, 0) == H.ERR_ARG_OUTOFRANGE
        assert H.lib.NSSetScalarBoundaryCondition(ns, 0, 6, 0, 0.0) == H.ERR_ARG_OUTOFRANGE
        assert H.lib.NSSetScalarBoundaryCondition(ns, 0, 0, 3, 0.0) == H.ERR_ARG_OUTOFRANGE
        assert H.lib.NSAddScalar(ns, b"x", -1.0, None, C.byref(C.c_int())) == H.ERR_ARG_OUTOFRANGE
        assert H.lib.NSAddScalar(ns, b"x", 0.0, b"nolimiter", C.byref(C.c_int())) == H.ERR_ARG_UNKNOWN_TYPE
    steps, cfls = [], []
    for _ in range(NSTEPS):
        assert H.lib.NSStep(ns) == 0
        steps.append((get(v, (3, N, N, N)), [get(C.c_void_p(V[d]), (N, N, N)) for d in range(3)], get(p, (N, N, N)), [get(a, (N, N, N)) for a in arrays]))
        out = (C.c_double * 2)()
        for sid in ids:
            assert H.lib.NSGetScalarCFL(ns, sid, out) == 0
            cfls.append((out[0], out[1]))
    H.lib.NSDestroy(C.byref(ns))
    H.lib.MeshDestroy(C.byref(mesh))
    return steps, dt, cfls


@pytest.fixture(scope="module")
def runs(H):
    starts = [phi_start(1), phi_start(2)]
    plain = run(H)
    # scalar 0: limiter and stages from the options; scalar 1: its own limiter, two substeps
    with_scalars = run(H, [(0.01, None, 1, starts[0]), (0.0, "superbee", 2, starts[1])], ("-ns_scalar_limiter", "vanleer", "-ns_scalar_stages", 3))
    return plain, with_scalars, starts


def test_flow_keeps_its_bits(runs):
    (plain, _, _), (scal, _, _), _ = runs
    for (v0, V0, p0, _), (v1, V1, p1, _) in zip(plain, scal):
        assert np.array_equal(v0, v1) and np.array_equal(p0, p1) and all(np.array_equal(a, b) for a, b in zip(V0, V1))
    assert np.abs(plain[-1][0] - plain[0][0]).max() > 1e-3          # (and it moves)


def problem(gamma, limiter):
    xf = [np.arange(N + 1) * (2 * np.pi / N)] * 3
    xc = [(np.arange(N) + 0.5) * (2 * np.pi / N)] * 3
    return sr.Problem(xf, (sr.PERIODIC,) * 6, gamma=gamma, limiter=limiter, xc=xc)


def test_scalar_follows_the_reference_with_the_new_velocity(runs):
    """-ns_scalar_limiter vanleer and -ns_scalar_stages 3 reach the handle: the reference with them is met step by step, the reference with the
    defaults (superbee, 5) is not"""
    _, (scal, dt, cfls), starts = runs
    Pr = problem(0.01, "vanleer")
    before = starts[0]
    for it, (_, V, _, phis) in enumerate(scal):
        want, B = sr.step(Pr, before, V, dt, 3, None, np.longdouble, bounds=True)
        err = np.abs(phis[0].astype(np.longdouble) - want).astype(np.float64)
        assert (err <= np.asarray(B, dtype=np.float64) * (1 + 2.0 ** -10)).all(), (it, float(err.max()), float(B.max()))
        other = sr.step(problem(0.01, "superbee"), before, V, dt, 5)
        assert np.abs(phis[0] - other).max() > 1e-4
        adv, dif = sr.cfl(Pr, V, dt)
        assert cfls[2 * it] == pytest.approx((adv, dif), rel=1e-12)
        before = phis[0]
    assert np.abs(scal[-1][3][0] - starts[0]).max() > 0.05


def test_two_substeps_are_two_half_steps(runs):
    _, (scal, dt, cfls), starts = runs
    Pr = problem(0.0, "superbee")
    before = starts[1]
    for it, (_, V, _, phis) in enumerate(scal):
        half, B1 = sr.step(Pr, before, V, dt / 2, 3, None, np.longdouble, bounds=True)
        want, B2 = sr.step(Pr, half, V, dt / 2, 3, None, np.longdouble, bounds=True, eps_in=float(B1.max()))
        err = np.abs(phis[1].astype(np.longdouble) - want).astype(np.float64)
        assert (err <= np.asarray(B2, dtype=np.float64) * (1 + 2.0 ** -10)).all(), (it, float(err.max()), float(B2.max()))
        one = sr.step(Pr, before, V, dt, 3)
        assert np.abs(phis[1] - one).max() > 1e-6                       # (one whole step is something else)
        assert cfls[2 * it + 1][0] == pytest.approx(sr.cfl(Pr, V, dt / 2)[0], rel=1e-12) and cfls[2 * it + 1][1] == 0.0
        before = phis[1]
