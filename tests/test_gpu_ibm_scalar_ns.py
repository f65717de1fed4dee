"""-m gpu: a scalar held at a value on an immersed sphere through the C host mirror (NSSetScalarImmersedBoundary, include/fluca_host.h).

A channel of 16 x 12 x 8 cells (h = 1/8: parabolic inlet, pressure outlet, walls in y, periodic span) with a sphere of radius 2 h, one scalar (0 at
the inlet).  With the forcing off NSStep keeps every bit of a run that never heard of it; with it on, phi after NSStep is, bit for bit, phi of an
NSStep without it followed by one fl_ibm_scalar_force on NSGetScalarArray's array, and the rate is (1 / dt) fl_ibm_scalar_rate of that Q -- with ONE
substep, explicit and with -ns_scalar_implicit_theta 1.  (Two substeps cannot be had from two half steps of a run without the forcing: the flow
would take two steps as well and hand the scalar other face velocities; two substeps are run for what can be said without that: no error, a finite
positive rate, another phi than one substep gives.)  Two ranks along x with owner-rank markers and the sphere moving across the rank face; the
error returns."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

from tests import ibm_regimes as R_
from tests import inproc
from tests.test_gpu_ibm_owner import _extra_options

pytestmark = pytest.mark.gpu

N, BOX, DT = (16, 12, 8), (2.0, 1.5, 1.0), 5e-3
H_ = BOX[0] / N[0]
VALUE = 1.0
NPASS = 2


def _sphere():
    X = R_.fib_sphere(50, (0.5 * BOX[0] - 0.4 * H_, 0.5 * BOX[1], 0.5 * BOX[2]), 2.0 * H_)
    return [np.ascontiguousarray(a) for a in X], np.full(50, H_ ** 3)


def _run(R, mode, nsteps=1, substeps=1, moving=False, manual=False):
    """mode: "never" (the feature is not touched), "off" (switched on, then off again before the first step), "on".  manual: after the steps one
    fl_ibm_scalar_force + fl_ibm_scalar_rate by hand on NSGetScalarArray's array.  -> this rank's v, p, phi and what the calls returned"""
    from fluca_amd import capi, hostapi as H
    P = C.c_void_p
    Lx, Ly, Lz = BOX
    rank, size = (0, 1) if R is None else (R.rank, R.size)
    rk = (2, 1, 1) if size > 1 else (1, 1, 1)
    mesh = P()
    assert H.lib.MeshCartCreate3d(0, 0, 1, N[0], N[1], N[2], rk[0], rk[1], rk[2], None, None, None, C.byref(mesh)) == 0
    assert H.lib.MeshSetRank(mesh, rank, size) == 0 and H.lib.MeshSetUp(mesh) == 0
    assert H.lib.MeshCartSetUniformCoordinates(mesh, 0., Lx, 0., Ly, 0., Lz) == 0
    ns = P()
    assert H.lib.NSCreate(C.byref(ns)) == 0 and H.lib.NSSetType(ns, b"cnlinear") == 0 and H.lib.NSSetMesh(ns, mesh) == 0
    assert H.lib.NSSetDensity(ns, 1.0) == 0 and H.lib.NSSetViscosity(ns, 0.05) == 0

    @H.BCFunc
    def inlet(dim, t, x, val, ctx):
        val[0], val[1], val[2] = 4.0 * x[1] * (Ly - x[1]) / Ly ** 2, 0.0, 0.0
        return 0

    @H.BCFunc
    def wall(dim, t, x, val, ctx):
        val[0] = val[1] = val[2] = 0.0
        return 0

    @H.BCFunc
    def outlet(dim, t, x, val, ctx):
        val[0] = 0.0
        return 0

    bcs = [H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=inlet), H.NSBoundaryCondition(type=H.NS_BC_PRESSURE_OUTLET, pressure=outlet),
           H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=wall), H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=wall),
           H.NSBoundaryCondition(type=H.NS_BC_PERIODIC), H.NSBoundaryCondition(type=H.NS_BC_PERIODIC)]
    for b in range(6):
        assert H.lib.NSSetBoundaryCondition(ns, b, bcs[b]) == 0
    argc, av = H.argv("-ns_time_step_size", DT, "-ns_ksp_rtol", 1e-10, "-ns_abf_schur_ksp_type", "bcgs", "-ns_abf_schur_ksp_rtol", 1e-12,
                      "-ns_abf_momentum_ksp_rtol", 1e-12, "-ns_scalar_ibm_passes", NPASS)
    assert H.lib.NSSetFromOptions(ns, argc, av) == 0 and H.lib.NSSetUp(ns) == 0
    hp = P()
    assert H.lib.NSGetPoisson(ns, C.byref(hp)) == 0
    if R is not None:
        R.attach(hp)
    X, dV = _sphere()
    L = X[0].size
    keep = []
    for a in X + [dV]:
        dptr = P()
        capi.check(capi.lib.fl_malloc(0, a.size * 8, C.byref(dptr)))
        capi.check(capi.lib.fl_memcpy_h2d(0, dptr, np.ascontiguousarray(a).ctypes.data_as(C.c_void_p), a.size * 8))
        keep.append(dptr)
    res = {}
    sid = C.c_int(-1)
    assert H.lib.NSAddScalar(ns, b"heat", 0.02, None, C.byref(sid)) == 0
    assert H.lib.NSSetScalarSubsteps(ns, sid.value, substeps) == 0
    val = (C.c_double * 1)(VALUE)
    rate = (C.c_double * 1)(-7.0)
    if mode != "never":
        res["early_rc"] = H.lib.NSSetScalarImmersedBoundary(ns, sid.value, -1, val)                  # before NSSetImmersedBoundary
    assert H.lib.NSSetImmersedBoundary(ns, 0, L, keep[0], keep[1], keep[2], keep[3], None) == 0
    centre0 = (C.c_double * 3)(0.5 * Lx - 0.4 * H_, 0.5 * Ly, 0.5 * Lz)

    @H.BodyMotionFunc
    def fn(t, centre, rotvec, velocity, omega, ctx):
        speed = 0.4 * H_ / DT                                                                        # 0.4 h per step along x, through the rank face
        centre[0], centre[1], centre[2] = centre0[0] + speed * t, centre0[1], centre0[2]
        velocity[0], velocity[1], velocity[2] = speed, 0.0, 0.0
        for a in range(3):
            rotvec[a] = omega[a] = 0.0
        return 0

    if moving:
        assert H.lib.NSSetImmersedBoundaryMotion(ns, centre0, fn, None) == 0
    if mode != "never":
        res["range_rc"] = [H.lib.NSSetScalarImmersedBoundary(ns, sid.value, 17, val), H.lib.NSSetScalarImmersedBoundary(ns, sid.value, -2, val),
                           H.lib.NSSetScalarImmersedBoundary(ns, 5, 1, val)]
        assert H.lib.NSSetScalarImmersedBoundary(ns, sid.value, -1, val) == 0                        # the option's count
        val[0] = np.nan                                                                              # the values were copied
        res["before_step_rc"] = H.lib.NSGetScalarImmersedBoundaryRate(ns, sid.value, rate)
        if mode == "off":
            assert H.lib.NSSetScalarImmersedBoundary(ns, sid.value, 0, None) == 0
    with tempfile.TemporaryDirectory() as tmp:
        vw = P()
        assert H.lib.FlucaViewerASCIIOpen(os.path.join(tmp, "view.txt").encode(), C.byref(vw)) == 0 and H.lib.NSView(ns, vw) == 0
        assert H.lib.FlucaViewerDestroy(C.byref(vw)) == 0
        res["view"] = open(os.path.join(tmp, "view.txt")).read()
    res["step_rc"] = [H.lib.NSStep(ns) for _ in range(nsteps)]
    res["rate_rc"] = H.lib.NSGetScalarImmersedBoundaryRate(ns, sid.value, rate) if mode != "never" else None
    res["rate"] = rate[0]
    sz = (C.c_int64 * 4)()
    assert H.lib.NSGetLocalSizes(ns, sz) == 0
    cc = [C.c_int64() for _ in range(6)]
    assert H.lib.MeshCartGetCorners(mesh, *[C.byref(q) for q in cc]) == 0
    v, p, Vp, phi = P(), P(), (C.c_void_p * 3)(), P()
    assert H.lib.NSGetSolutionArrays(ns, C.byref(v), Vp, C.byref(p)) == 0
    assert H.lib.NSGetScalarArray(ns, sid.value, C.byref(phi)) == 0

    def get(ptr, m):
        out = np.empty(m)
        capi.check(capi.lib.fl_poisson_synchronize(hp))
        capi.check(capi.lib.fl_memcpy_d2h(0, out.ctypes.data_as(C.c_void_p), ptr, m * 8))
        return out

    if manual:
        ibm, Q = P(), P()
        assert H.lib.NSGetImmersedBoundary(ns, C.byref(ibm)) == 0
        capi.check(capi.lib.fl_malloc(0, L * 8, C.byref(Q)))
        one = (C.c_double * 1)(VALUE)
        capi.check(capi.lib.fl_ibm_scalar_force(ibm, NPASS, None, None, 1, one, keep[3], phi, Q), "fl_ibm_scalar_force")
        r = (C.c_double * 1)()
        capi.check(capi.lib.fl_ibm_scalar_rate(ibm, Q, keep[3], None, 1, r), "fl_ibm_scalar_rate")
        res["manual_rate"] = (1.0 / DT) * r[0]
        capi.lib.fl_free(0, Q)
    res.update(lo=[q.value for q in cc[:3]], ln=[q.value for q in cc[3:]], v=get(v, 3 * sz[0]), p=get(p, sz[0]), phi=get(phi, sz[0]))
    if mode == "on":
        # a new marker set switches the forcing off
        assert H.lib.NSSetImmersedBoundary(ns, 0, L, keep[0], keep[1], keep[2], keep[3], None) == 0
        res["after_reset_rc"] = H.lib.NSGetScalarImmersedBoundaryRate(ns, sid.value, rate)
    H.lib.NSDestroy(C.byref(ns))
    H.lib.MeshDestroy(C.byref(mesh))
    for dptr in keep:
        capi.lib.fl_free(0, dptr)
    return res


@functools.lru_cache(maxsize=None)
def _one(mode, theta=0.0, **kw):
    opts = ("-ns_scalar_implicit_theta", theta) if theta else ()
    with _extra_options(*opts):
        return inproc.run_threads(1, lambda R: _run(None, mode, **kw))[0]


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def test_with_the_forcing_off_nsstep_keeps_every_bit():
    a, b = _one("never", nsteps=2), _one("off", nsteps=2)
    assert a["step_rc"] == b["step_rc"] == [0, 0]
    assert same_bits(a["v"], b["v"]) and same_bits(a["p"], b["p"]) and same_bits(a["phi"], b["phi"])
    assert b["rate_rc"] == 73                                                           # E_ARG_WRONGSTATE: the forcing is off
    # NSView: the pass count and the values only while the forcing is on
    on = _one("on")
    assert a["view"] == b["view"] and "on the immersed boundary" not in a["view"]
    assert on["view"].startswith(a["view"].rstrip("\n")) and "Scalar heat on the immersed boundary: 2 passes, value 1\n" in on["view"]


@pytest.mark.parametrize("theta", [0.0, 1.0], ids=["explicit", "backward_euler"])
def test_one_substep_is_the_step_without_it_and_one_call_by_hand(theta):
    on, by_hand = _one("on", theta=theta), _one("never", theta=theta, manual=True)
    assert on["step_rc"] == [0] and on["rate_rc"] == 0
    assert same_bits(on["v"], by_hand["v"]) and same_bits(on["p"], by_hand["p"])         # the scalar is passive: the flow does not see the forcing
    assert same_bits(on["phi"], by_hand["phi"])
    assert not np.array_equal(on["phi"], _one("never", theta=theta)["phi"])
    assert same_bits([on["rate"]], [by_hand["manual_rate"]]) and on["rate"] > 0.0         # a body at 1 in a fluid at 0 gives


def test_two_substeps_add_their_rates():
    on = _one("on", substeps=2)
    assert on["step_rc"] == [0] and on["rate_rc"] == 0 and np.isfinite(on["rate"]) and on["rate"] > 0.0
    assert np.all(np.isfinite(on["phi"])) and not np.array_equal(on["phi"], _one("on")["phi"])


def test_the_returns_of_the_setter_and_the_getter():
    on = _one("on")
    assert on["early_rc"] == 73                                                          # E_ARG_WRONGSTATE: no immersed boundary yet
    assert on["range_rc"] == [63, 63, 63]                                                # E_ARG_OUTOFRANGE: npass 17, -2; scalar id 5
    assert on["before_step_rc"] == 73 and on["after_reset_rc"] == 73


def test_two_ranks_with_owner_markers_and_a_sphere_that_crosses_the_rank_face():
    """three steps of 0.4 h along x, the centre starting 0.4 h before the face between the two ranks: no error, the rate the same on both ranks, phi
    within 1e-7 of the one-rank run relative to max |phi| -- the bound tests/test_gpu_ibm_motion.py holds the several-rank pressure to (the two runs
    differ by their flow solves, not by rounding)"""
    with _extra_options("-ns_ibm_marker_distribution", "owner"):
        parts = inproc.run_threads(2, _run, "on", 3, 1, True)
    one = inproc.run_threads(1, lambda R: _run(None, "on", 3, 1, True))[0]
    assert all(r["step_rc"] == [0, 0, 0] and r["rate_rc"] == 0 for r in parts) and one["step_rc"] == [0, 0, 0]
    assert same_bits([parts[0]["rate"]], [parts[1]["rate"]]) and np.isfinite(parts[0]["rate"])
    phi = np.full((N[2], N[1], N[0]), np.nan)
    for r in parts:
        lo, ln = r["lo"], r["ln"]
        phi[lo[2]:lo[2] + ln[2], lo[1]:lo[1] + ln[1], lo[0]:lo[0] + ln[0]] = r["phi"].reshape(ln[2], ln[1], ln[0])
    err = float(np.abs(phi.ravel() - one["phi"]).max())
    print(f"rate {parts[0]['rate']:.6e} (one rank {one['rate']:.6e}), max |phi - one rank| {err:.2e}, max |phi| {np.abs(one['phi']).max():.3f}")
    assert err <= 1e-7 * float(np.abs(one["phi"]).max())
    assert abs(parts[0]["rate"] - one["rate"]) <= 1e-7 * abs(one["rate"])
