"""CPU-only: the Boussinesq coupling as far as it goes without a GPU -- the argument checks of fl_momentum_add_buoyancy and fl_scalar_boundary_flux
(made before a handle is touched), the mirror calls before set-up, -ns_gravity, and the references of tests/buoyancy_reference.py pinned to
mathematics: the diffusive wall flux of a linear field, and the exact budget  sum_c R(phi)(c) vol(c) = sum_d (flux_lo - flux_hi) + sum_c q vol.
(The mirror calls with a bad id need a set-up NS, hence a GPU: tests/test_gpu_buoyancy_ns.py.)"""
import ctypes as C

import numpy as np
import pytest

from tests import buoyancy_reference as br
from tests import scalar_cases as sc
from tests import scalar_reference as sr

P = C.c_void_p
U = sr.U


@pytest.fixture(scope="module")
def H():
    from fluca_amd import build
    build.build()
    from fluca_amd import hostapi
    return hostapi


def test_buoyancy_argument_checks(H):
    """every check is made before the handle is used: a stand-in for it (64 zero bytes, never a handle) is enough where the handle must not be NULL"""
    lib = H.capi.lib
    fake = C.create_string_buffer(64)
    m = C.cast(fake, C.c_void_p)
    buf = (C.c_double * 8)()
    ptr = C.cast(buf, C.c_void_p)
    one = (C.c_void_p * 1)(ptr)
    d = lambda *v: (C.c_double * len(v))(*v)
    a1, r1 = d(0.0, -1.0, 0.0), d(0.5)
    f = lib.fl_momentum_add_buoyancy
    assert f(None, 1, one, a1, r1, 0.1, ptr) == -85
    assert f(m, 1, None, a1, r1, 0.1, ptr) == -85 and f(m, 1, one, None, r1, 0.1, ptr) == -85
    assert f(m, 1, one, a1, None, 0.1, ptr) == -85 and f(m, 1, one, a1, r1, 0.1, None) == -85
    assert f(m, 1, (C.c_void_p * 1)(None), a1, r1, 0.1, ptr) == -85
    nine = (C.c_void_p * 9)(*([ptr] * 9))
    assert f(m, 0, one, a1, r1, 0.1, ptr) == -63 and f(m, 9, nine, d(*([1.0] * 27)), d(*([0.0] * 9)), 0.1, ptr) == -63
    assert f(m, -1, one, a1, r1, 0.1, ptr) == -63
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert f(m, 1, one, d(0.0, bad, 0.0), r1, 0.1, ptr) == -63
        assert f(m, 1, one, a1, d(bad), 0.1, ptr) == -63
        assert f(m, 1, one, a1, r1, bad, ptr) == -63
    # all coefficients zero: success, and nothing is launched (there is no GPU here, and the stand-in is no handle)
    assert f(m, 1, one, d(0.0, 0.0, 0.0), r1, 0.1, ptr) == 0
    assert f(m, 2, (C.c_void_p * 2)(ptr, ptr), d(0.0, -0.0, 0.0, 0.0, 0.0, 0.0), d(0.5, 1.0), 0.1, ptr) == 0
    out = (C.c_double * 12)()
    g = lib.fl_scalar_boundary_flux
    assert g(None, ptr, out) == -85 and g(m, None, out) == -85 and g(m, ptr, None) == -85


def new_ns(H):
    ns = P()
    assert H.lib.NSCreate(C.byref(ns)) == 0 and H.lib.NSSetType(ns, b"cnlinear") == 0
    return ns


def test_mirror_calls_before_setup(H):
    ns = new_ns(H)
    g = (C.c_double * 3)(9.0, 9.0, 9.0)
    assert H.lib.NSGetGravity(None, g) == H.ERR_ARG_NULL and H.lib.NSGetGravity(ns, None) == H.ERR_ARG_NULL
    assert H.lib.NSGetGravity(ns, g) == 0 and tuple(g) == (0.0, 0.0, 0.0)                   # the default
    assert H.lib.NSSetGravity(None, g) == H.ERR_ARG_NULL and H.lib.NSSetGravity(ns, None) == H.ERR_ARG_NULL
    assert H.lib.NSSetGravity(ns, (C.c_double * 3)(0.0, -9.81, 0.25)) == 0                   # before set-up: like the density
    assert H.lib.NSGetGravity(ns, g) == 0 and tuple(g) == (0.0, -9.81, 0.25)
    for bad in (float("nan"), float("inf")):
        assert H.lib.NSSetGravity(ns, (C.c_double * 3)(0.0, bad, 0.0)) == H.ERR_ARG_OUTOFRANGE
    assert H.lib.NSGetGravity(ns, g) == 0 and tuple(g) == (0.0, -9.81, 0.25)                 # a rejected value changes nothing
    assert H.lib.NSSetScalarBuoyancy(None, 0, 1.0, 0.0) == H.ERR_ARG_NULL
    assert H.lib.NSSetScalarBuoyancy(ns, 0, 1.0, 0.0) == H.ERR_ARG_WRONGSTATE
    out = (C.c_double * 12)()
    assert H.lib.NSGetScalarBoundaryFlux(None, 0, out) == H.ERR_ARG_NULL and H.lib.NSGetScalarBoundaryFlux(ns, 0, None) == H.ERR_ARG_NULL
    assert H.lib.NSGetScalarBoundaryFlux(ns, 0, out) == H.ERR_ARG_WRONGSTATE
    H.lib.NSDestroy(C.byref(ns))


def test_gravity_option(H):
    ns = new_ns(H)
    g = (C.c_double * 3)()
    argc, av = H.argv("-ns_gravity", "0.5,-9.81,1e-3")
    assert H.lib.NSSetFromOptions(ns, argc, av) == 0
    assert H.lib.NSGetGravity(ns, g) == 0 and tuple(g) == (0.5, -9.81, 1e-3)
    argc, av = H.argv("-ns_gravity", "-1,0,0")
    assert H.lib.NSSetFromOptions(ns, argc, av) == 0 and H.lib.NSGetGravity(ns, g) == 0 and tuple(g) == (-1.0, 0.0, 0.0)
    for bad in ("0,-9.81", "1", "1,2,3,4", "1,2,", "a,b,c", "1,2,x", "1 2 3"):
        argc, av = H.argv("-ns_gravity", bad)
        assert H.lib.NSSetFromOptions(ns, argc, av) == H.ERR_ARG_WRONG, bad
    argc, av = H.argv("-ns_gravity", "0,nan,0")
    assert H.lib.NSSetFromOptions(ns, argc, av) == H.ERR_ARG_OUTOFRANGE
    assert H.lib.NSGetGravity(ns, g) == 0 and tuple(g) == (-1.0, 0.0, 0.0)
    H.lib.NSDestroy(C.byref(ns))


# ---- the references, pinned to mathematics

N = (7, 5, 6)
GAMMA = 0.0125


def linear_problem(d, kinds_of_axis, slope, offset):
    """stretched grid; phi = offset + slope x_d; the ends of axis d Dirichlet with the line's values or Neumann with its slope; Neumann 0 elsewhere"""
    xf = sc.faces(N, False)
    kinds, vals = [sr.NEUMANN] * 6, [0.0] * 6
    for side in (0, 1):
        kinds[2 * d + side] = kinds_of_axis[side]
        vals[2 * d + side] = offset + slope * xf[d][-1 if side else 0] if kinds_of_axis[side] == sr.DIRICHLET else slope
    Pr = sr.Problem(xf, kinds, vals, gamma=GAMMA)
    shape = [1, 1, 1]
    shape[2 - d] = N[d]
    phi = np.broadcast_to((offset + slope * Pr.xc[d]).reshape(shape), (N[2], N[1], N[0])).copy()
    return Pr, phi


@pytest.mark.parametrize("d", [0, 1, 2])
def test_diffusive_wall_flux_of_a_linear_field(d):
    slope, offset = -1.75, 0.6
    rng = np.random.default_rng(5)
    # Dirichlet at both ends: -Gamma slope area, to 8 U sum |coefficient| |value| of the two-point row (1 / dist) (phi_0 - phi_b)
    Pr, phi = linear_problem(d, (sr.DIRICHLET, sr.DIRICHLET), slope, offset)
    V = [rng.uniform(-1.0, 1.0, s) for s in Pr.shapes()[1]]
    # (the field and the boundary values are the line rounded to binary64: those roundings, a few U of |value| each, are what the bound is for;
    # the flux itself is evaluated in long double)
    flux, _ = br.wall_fluxes(Pr, phi, V, np.longdouble)
    A = br.areas(Pr, d, np.float64)
    for side in (0, 1):
        near, dist = (Pr.xc[d][-1], Pr.xf[d][-1] - Pr.xc[d][-1]) if side else (Pr.xc[d][0], Pr.xc[d][0] - Pr.xf[d][0])
        absrow = GAMMA * A.sum() * (abs(offset + slope * near) + abs(Pr.val[2 * d + side])) / dist
        want = -GAMMA * slope * A.sum()
        err = abs(float(flux[2 * d + side, 1]) - want)
        print(f"axis {d} side {side}: |flux - (-Gamma slope area)| = {err / (U * absrow):.2f} U sum |coefficient| |value|")
        assert err <= 8 * U * absrow, (side, float(flux[2 * d + side, 1]), want)
        assert abs(want) > 1e-3
    # the other axes: Neumann 0, an exact zero (either sign)
    for b in range(6):
        if b // 2 != d:
            assert flux[b, 1] == 0.0
    # Neumann: -Gamma value area exactly, face by face
    Pr, phi = linear_problem(d, (sr.NEUMANN, sr.NEUMANN), slope, offset)
    flux, bound = br.wall_fluxes(Pr, phi, V, np.float64)
    for side in (0, 1):
        assert flux[2 * d + side, 1] == (-np.float64(GAMMA) * np.float64(slope) * A).sum()
    # ... and its convective part carries phi_near -/+ dist slope = the line's value on the face
    t = sr.axis_terms(Pr, phi, V[d], d, np.float64)
    for side, f in ((0, 0), (1, N[d])):
        assert np.abs(t["F"][f] - (offset + slope * Pr.xf[d][f])).max() <= 4 * U * (abs(offset) + abs(slope))


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "stretched"])
@pytest.mark.parametrize("bcname", list(sc.BC_SETS))
@pytest.mark.parametrize("limiter", ["superbee", "vanleer"])
def test_exact_budget_of_the_reference(bcname, uniform, limiter):
    """sum_c R(phi)(c) vol(c) telescopes to the boundary fluxes in long double; the bound is the one tests/test_gpu_scalar_flux.py uses on the GPU's
    numbers (U sum_c E(c) vol(c) + the flux bounds), and the long-double reference alone must stay inside it with margin (1 / 8 of it: its own
    unit roundoff is 2^-11 U)."""
    Pr = sc.problem(N, uniform, bcname)
    V = sc.velocity(N, bcname)                     # both signs on the boundary faces: inflow and outflow
    q = sc.source(N)
    phi = sc.phi_field(N, "random")
    keep = Pr.gamma
    try:
        for gamma in (0.0, GAMMA):
            Pr.gamma = gamma
            R, E, _ = sr.rhs(Pr, phi, V, q, np.longdouble, bounds=True, limiter=limiter)
            vol = sr.volumes(Pr, np.longdouble)
            flux, fb = br.wall_fluxes(Pr, phi, V, np.longdouble, limiter=limiter)
            lhs = (R * vol).sum()
            rhs = br.budget(flux) + (np.asarray(q, dtype=np.longdouble) * vol).sum()
            bound = float(U * (E * vol).sum()) + float(fb.sum())
            print(f"budget {bcname} {limiter} gamma={gamma}: |lhs - rhs| / bound = {float(abs(lhs - rhs)) / bound:.3e}")
            assert float(abs(lhs - rhs)) <= bound / 8, (float(lhs), float(rhs), bound)
            assert float(abs(lhs)) > 1e-3
            for d in range(3):
                if Pr.periodic(d):
                    assert (flux[2 * d:2 * d + 2] == 0).all()
    finally:
        Pr.gamma = keep
