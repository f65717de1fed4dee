"""-m gpu: the implicit scalar diffusion of include/fluca_hip_implicit.h -- fl_scalar_diffusion_apply / _solve and fl_scalar_step_imex -- against
tests/scalar_implicit_reference.py (ir).

What is asserted, and where each bound comes from:

  apply     every cell against long double within U times ir.apply_bound: the derived bound E of D (sr.rhs with V = 0, Gamma = 1) times c, one
            rounding on |c D| for the product and one on |phi| + |c D| for the difference (scalar_cases.rhs_slack's shares on top)
  two steps maxit = 2 against the long-double recurrence, cell by cell, within two_step_bound (derived in its docstring)
  solve     |x - x_exact| <= B_k |x_0 - x_exact| + floor in the norm sum vol diag e^2, x_exact by a sparse direct solve refined in long double (the
            grid in the launch plan of 512^3: a manufactured solution, b = H_c(x_exact) in long double -- a direct solve of 270 000 unknowns is not
            a matter of seconds); floor = FLOOR_MARGIN times the distance of ir's binary64 recurrence from its long-double twin on the same inputs;
            info = ir's count, bound and interval
  imex      against ir.imex_step (exact solve): the explicit step's derived bound (sr.step, bounds=True) carried through the solve -- |A^-1| <= 1 in
            the maximum norm, so a field error of at most eps is at most eps sqrt(sum w) in the weighted norm -- plus B_k |e_0| plus the floor

Every check takes the results from a `backend` (here: the GPU through fluca_amd.scalar.Scalar), so that the bounds can be tried on ir's own
binary64 recurrence where there is no device.

Grids: (7, 5, 3); (6, 2, 1) with the short axes periodic (a two-cell periodic axis, a one-cell axis that contributes nothing); (65, 3, 2) and (130, 4, 3)
(an x line crosses the 64-lane segment with a ragged tail); and regime_grid(): the smallest grid that takes k_scalar_cheb's launch plan of 512^3 and
sends some waves through their loop a second time, found through fldbg_scalar_cheb_plan."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import scalar_cases as sc
from tests import scalar_implicit_reference as ir
from tests import scalar_reference as sr

pytestmark = pytest.mark.gpu

U = sr.U
FLOOR_MARGIN = 8.0          # the other summation order of the three axes and FMA contraction
SMALL = (7, 5, 3)
SHORT = (6, 2, 1)
RAGGED = [(65, 3, 2), (130, 4, 3)]
BOTH = pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "stretched"])
BCS = pytest.mark.parametrize("bcname", list(sc.BC_SETS))
ids_n = lambda n: "x".join(map(str, n))


# ------------------------------------------------------------------------------------------------------------------ the backend

def _dev(a):
    from tests.gpu_common import dev
    return dev(np.ascontiguousarray(a, dtype=np.float64).reshape(-1))


def _host(t):
    from tests.gpu_common import host
    return host(t)


class Gpu:
    """fluca_amd.scalar.Scalar on the grid of an sr.Problem; handles are kept per problem and closed with the module"""

    def __init__(self):
        self.made = {}

    def handles(self, P, fresh=False):
        from fluca_amd.poisson import Poisson
        from fluca_amd.scalar import Scalar
        key = id(P)
        if fresh or key not in self.made:
            Pz = Poisson(P.n, P.xf, sc.poisson_bc(P.bc), 1e-3)
            S = Scalar(Pz, P.bc, P.val, limiter=P.limiter, gamma=P.gamma)
            if fresh:
                return Pz, S
            self.made[key] = (Pz, S, P)         # (P kept: its id stays taken)
        return self.made[key][:2]

    def close(self):
        for Pz, S, _ in self.made.values():
            S.close()
            Pz.close()
        self.made = {}

    def apply(self, P, c, phi):
        """out stands between sentinels (tests/caller_arrays.py's), which must survive the call"""
        import torch
        from tests.caller_arrays import GUARD, SENTINEL
        Pz, S = self.handles(P)
        N = Pz.ncell
        buf = torch.full((N + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        S.diffusion_apply(c, _dev(phi), out=buf[GUARD:GUARD + N])
        got = _host(buf)
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + N:] == SENTINEL).all(), "fl_scalar_diffusion_apply wrote beside out"
        assert not (got[GUARD:GUARD + N].view(np.int64) == np.float64(SENTINEL).view(np.int64)).any(), "cells of out were not written"
        return got[GUARD:GUARD + N].copy().reshape(P.shapes()[0])

    def solve(self, P, c, rtol, maxit, b, x0):
        _, S = self.handles(P)
        x = _dev(x0)
        info = S.diffusion_solve(c, _dev(b), x, rtol, maxit)
        return _host(x).reshape(P.shapes()[0]), info

    def step_imex(self, P, phi, V, dt, s, theta, rtol, maxit, q=None, handles=None):
        _, S = handles or self.handles(P)
        S.set_diffusivity(P.gamma)
        S.set_velocity(*[_dev(v) for v in V])
        x = _dev(phi)
        info = S.step_imex(x, dt, s, theta, rtol, maxit, None if q is None else _dev(q))
        return _host(x).reshape(P.shapes()[0]), info


@pytest.fixture(scope="module")
def gpu():
    g = Gpu()
    yield g
    g.close()


@functools.lru_cache(maxsize=None)
def problem(n, uniform, bcname, short_periodic=False):
    return ir.grid_problem(n, uniform, bcname, short_periodic)


@functools.lru_cache(maxsize=None)
def regime_grid():
    """the smallest (65, ny, nz), ny a multiple of 8, whose k_scalar_cheb plan is that of 512^3 -- blocks per XCD at their cap, every wave keeping one x
    segment -- with more row segments in an XCD's band than the XCD has waves: some waves take a second trip through their loop"""
    from fluca_amd import capi
    f = capi.lib.fldbg_scalar_cheb_plan
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    out = (C.c_int * 5)()
    assert f(512, 512, 512, out, 5) == 5
    big = list(out)
    assert big[3] == 1
    best = None
    for ny in range(8, 129, 8):
        for nz in range(1, 1200):
            assert f(65, ny, nz, out, 5) == 5
            per_xcd, nseg, band, fixed, items = list(out)
            if (per_xcd, fixed) == (big[0], big[3]) and nseg * band * nz > 4 * per_xcd:
                if best is None or 65 * ny * nz < best[0]:
                    best = (65 * ny * nz, (65, ny, nz))
                break
    assert best is not None
    return best[1]


def field(n, kind, seed=7):
    return sc.phi_field(tuple(n), kind, seed)


# ------------------------------------------------------------------------------------------------------------------ apply

def check_apply(be, P, c, phi, label):
    got = be.apply(P, c, phi)
    Dx, E = ir.D(P, phi, np.longdouble, bounds=True)
    want = np.asarray(phi, dtype=np.longdouble) - np.longdouble(c) * Dx
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    tol = sc.rhs_slack(ir.apply_bound(c, phi, Dx, E))
    bad = np.argwhere(err > tol)
    print(f"apply {label}: largest error / bound = {float((err / tol).max()):.3f}")
    assert bad.size == 0, (label, len(bad), tuple(bad[0]), float(err[tuple(bad[0])]), float(tol[tuple(bad[0])]))
    return got


@BOTH
@BCS
@pytest.mark.parametrize("n", [SMALL, SHORT] + RAGGED, ids=ids_n)
def test_apply(gpu, n, bcname, uniform):
    P = problem(n, uniform, bcname, n == SHORT)
    for S in (0.3, 60.0):
        for kind in ("random", "step"):
            check_apply(gpu, P, ir.c_for_S(P, S), field(n, kind), f"{n} {bcname} {'uniform' if uniform else 'stretched'} S={S} {kind}")


@pytest.mark.parametrize("bcname", ["channel", "dirichlet"])
def test_apply_in_the_plan_of_512_cubed(gpu, bcname):
    n = regime_grid()
    print("regime grid", n)
    P = problem(n, False, bcname)
    check_apply(gpu, P, ir.c_for_S(P, 5.0), field(n, "random"), f"{n} {bcname} stretched")


@pytest.mark.parametrize("bcname", ["channel", "periodic"])
@pytest.mark.parametrize("n", [SMALL, RAGGED[0]], ids=ids_n)
def test_apply_on_guarded_unaligned_arrays(gpu, n, bcname):
    """out between sentinels, phi between NaN guards (tests/caller_arrays.py), on 16-byte boundaries (A) and 8 bytes off them (B): the same bits, and no
    word outside out changes"""
    from fluca_amd import capi
    from tests.caller_arrays import Arena
    P = problem(n, False, bcname)
    _, S = gpu.handles(P)
    N, c, phi = P.n[0] * P.n[1] * P.n[2], ir.c_for_S(P, 5.0), field(n, "random")
    res = {}
    for placement in ("A", "B"):
        T = Arena([("phi", N, "in"), ("out", N, "out")], placement)
        assert T.phase("out") == (8 if placement == "B" else 0)
        T.fill("phi", phi)
        T.freeze()
        assert capi.lib.fl_scalar_diffusion_apply(S.h, c, C.c_void_p(T["phi"].data_ptr()), C.c_void_p(T["out"].data_ptr())) == 0
        T.check(written=["out"])
        res[placement] = T.get("out")
    assert np.array_equal(res["A"].view(np.int64), res["B"].view(np.int64))
    assert np.array_equal(res["A"].view(np.int64), np.ascontiguousarray(gpu.apply(P, c, phi)).reshape(-1).view(np.int64))


# ------------------------------------------------------------------------------------------------------------------ two steps at rounding level

def two_step_bound(P, c, b, x0):
    """-> (x_2 in long double, the bound on |binary64 x_2 - x_2| per cell).  Units of U, every quantity the long-double one.
    Step 1:  H_0 = H_c(x_0) is off by a_0 = ir.apply_bound (D's derived bound times c, the product, the difference);  r_0 = b - H_0 by a_0 + |r_0|;
    the diagonal 1 + c (dg_x + dg_y + dg_z), dg = (w_1 + w_2) ih, carries per dg the two table entries (a difference and a reciprocal each: 2), the
    sum, ih (2) and the product: 6 relative, then two sums, the product with c and the sum with 1: DG = 10 relative roundings at most;
    z_0 = r_0 / diag by (a_0 + |r_0|) / diag + (DG + 1) |z_0|;  d_1 = q_1 z_0 by one more:  e_d1 = q_1 (a_0 + |r_0|) / diag + (DG + 2) |d_1|;
    x_1 = x_0 + d_1:  e_x1 = e_d1 + |x_1|.
    Step 2 starts from an x_1 that is off by at most m = max e_x1 U:  H moves by at most (diag + c sum |offdiag|) m <= (2 diag - 1) m, so
    r_1 is off by a_1 + |r_1| + (2 diag - 1) m;  z_1 by that / diag + (DG + 1) |z_1|;  d_2 = p_2 d_1 + q_2 z_1 by |p_2| e_d1 + q_2 e_z1 and the two
    products and the sum, |p_2 d_1| + |q_2 z_1| + |d_2|;  x_2 = x_1 + d_2 by e_x1 + e_d2 + |x_2|."""
    ld, DG = np.longdouble, 10.0
    f64 = lambda a: np.abs(np.asarray(a)).astype(np.float64)
    emin, emax = ir.interval(P, c)
    (p1, q1), (p2, q2) = ir.coefficients(emin, emax, 2)
    dg = ir.diagonal(P, c, ld)
    dgf = dg.astype(np.float64)
    shape = P.shapes()[0]
    x0, b = np.asarray(x0, dtype=ld).reshape(shape), np.asarray(b, dtype=ld).reshape(shape)
    D0, E0 = ir.D(P, x0, ld, bounds=True)
    a0 = ir.apply_bound(c, x0, D0, E0)
    r0 = b - (x0 - ld(c) * D0)
    d1 = ld(q1) * (r0 / dg)
    x1 = x0 + d1
    e_d1 = q1 * (a0 + f64(r0)) / dgf + (DG + 2) * f64(d1)
    e_x1 = e_d1 + f64(x1)
    m = float(e_x1.max())
    D1, E1 = ir.D(P, x1, ld, bounds=True)
    a1 = ir.apply_bound(c, x1, D1, E1)
    r1 = b - (x1 - ld(c) * D1)
    z1 = r1 / dg
    d2 = ld(p2) * d1 + ld(q2) * z1
    x2 = x1 + d2
    e_z1 = (a1 + f64(r1) + (2 * dgf - 1) * m) / dgf + (DG + 1) * f64(z1)
    e_d2 = abs(p2) * e_d1 + q2 * e_z1 + f64(ld(p2) * d1) + f64(ld(q2) * z1) + f64(d2)
    return x2, e_x1 + e_d2 + f64(x2)


def check_two_steps(be, P, S, label, x_is_b=False):
    c = ir.c_for_S(P, S)
    rng = np.random.default_rng(11)
    b = rng.uniform(-1, 1, P.shapes()[0])
    x0 = b if x_is_b else rng.uniform(-1, 1, b.shape)
    got, info = be.solve(P, c, 1e-12, 2, b, x0)
    assert info["steps"] == 2 and info["capped"]
    want, E = two_step_bound(P, c, b, x0)
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    tol = sc.rhs_slack(E)
    # (the recurrence of ir, on D_lines, is the same x_2 within the long-double share of the bound)
    assert (np.abs(ir.chebyshev(P, c, b, x0, 2, np.longdouble) - want).astype(np.float64) <= 2.0 ** -10 * tol).all()
    print(f"two steps {label} S={S}: largest error / bound = {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), (label, S, float((err / tol).max()))


@BOTH
@BCS
@pytest.mark.parametrize("n", [SMALL, SHORT, RAGGED[0]], ids=ids_n)
def test_two_steps_at_rounding_level(gpu, n, bcname, uniform):
    P = problem(n, uniform, bcname, n == SHORT)
    for S in (0.3, 60.0):
        check_two_steps(gpu, P, S, f"{n} {bcname} {'uniform' if uniform else 'stretched'}")
    check_two_steps(gpu, P, 5.0, f"{n} {bcname} x = b", x_is_b=True)


# ------------------------------------------------------------------------------------------------------------------ solve

def same_info(info, P, c, rtol, maxit):
    """steps and capped exactly; interval and bound to a few units in the last place (the library forms a periodic seam's distance from its padded
    centres, ir from the period: the same number to rounding)"""
    emin, emax = ir.interval(P, c)
    k, Bk = ir.steps(emin, emax, rtol, maxit)
    assert (info["steps"], info["capped"]) == (k, Bk > rtol), (info, k, Bk)
    for name, want in (("emin", emin), ("emax", emax)):
        assert abs(info[name] - want) <= 16 * U * want, (name, info[name], want)
    assert abs(info["bound"] - Bk) <= 64 * k * U * Bk + 16 * U, (info["bound"], Bk)
    return k, Bk


def check_solve(be, P, S, rtol, guess, label, manufactured=False, seed=5):
    c = ir.c_for_S(P, S)
    rng = np.random.default_rng(seed)
    shape = P.shapes()[0]
    ld = np.longdouble
    slip = 0.0
    if manufactured:
        x = rng.uniform(-1, 1, shape).astype(ld)
        bl = x - ld(c) * ir.D_lines(P, x, ld)
        b = bl.astype(np.float64)
        # b is rounded: the solution of the rounded system is off by at most max |b - bl| in the maximum norm (|A^-1| <= 1)
        slip = float(np.abs(b - bl).max()) + 2.0 ** -60 * float(np.abs(x).max())
    else:
        b = rng.uniform(-1, 1, shape)
        x = ir.solve_exact(P, c, b)
    x0 = b if guess == "b" else rng.uniform(-1, 1, shape)
    got, info = be.solve(P, c, rtol, 100000, b, x0)
    k, Bk = same_info(info, P, c, rtol, 100000)
    assert Bk <= rtol and not info["capped"]
    w = ir.weights(P, c)
    twin, exact = ir.chebyshev(P, c, b, x0, k, np.float64), ir.chebyshev(P, c, b, x0, k, ld)
    yard = ir.wnorm(w, twin - exact)
    floor = FLOOR_MARGIN * yard + slip * float(np.sqrt(w.sum()))
    e0, e = ir.wnorm(w, np.asarray(x0, dtype=ld) - x), ir.wnorm(w, got.astype(ld) - x)
    ratio = ir.wnorm(w, got.astype(ld) - exact) / yard if yard > 0 else float("nan")
    print(f"solve {label} S={S} rtol={rtol:g} guess={guess}: k = {k}, B_k = {Bk:.3e}, |e| / |e0| = {e / e0:.3e}, GPU error / yardstick = {ratio:.3f}")
    assert e <= Bk * e0 + floor, (label, S, rtol, guess, e, Bk * e0, floor)
    assert ir.wnorm(w, got.astype(ld) - exact) <= floor, (label, "off the long-double recurrence by more than the floor", ratio)


@BOTH
@BCS
def test_solve(gpu, bcname, uniform):
    P = problem(SMALL, uniform, bcname)
    for S in (0.3, 5.0, 60.0):
        for rtol in (1e-4, 1e-8):
            for guess in ("random", "b"):
                check_solve(gpu, P, S, rtol, guess, f"{SMALL} {bcname} {'uniform' if uniform else 'stretched'}")


@pytest.mark.parametrize("n,bcname", [(SHORT, "periodic"), (SHORT, "channel"), ((65, 3, 2), "dirichlet"), ((11, 9, 13), "channel"), ((11, 9, 13), "neumann")])
def test_solve_elsewhere(gpu, n, bcname):
    assert n[0] * n[1] * n[2] <= 1500
    P = problem(n, False, bcname, n == SHORT)
    for S, rtol in ((5.0, 1e-8), (60.0, 1e-4)):
        check_solve(gpu, P, S, rtol, "random", f"{n} {bcname} stretched")


def test_solve_in_the_plan_of_512_cubed(gpu):
    n = regime_grid()
    check_solve(gpu, problem(n, False, "channel"), 5.0, 1e-4, "random", f"{n} channel stretched", manufactured=True)


def test_solve_with_c_zero_copies_b(gpu):
    P = problem(SMALL, False, "channel")
    rng = np.random.default_rng(2)
    b, x0 = rng.uniform(-1, 1, P.shapes()[0]), rng.uniform(-1, 1, P.shapes()[0])
    got, info = gpu.solve(P, 0.0, 1e-6, 100, b, x0)
    assert np.array_equal(got.view(np.int64), b.view(np.int64)) and info["steps"] == 0 and not info["capped"]
    assert (info["emin"], info["emax"], info["bound"]) == (1.0, 1.0, 1.0)
    assert gpu.handles(P)[1].diffusion_interval(0.0) == (1.0, 1.0)
    got, info = gpu.solve(P, ir.c_for_S(P, 5.0), 1e-6, 1, b, x0)          # maxit rounds down to 0: the guess stays
    assert np.array_equal(got.view(np.int64), x0.view(np.int64)) and info["steps"] == 0 and info["capped"]


# ------------------------------------------------------------------------------------------------------------------ the IMEX step

STAGES = 3


def imex_case(P0, target, with_V=True):
    """-> (P with Gamma set, V, dt): a convective Courant number of 0.4 (V = 0: dt = 0.01), Gamma so that fl_scalar_cfl's diffusive number is `target`"""
    if with_V:
        rng = np.random.default_rng(20261020)
        V = [rng.uniform(-1.0, 1.0, s) for s in P0.shapes()[1]]
        dt = 0.4 / sr.cfl(P0, V, 1.0)[0]
    else:
        V, dt = ir.zero_velocity(P0), 0.01
    gamma = target / sr.cfl(ir.with_gamma(P0, 1.0), V, dt)[1]
    return ir.with_gamma(P0, gamma), V, dt


def check_imex(be, P0, target, theta, rtol, label):
    P, V, dt = imex_case(P0, target)
    n = P.n
    phi, q = field(n, "random") * 0.5 + field(n, "step"), sc.source(tuple(n))
    ld = np.longdouble
    want, star, b, Bx = ir.imex_step(P, phi, V, dt, STAGES, theta, q, bounds=True)
    got, info = be.step_imex(P, phi, V, dt, STAGES, theta, rtol, 100000, q)
    c = theta * dt * P.gamma
    k, Bk = same_info(info, P, c, rtol, 100000)
    w = ir.weights(P, c)
    star64, b64 = np.asarray(star, dtype=np.float64), np.asarray(b, dtype=np.float64)
    yard = ir.wnorm(w, ir.chebyshev(P, c, b64, star64, k, np.float64) - ir.chebyshev(P, c, b64, star64, k, ld))
    explicit = float(np.max(Bx)) * (1 + 2.0 ** -10) * float(np.sqrt(w.sum()))
    e0, e = ir.wnorm(w, star - want), ir.wnorm(w, got.astype(ld) - want)
    tol = (1 + Bk) * explicit + Bk * e0 + FLOOR_MARGIN * yard
    print(f"imex {label} out[1]={target} theta={theta}: k = {k}, |e| = {e:.3e}, explicit {explicit:.3e}, B_k |e0| = {Bk * e0:.3e}, floor {FLOOR_MARGIN * yard:.3e}")
    assert e <= tol, (label, target, theta, e, tol)


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("bcname", ["channel", "dirichlet", "periodic"])
def test_step_imex(gpu, bcname, theta):
    P0 = problem(SMALL, False, bcname)
    for target in (0.5, 8.0, 80.0):
        check_imex(gpu, P0, target, theta, 1e-6, f"{SMALL} {bcname} stretched")


def test_step_imex_on_a_ragged_row(gpu):
    check_imex(gpu, problem(RAGGED[0], False, "channel"), 8.0, 1.0, 1e-6, f"{RAGGED[0]} channel stretched")


def test_step_imex_without_diffusivity_is_the_explicit_step(gpu):
    P0 = problem(SMALL, False, "channel")
    P, V, dt = imex_case(P0, 0.0)
    assert P.gamma == 0.0
    phi, q = field(SMALL, "random"), sc.source(SMALL)
    _, S = gpu.handles(P0)
    S.set_diffusivity(0.0)
    S.set_velocity(*[_dev(v) for v in V])
    a = S.step(_dev(phi), dt, STAGES, _dev(q))
    b, info = gpu.step_imex(P, phi, V, dt, STAGES, 1.0, 1e-6, 100, q)
    assert np.array_equal(_host(a).view(np.int64), b.reshape(-1).view(np.int64)) and info["steps"] == 0


def check_maximum_principle(be, bcname, rtol=1e-6):
    """theta = 1, Neumann 0 / periodic / Dirichlet ends, step data, V = 0, a diffusive number of 80: I - c L is an M-matrix with row sums >= 1, so the
    exact solve stays within [min, max] of phi^n and the Dirichlet values (tests/test_scalar_implicit_host.py); the Chebyshev iterate may leave it by
    rtol (max - min)"""
    P0 = ir.grid_problem(SMALL, False, bcname, homogeneous_neumann=True)
    P, V, dt = imex_case(P0, 80.0, with_V=False)
    phi = field(SMALL, "step")
    got, info = be.step_imex(P, phi, V, dt, STAGES, 1.0, rtol, 100000)
    ends = [v for k, v in zip(P.bc, P.val) if k == sr.DIRICHLET]
    lo, hi = min([phi.min()] + ends), max([phi.max()] + ends)
    wide = rtol * (hi - lo)
    print(f"maximum principle {bcname}: k = {info['steps']}, [{got.min() - lo:.3e}, {hi - got.max():.3e}] inside, allowed outside {wide:.3e}")
    assert lo - wide <= got.min() and got.max() <= hi + wide, (bcname, lo, float(got.min()), float(got.max()), hi, wide)


@BCS
def test_backward_euler_keeps_the_maximum_principle(gpu, bcname):
    check_maximum_principle(gpu, bcname)


# ------------------------------------------------------------------------------------------------------------------ history

def test_history_changes_no_bit(gpu):
    """step_imex after rhs, step, boundary_flux and an earlier solve = step_imex on a fresh handle; fl_scalar_step after an implicit step = fl_scalar_step on
    a fresh handle (the work arrays the two paths share are written before they are read)"""
    P0 = problem(SMALL, False, "channel")
    P, V, dt = imex_case(P0, 8.0)
    phi, q = field(SMALL, "random"), sc.source(SMALL)
    bits = lambda a: np.ascontiguousarray(a).reshape(-1).view(np.int64)
    fresh = {}
    for theta in (1.0, 0.5):
        h = gpu.handles(P, fresh=True)
        fresh[theta] = gpu.step_imex(P, phi, V, dt, STAGES, theta, 1e-6, 1000, q, handles=h)[0]
        h[1].close(); h[0].close()
    h = gpu.handles(P, fresh=True)
    S = h[1]
    S.set_velocity(*[_dev(v) for v in V])
    want_step = _host(S.step(_dev(phi), dt, 5, _dev(q)))
    S.rhs(_dev(phi), _dev(q))
    S.boundary_flux(_dev(phi))
    x = _dev(field(SMALL, "step"))
    S.diffusion_solve(ir.c_for_S(P, 60.0), _dev(phi), x, 1e-8, 1000)
    for theta in (1.0, 0.5):
        got = gpu.step_imex(P, phi, V, dt, STAGES, theta, 1e-6, 1000, q, handles=h)[0]
        assert np.array_equal(bits(got), bits(fresh[theta])), theta
    S.set_velocity(*[_dev(v) for v in V])
    assert np.array_equal(bits(_host(S.step(_dev(phi), dt, 5, _dev(q)))), bits(want_step))
    h[1].close(); h[0].close()


# ------------------------------------------------------------------------------------------------------------------ pending inputs

@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_solve_and_step_imex_behind_a_delay(theta):
    """one solve and one step_imex queued behind a delay on the handle's stream, their inputs produced behind the delay and poisoned right after the
    calls (tests/test_gpu_stream_order.py's two plays): the idle stream's bits, and the delay still pending when the last call has returned"""
    from fluca_amd.poisson import Poisson
    from fluca_amd.scalar import Scalar
    from tests.test_gpu_stream_order import both
    P0 = problem(RAGGED[0], False, "channel")
    P, V, dt = imex_case(P0, 8.0)
    n = P.n
    N = n[0] * n[1] * n[2]
    Pz = Poisson(P.n, P.xf, sc.poisson_bc(P.bc), 1e-3)
    Sc = Scalar(Pz, P.bc, P.val, gamma=P.gamma)
    c = ir.c_for_S(P, 5.0)
    rng = np.random.default_rng(4)
    inputs = {"b": rng.uniform(-1, 1, N), "x": rng.uniform(-1, 1, N), "phi": field(n, "random"), "q": sc.source(tuple(n)), **{f"V{d}": V[d] for d in range(3)}}
    Sc.diffusion_solve(c, _dev(inputs["b"]), _dev(inputs["x"]), 1e-6, 1000)          # the first implicit call allocates
    Pz.synchronize()

    def seq(S):
        Sc.set_velocity(S["V0"], S["V1"], S["V2"])
        info = S.do(Sc.diffusion_solve, c, S["b"], S["x"], 1e-6, 1000); S.snap("x", "x")
        S.release("b")
        info2 = S.do(Sc.step_imex, S["phi"], dt, STAGES, theta, 1e-6, 1000, S["q"]); S.snap("phi", "phi")
        S.still_pending(f"solve ({info['steps']} steps) + step_imex theta={theta} ({info2['steps']} steps)")
        S.release("q", "V0", "V1", "V2", "x", "phi")
    try:
        both(f"implicit scalar theta={theta}", Pz, seq, inputs, {})
    finally:
        Sc.close()
        Pz.close()


# ------------------------------------------------------------------------------------------------------------------ errors

def test_errors_leave_the_outputs_alone(gpu):
    from fluca_amd import capi
    lib = capi.lib
    P = problem(SMALL, False, "channel")
    Pz, S = gpu.handles(P, fresh=True)
    N = Pz.ncell
    rng = np.random.default_rng(9)
    keep = rng.uniform(-1, 1, N)
    x, b = _dev(keep), _dev(rng.uniform(-1, 1, N))
    px, pb = C.c_void_p(x.data_ptr()), C.c_void_p(b.data_ptr())
    info = capi.fl_scalar_cheb_info(steps=-7)
    nan, inf = float("nan"), float("inf")
    lo, hi = C.c_double(-1.0), C.c_double(-1.0)
    assert lib.fl_scalar_diffusion_interval(S.h, 1.0, None, C.byref(hi)) == -85 and lib.fl_scalar_diffusion_interval(S.h, 1.0, C.byref(lo), None) == -85
    for c in (-1.0, nan, inf):
        assert lib.fl_scalar_diffusion_interval(S.h, c, C.byref(lo), C.byref(hi)) == -63 and (lo.value, hi.value) == (-1.0, -1.0)
        assert lib.fl_scalar_diffusion_apply(S.h, c, pb, px) == -63
        assert lib.fl_scalar_diffusion_solve(S.h, c, 1e-6, 10, pb, px, C.byref(info)) == -63
    assert lib.fl_scalar_diffusion_apply(S.h, 1.0, None, px) == -85 and lib.fl_scalar_diffusion_apply(S.h, 1.0, px, None) == -85
    assert lib.fl_scalar_diffusion_apply(S.h, 1.0, px, px) == -62
    assert lib.fl_scalar_diffusion_solve(S.h, 1.0, 1e-6, 10, None, px, None) == -85 and lib.fl_scalar_diffusion_solve(S.h, 1.0, 1e-6, 10, pb, None, None) == -85
    assert lib.fl_scalar_diffusion_solve(S.h, 1.0, 1e-6, 10, px, px, C.byref(info)) == -62
    for rtol in (0.0, 1.0, -0.5, nan, inf):
        assert lib.fl_scalar_diffusion_solve(S.h, 1.0, rtol, 10, pb, px, C.byref(info)) == -63
        assert lib.fl_scalar_step_imex(S.h, 0.1, 3, 1.0, rtol, 10, None, px, C.byref(info)) == -63
    assert lib.fl_scalar_diffusion_solve(S.h, 1.0, 1e-6, -1, pb, px, C.byref(info)) == -63
    # step_imex: its own ranges, then the state
    for theta in (0.49, 1.01, 0.0, nan):
        assert lib.fl_scalar_step_imex(S.h, 0.1, 3, theta, 1e-6, 10, None, px, C.byref(info)) == -63
    for dt in (nan, inf, -0.1):
        assert lib.fl_scalar_step_imex(S.h, dt, 3, 1.0, 1e-6, 10, None, px, C.byref(info)) == -63
    assert lib.fl_scalar_step_imex(S.h, 0.1, 1, 1.0, 1e-6, 10, None, px, C.byref(info)) == -63
    assert lib.fl_scalar_step_imex(S.h, 0.1, 3, 1.0, 1e-6, -2, None, px, C.byref(info)) == -63
    assert lib.fl_scalar_step_imex(S.h, 0.1, 3, 1.0, 1e-6, 10, None, None, C.byref(info)) == -85
    S.set_diffusivity(0.1)
    assert lib.fl_scalar_step_imex(S.h, 0.1, 3, 1.0, 1e-6, 10, None, px, C.byref(info)) == -73            # no velocity yet
    Pz.synchronize()
    assert info.steps == -7
    assert np.array_equal(_host(x).view(np.int64), keep.view(np.int64)), "an argument error wrote to an output"
    S.close()
    Pz.close()


def _ranks_worker(R, case):
    import torch
    from fluca_amd import capi
    from fluca_amd.scalar import Scalar
    from tests.test_gpu_config5 import _handle
    P, d, s = _handle(R, case)
    with torch.cuda.stream(s):
        S = Scalar(P, case.kinds, case.vals, gamma=0.1)
        S.set_velocity(*[torch.zeros(m, dtype=torch.float64, device="cuda") for m in P.nface])
        keep = np.random.default_rng(R.rank).uniform(-1, 1, P.ncell)
        x, b = torch.as_tensor(keep, device="cuda"), torch.zeros(P.ncell, dtype=torch.float64, device="cuda")
        px, pb = C.c_void_p(x.data_ptr()), C.c_void_p(b.data_ptr())
        rcs = (capi.lib.fl_scalar_diffusion_apply(S.h, 1.0, pb, px), capi.lib.fl_scalar_diffusion_solve(S.h, 1.0, 1e-6, 10, pb, px, None),
               capi.lib.fl_scalar_step_imex(S.h, 0.1, 3, 1.0, 1e-6, 10, None, px, None))
        lo, hi = S.diffusion_interval(1.0)            # host arithmetic on the global tables: every rank gets the one-rank interval
        s.synchronize()
        same = np.array_equal(x.cpu().numpy().view(np.int64), keep.view(np.int64))
        S.close()
    P.close()
    return rcs, same, (lo, hi)


def test_several_ranks_are_not_supported():
    from tests import inproc
    from tests import scalar_ranks as rk
    case = rk.Case((8, 6, 4), (2, 1, 1), "channel")
    res = inproc.run_threads(case.size, _ranks_worker, case)
    for rcs, same, iv in res:
        assert rcs == (-56, -56, -56) and same
        assert iv == res[0][2] and abs(iv[0] - ir.interval(case.problem(), 1.0)[0]) <= 16 * U
