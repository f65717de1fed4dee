"""No GPU: the arithmetic behind the implicit scalar diffusion (include/fluca_hip_implicit.h) on tests/scalar_implicit_reference.py -- the symmetry
of W (I - c L), the Gershgorin interval against dense eigenvalues, the Chebyshev bound B_k against the long-double recurrence, the maximum principle
of the exact backward-Euler step -- and what of the library runs without a device: fl_scalar_cheb_steps, the NULL checks, the header against the
ctypes table and the exports, and the stream-order rows of the new functions.

Grids: the four boundary sets of tests/scalar_cases.py, uniform and stretched, with an axis of one and of two cells among them (a one-cell periodic
axis contributes nothing; a two-cell periodic axis has both faces of a cell on the same neighbour)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import scalar_cases as sc
from tests import scalar_implicit_reference as ir
from tests import scalar_reference as sr
from tests import stream_order as so
from tests.test_stream_order import problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(7, 5, 3), (6, 2, 1), (5, 1, 4), (2, 9, 2)]
S_VALUES = (0.3, 5.0, 60.0)
BOTH = pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "stretched"])
BCS = pytest.mark.parametrize("bcname", list(sc.BC_SETS))
NS = pytest.mark.parametrize("n", GRIDS, ids=lambda n: "x".join(map(str, n)))


def problem(n, uniform, bcname):
    return ir.grid_problem(n, uniform, bcname)


@BOTH
@BCS
@NS
def test_lines_are_sr_rhs_and_the_matrix_is_the_operator(n, bcname, uniform):
    """D_lines (what the recurrences run on) against D = sr.rhs with V = 0, Gamma = 1 within its derived bound; the assembled matrix and d_bc against
    both; the diagonal from the rows against the matrix's"""
    P = problem(n, uniform, bcname)
    phi = sc.phi_field(n, "random")
    want, E = ir.D(P, phi, np.longdouble, bounds=True)
    for got in (ir.D_lines(P, phi), ir.D_lines(P, phi, np.longdouble), ir.D(P, phi)):
        assert (np.abs(got - want).astype(np.float64) <= sc.rhs_slack(E)).all()
    c = ir.c_for_S(P, 5.0)
    A, dbc, dg = ir.assemble(P, c)
    H = (A @ phi.reshape(-1) - c * dbc).reshape(phi.shape)
    exact = phi - np.longdouble(c) * want
    assert (np.abs(H - exact).astype(np.float64) <= 4 * ir.apply_bound(c, phi, want, E) * sr.U * (1 + 2.0 ** -10) + np.finfo(float).tiny).all()
    assert np.abs(dg - ir.diagonal(P, c)).max() <= 8 * sr.U * dg.max()
    assert (dg >= 1.0).all()


@BOTH
@BCS
@NS
def test_weighted_matrix_is_symmetric(n, bcname, uniform):
    """a face's 1 / distance and its area are shared by the two cells: vol_a ic_f / h_a = (area of f) ic_f on either side"""
    P = problem(n, uniform, bcname)
    A, _, _ = ir.assemble(P, ir.c_for_S(P, 5.0))
    W = sr.volumes(P).reshape(-1)
    WA = (A.multiply(W[:, None])).toarray()
    assert np.abs(WA - WA.T).max() <= 8 * sr.U * np.abs(WA).max()


@BOTH
@BCS
@NS
def test_spectrum_lies_in_the_interval(n, bcname, uniform):
    P = problem(n, uniform, bcname)
    assert n[0] * n[1] * n[2] <= 400
    for S in S_VALUES:
        c = ir.c_for_S(P, S)
        assert abs(ir.S_of(P, c) - S) <= 4 * sr.U * S
        emin, emax = ir.interval(P, c)
        A, _, dg = ir.assemble(P, c)
        ev = np.linalg.eigvals(A.toarray() / dg.reshape(-1)[:, None])
        assert np.abs(ev.imag).max() <= 1e-9, "diag^-1 A is similar to a symmetric matrix: a real spectrum"
        slack = 1e-12 * emax
        assert emin - slack <= ev.real.min() and ev.real.max() <= emax + slack, (S, emin, ev.real.min(), ev.real.max(), emax)
        assert abs(emax / emin - (1 + 2 * S)) <= 1e-12 * (1 + 2 * S)


def test_an_axis_of_one_cell_contributes_nothing():
    P = problem((5, 1, 4), True, "periodic")
    assert ir.omega_max(P, 1) == 0.0
    Pd = problem((5, 1, 4), True, "dirichlet")                          # no partner, but the Dirichlet faces stand on the true diagonal
    assert ir.omega_max(Pd, 1) == 0.0
    N, Dk = sr.NEUMANN, sr.DIRICHLET
    Py = sr.Problem(sc.faces((5, 1, 4), True), (N, N, Dk, Dk, N, N), (0.0,) * 6)
    Pn = sr.Problem(sc.faces((5, 1, 4), True), (N,) * 6, (0.0,) * 6)
    ic, ih = ir.axis_rows(Py, 1)
    assert np.allclose(ir.diagonal(Py, 1.0) - ir.diagonal(Pn, 1.0), (ic[0] + ic[1]) * ih[0], rtol=1e-13)
    A, _, dg = ir.assemble(Py, 1.0)
    assert np.allclose(dg, ir.diagonal(Py, 1.0), rtol=1e-13)


@BOTH
@BCS
@pytest.mark.parametrize("n", [(7, 5, 3), (6, 2, 1)], ids=lambda n: "x".join(map(str, n)))
def test_long_double_recurrence_keeps_the_bound(n, bcname, uniform):
    """|e_k| <= B_k |e_0| in the norm sum vol diag e^2 at every even k up to the chosen one"""
    P = problem(n, uniform, bcname)
    rng = np.random.default_rng(3)
    b = rng.uniform(-1, 1, P.shapes()[0])
    for S, rtol in ((0.3, 1e-8), (5.0, 1e-8), (60.0, 1e-4), (60.0, 1e-8)):
        c = ir.c_for_S(P, S)
        emin, emax = ir.interval(P, c)
        k, Bk = ir.steps(emin, emax, rtol, 10000)
        assert k % 2 == 0 and Bk <= rtol and (k == 2 or ir.bound(emin, emax, k - 2) > rtol)
        x = ir.solve_exact(P, c, b)
        for x0 in (rng.uniform(-1, 1, b.shape), b):
            xs = ir.chebyshev(P, c, b, x0, k, np.longdouble, every=True)
            w = ir.weights(P, c)
            e0 = ir.wnorm(w, xs[0] - x)
            for j in range(2, k + 1, 2):
                assert ir.wnorm(w, xs[j] - x) <= ir.bound(emin, emax, j) * e0 * (1 + 1e-9) + 1e-17 * e0, (S, rtol, j)


@BCS
def test_exact_backward_euler_keeps_the_maximum_principle(bcname):
    """theta = 1, homogeneous Neumann / periodic / Dirichlet ends, step data, a diffusion number of about 80: the exact solve stays within [min, max] of
    phi^n and the Dirichlet values with no widening (I - c L is an M-matrix with row sums >= 1)"""
    n = (7, 5, 3)
    kinds, vals = sc.BC_SETS[bcname]
    vals = tuple(v if k == sr.DIRICHLET else 0.0 for k, v in zip(kinds, vals))
    P = sr.Problem(sc.faces(n, False), kinds, vals, gamma=1.0)
    phi = sc.phi_field(n, "step")
    dt = 80.0 / sr.cfl(P, ir.zero_velocity(P), 1.0)[1]
    new, star, b = ir.imex_step(P, phi, ir.zero_velocity(P), dt, 3, 1.0)
    assert np.array_equal(np.asarray(star, dtype=np.float64), phi)          # V = 0, Gamma = 0: the explicit part moves nothing
    lo = min([phi.min()] + [v for k, v in zip(kinds, vals) if k == sr.DIRICHLET])
    hi = max([phi.max()] + [v for k, v in zip(kinds, vals) if k == sr.DIRICHLET])
    assert lo <= new.min() and new.max() <= hi, (lo, float(new.min()), float(new.max()), hi)


# ---- the library, without a device ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def capi():
    from fluca_amd import build
    build.build()
    from fluca_amd import capi
    return capi


def test_cheb_steps_is_the_helpers_count(capi):
    k, B = C.c_int(-1), C.c_double(-1.0)
    f = capi.lib.fl_scalar_cheb_steps
    for S in (1e-3, 0.3, 5.0, 60.0, 1e4):
        emin, emax = 1.0 / (1.0 + S), (1.0 + 2.0 * S) / (1.0 + S)
        for rtol in (0.5, 1e-4, 1e-8, 1e-13):
            for maxit in (10000, 7, 2, 1, 0):
                assert f(emin, emax, rtol, maxit, C.byref(k), C.byref(B)) == 0
                want = ir.steps(emin, emax, rtol, maxit)
                assert (k.value, B.value) == want, (S, rtol, maxit, k.value, B.value, want)
                assert k.value % 2 == 0 and k.value <= maxit
                assert B.value <= rtol or k.value == maxit - maxit % 2
    assert f(1.0, 1.0, 1e-6, 100, C.byref(k), C.byref(B)) == 0 and k.value == 2 and B.value == 0.0      # a point interval: the first step is exact
    for rtol in (0.0, 1.0, -1e-3, 1.5, float("nan"), float("inf")):
        assert f(0.5, 1.5, rtol, 100, C.byref(k), C.byref(B)) == -63
    assert f(0.5, 1.5, 1e-6, -1, C.byref(k), C.byref(B)) == -63
    for emin, emax in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (1.0, float("inf"))):
        assert f(emin, emax, 1e-6, 100, C.byref(k), C.byref(B)) == -63
    assert f(0.5, 1.5, 1e-6, 100, None, C.byref(B)) == -85 and f(0.5, 1.5, 1e-6, 100, C.byref(k), None) == -85


def test_null_handles(capi):
    lib = capi.lib
    a, b = C.c_double(), C.c_double()
    x = C.c_void_p(4096)                       # never dereferenced: the handle is checked first
    assert lib.fl_scalar_diffusion_interval(None, 1.0, C.byref(a), C.byref(b)) == -85
    assert lib.fl_scalar_diffusion_apply(None, 1.0, x, x) == -85
    assert lib.fl_scalar_diffusion_solve(None, 1.0, 1e-6, 10, x, x, None) == -85
    assert lib.fl_scalar_step_imex(None, 0.1, 3, 1.0, 1e-6, 10, None, x, None) == -85


def implicit_header():
    return open(os.path.join(ROOT, "include", "fluca_hip_implicit.h")).read()


def test_header_table_and_exports_name_the_same_functions(capi):
    decl = so.declarations(implicit_header())
    assert sorted(decl) == sorted(capi.PROTOTYPES_IMPLICIT) and len(decl) == 5
    for name, (params, comment) in decl.items():
        assert hasattr(capi.lib, name), name
        assert len(params) == len(capi.PROTOTYPES_IMPLICIT[name][1]), name
        assert comment.strip(), f"{name} has no comment"
    assert not set(capi.PROTOTYPES_IMPLICIT) & set(capi.PROTOTYPES)
    main = open(os.path.join(ROOT, "include", "fluca_hip.h")).read()
    assert not re.search(r"fl_scalar_(diffusion|step_imex|cheb)", main) and '#include "fluca_hip.h"' in implicit_header()


# the stream-order contract of the new functions, in the words of tests/stream_order.py
TABLE = {
    "fl_scalar_cheb_steps": (so.HOST, dict(steps=so.C, bound=so.C)),
    "fl_scalar_diffusion_interval": (so.HOST, dict(emin=so.C, emax=so.C)),
    "fl_scalar_diffusion_apply": (so.ASYNC, dict(phi_dev=so.C, out_dev=so.C)),
    "fl_scalar_diffusion_solve": (so.ASYNC, dict(b_dev=so.C, x_dev=so.C, info=so.C)),
    "fl_scalar_step_imex": (so.ASYNC, dict(source_dev=so.C, phi_dev=so.C, info=so.C)),
}


def test_stream_order_rows_of_the_new_functions():
    header = implicit_header()
    assert problems(TABLE, header) == []
    decl = so.declarations(header)
    for name in ("fl_scalar_diffusion_apply", "fl_scalar_diffusion_solve", "fl_scalar_step_imex"):
        assert TABLE[name][0] == so.ASYNC
        assert re.search(r"[Ee]nqueues and returns", decl[name][1]), name
        assert "CONSUMED" in decl[name][1], name
    short = dict(TABLE)
    del short["fl_scalar_step_imex"]
    assert len(problems(short, header)) == 1
