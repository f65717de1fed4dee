"""CPU: StepOracle.form_function (oracle/fluca_oracle.py) -- the right-hand side of a CNLinear step and v0interp -- pinned to mathematics, and
step_once pinned to what it returned before form_function was split out of it.

The oracle and the C host mirror were written from the same reference lines, so a mistake shared by both passes every parity test.  Here the wall
coefficients are checked against what they discretise, on stretched grids, on both sides of every axis: the one-sided rows reproduce polynomials of
their order EXACTLY, so the assembled right-hand side must equal the analytic derivative up to the rounding of one row.

Tolerance (derived, the same everywhere): a row  sum_k c_k x_k  evaluated in floating point differs from its exact value by at most about
(number of terms + roundings in each coefficient) * 2^-53 * sum_k |c_k| |x_k|; the rows here have 4 to 10 terms whose errors do not all line up, and
the bound used is  8 * 2^-53 * sum |coefficient| |value|  with the sum over the assembled CSR row (or the 1-D row of G, B, T) plus the boundary term."""
import os
from fractions import Fraction

import numpy as np
import pytest

from oracle import fluca_oracle as fo
from tests import step_rhs as sr

U = 2.0 ** -53
N = (7, 6, 5)
# cv = mu dt / (2 rho) = 1 and kappa = dt / rho = 1: momrhs = v0 + (L v0 + vbcL) - (G p + vbcG), every operator at its own magnitude
RHO, MU, DT = 1.0, 2.0, 1.0


def _grid(bc):
    from tests.gpu_common import stretched_faces
    return fo.Grid(N, stretched_faces(N, sr.BOX), bc, DT / RHO)


def _centres(g):
    return [0.5 * (g.xf[d][1:] + g.xf[d][:-1]) for d in range(3)]


def _poly(coef, x):
    """exact value (Fraction) of sum coef[k] x^k at the float x"""
    xf = Fraction(float(x))
    return sum(Fraction(c) * xf ** k for k, c in enumerate(coef))


def _cell_field(g, ax, coef):
    """float field on the cells that depends on the coordinate of axis ax only: the rounded polynomial"""
    xc = _centres(g)[ax]
    line = np.array([float(_poly(coef, x)) for x in xc])
    shp = [1, 1, 1]
    shp[2 - ax] = g.n[ax]
    return np.broadcast_to(line.reshape(shp), (g.n[2], g.n[1], g.n[0])).ravel().copy()


def test_step_once_returns_what_it_returned_before_the_split(golden_dir):
    """tests/golden/step_once_steps.npz: v, V, p, phalf and the outer iteration count of two steps of a cavity and of a channel with an unsteady outlet,
    recorded from step_once before form_function existed (tests/golden/gen_step_once_fixtures.py) -- bit for bit.  (rnorm comes out of numpy's
    BLAS dot, whose summation order belongs to the machine: compared to 1e-10.)"""
    ref = np.load(os.path.join(golden_dir, "step_once_steps.npz"))
    seen = 0
    for name in sr.golden_step_cases():
        out = sr.run_golden_steps(name)
        for k, a in out.items():
            if k.endswith("_rnorm"):
                assert np.allclose(a, ref[k], rtol=1e-10, atol=0.0), k
            else:
                assert a.shape == ref[k].shape and np.array_equal(a, ref[k]), k
            seen += 1
    assert seen == len(ref.files) == 32


@pytest.mark.parametrize("ax", [0, 1, 2])
def test_wall_row_of_L_is_the_exact_second_derivative_of_a_cubic(ax):
    """cl = 2 (h2 + h3) / (h1 (h1 + h2) (h1 + h3)): the four-point one-sided second derivative through the wall value.  u_q = a cubic in the
    coordinate of axis ax (a different one per component), every wall's value = u on the wall at time t and 0 at t + dt (so that the wall terms
    of t + dt and of C drop out): momrhs = u + (L u + vbcL(t)), which in the two wall-adjacent layers of axis ax must be u + u''."""
    g = _grid([sr.V] * 6)
    cubics = [(0.3, -1.1, 2.3, 1.7), (-0.7, 0.9, -1.3, 2.9), (1.9, 0.4, 3.1, -2.2)]
    v0 = np.concatenate([_cell_field(g, ax, cubics[q]) for q in range(3)])
    t0 = 0.25

    def velocity(b, t, X):
        if t != t0:
            return np.zeros((3, len(X)))
        return np.array([[float(_poly(cubics[q], x[ax])) for x in X] for q in range(3)])

    so = fo.StepOracle(g, DT, RHO, MU, velocity=velocity)
    so.t = t0
    momrhs, _, _, scale = so.form_function(v0, [np.zeros(nf) for nf in g.nface], np.zeros(g.ncell))
    rp, col, val = so.L.arrays()
    rowabs = np.add.reduceat(np.abs(val) * np.abs(v0)[col], rp[:-1])
    xc, xf, n = _centres(g)[ax], g.xf[ax], g.n[ax]
    checked = 0
    for side in (0, 1):
        i = n - 1 if side else 0
        if side == 0:
            h1, h2, h3 = xc[0] - xf[0], xc[1] - xc[0], xc[2] - xc[0]
        else:
            h1, h2, h3 = xf[n] - xc[n - 1], xc[n - 1] - xc[n - 2], xc[n - 1] - xc[n - 3]
        cl = 2.0 * (h2 + h3) / (h1 * (h1 + h2) * (h1 + h3))
        for q in range(3):
            a = cubics[q]
            want = _poly(a, xc[i]) + _poly((2 * Fraction(a[2]), 6 * Fraction(a[3])), xc[i])        # u + u''
            wall = abs(float(_poly(a, xf[n] if side else xf[0])))
            got = so._layer(momrhs[q * g.ncell:(q + 1) * g.ncell].reshape(so.cshape), ax, i)
            absrow = so._layer((np.abs(v0) + rowabs)[q * g.ncell:(q + 1) * g.ncell].reshape(so.cshape), ax, i) + cl * wall
            err = np.abs(got - float(want))
            print(f"axis {ax} side {side} component {q}: max err / (2^-53 sum|c||x|) = {float((err / (U * absrow)).max()):.2f}")
            assert (err <= 8 * U * absrow).all(), (ax, side, q, float((err / (U * absrow)).max()))
            # the term scale of form_function is this very sum (next to the other walls it holds their boundary terms as well)
            sc = so._layer(scale["v"][q * g.ncell:(q + 1) * g.ncell].reshape(so.cshape), ax, i)
            assert (sc >= absrow * (1 - 1e-12)).all() and np.allclose(sc[1:-1, 1:-1], absrow[1:-1, 1:-1], rtol=1e-12)
            checked += got.size
    assert checked == 2 * 3 * g.ncell // n


@pytest.mark.parametrize("ax", [0, 1, 2])
def test_outlet_row_of_G_is_the_exact_first_derivative_of_a_quadratic(ax):
    """cg = -+ h2 / (h1 (h1 + h2)): the one-sided first derivative through the outlet pressure.  p = a quadratic in the coordinate of axis ax,
    the outlet pressure = p on the boundary, v0 = 0: momrhs_ax = -(G p + vbcG), which in the two outlet-adjacent layers must be -p'."""
    bc = [sr.V] * 6
    bc[2 * ax] = bc[2 * ax + 1] = sr.O
    g = _grid(bc)
    quad = (0.6, -1.7, 2.9)
    p = _cell_field(g, ax, quad)
    pressure = lambda b, t, X: np.array([float(_poly(quad, x[ax])) for x in X])
    so = fo.StepOracle(g, DT, RHO, MU, velocity=lambda b, t, X: np.zeros((3, len(X))), pressure=pressure)
    momrhs, interprhs, _, scale = so.form_function(np.zeros(3 * g.ncell), [np.zeros(nf) for nf in g.nface], p)
    G1 = so._line_matrix("G", ax)
    xc, xf, n = _centres(g)[ax], g.xf[ax], g.n[ax]
    pline = np.array([float(_poly(quad, x)) for x in xc])
    for side in (0, 1):
        i = n - 1 if side else 0
        h1, h2 = (xf[n] - xc[n - 1], xc[n - 1] - xc[n - 2]) if side else (xc[0] - xf[0], xc[1] - xc[0])
        cg = (1.0 if side else -1.0) * h2 / (h1 * (h1 + h2))
        want = -_poly((Fraction(quad[1]), 2 * Fraction(quad[2])), xc[i])
        absrow = float(np.abs(G1[i]) @ np.abs(pline)) + abs(cg) * abs(float(_poly(quad, xf[n] if side else xf[0])))
        got = so._layer(momrhs[ax * g.ncell:(ax + 1) * g.ncell].reshape(so.cshape), ax, i)
        err = np.abs(got - float(want))
        print(f"axis {ax} side {side}: max err / (2^-53 sum|c||x|) = {float(err.max() / (U * absrow)):.2f}")
        assert (err <= 8 * U * absrow).all(), (ax, side, float(err.max() / (U * absrow)))
        assert np.allclose(so._layer(scale["v"][ax * g.ncell:(ax + 1) * g.ncell].reshape(so.cshape), ax, i), absrow, rtol=1e-12)
    # a steady outlet pressure leaves no Rhie-Chow boundary term: interprhs is exactly zero
    assert all(not a.any() for a in interprhs)
    # the other two components see no pressure gradient: p is constant along their axes (the rows sum to zero up to their rounding)
    for d in range(3):
        if d != ax:
            absG = so._along(np.abs(so._line_matrix("G", d)), np.abs(p).reshape(so.cshape), d).ravel()
            assert (np.abs(momrhs[d * g.ncell:(d + 1) * g.ncell]) <= 8 * U * absG).all()


def test_T_and_B_with_wall_values_reproduce_a_linear_field():
    """B (every component on every face family) and T (the face-normal one) interpolate between the two cell centres next to a face: exact for
    u_q = a_q + b_q . x.  With the wall values inserted (W) or carried by interprhs (T's boundary-condition vector, at t + dt) the whole face arrays
    equal the linear field at the face centres: wall faces bit for bit (an insertion), inner faces to the rounding of a two-term row."""
    g = _grid([sr.V] * 6)
    lin = [(0.4, 1.3, -0.8, 2.1), (-1.2, 0.7, 1.9, -0.6), (0.9, -2.3, 0.5, 1.1)]         # a, bx, by, bz
    field = lambda q, X: lin[q][0] + lin[q][1] * X[..., 0] + lin[q][2] * X[..., 1] + lin[q][3] * X[..., 2]
    xc = _centres(g)
    Z, Y, X = np.meshgrid(xc[2], xc[1], xc[0], indexing="ij")
    v0 = np.concatenate([field(q, np.stack([X, Y, Z], axis=-1)).ravel() for q in range(3)])
    t0 = 0.5
    # steady in time except for a factor that tells t from t + dt: W must carry t, interprhs t + dt
    velocity = lambda b, t, Xb: np.stack([field(q, Xb) for q in range(3)]) * (1.0 if t == t0 else 3.0)
    so = fo.StepOracle(g, DT, RHO, MU, velocity=velocity)
    so.t = t0
    _, interprhs, W, scale = so.form_function(v0, [np.zeros(nf) for nf in g.nface], np.zeros(g.ncell))
    Tv = g.apply_T(v0, interprhs)
    absB = g.apply_B(np.abs(v0))
    for d in range(3):
        assert all(w >= 0.0 for f in range(1, g.n[d]) for c in range(3) for _, w in g.B_row(d, f, c)) and all(w >= 0.0 for f in range(1, g.n[d]) for _, w in g.T_row(d, f))
        pos = [xc[0], xc[1], xc[2]]
        pos[d] = g.xf[d]
        Zf, Yf, Xf = np.meshgrid(pos[2], pos[1], pos[0], indexing="ij")
        Xb = np.stack([Xf, Yf, Zf], axis=-1)
        inner = [slice(None)] * 3
        inner[2 - d] = slice(1, g.n[d])
        inner = tuple(inner)
        for side in (0, 1):
            wall = [slice(None)] * 3
            wall[2 - d] = -1 if side else 0
            wall = tuple(wall)
            for q in range(3):
                assert np.array_equal(W[q * 3 + d].reshape(so.fshape[d])[wall], field(q, Xb)[wall]), (d, side, q)
            assert np.array_equal(interprhs[d].reshape(so.fshape[d])[wall], 3.0 * field(d, Xb)[wall]), (d, side)
            assert np.array_equal(Tv[d].reshape(so.fshape[d])[wall], 3.0 * field(d, Xb)[wall])
            assert np.array_equal(scale["V"][d].reshape(so.fshape[d])[wall], np.abs(3.0 * field(d, Xb)[wall]))
        assert not interprhs[d].reshape(so.fshape[d])[inner].any()
        for q in range(3):
            # the exact field at the face centres: the linear function of the float coordinates, evaluated in float (3 products, 3 sums: 6 roundings
            # of at most sum |term|, on top of the row's own)
            want = field(q, Xb)[inner]
            mag = (abs(lin[q][0]) + abs(lin[q][1] * Xb[..., 0]) + abs(lin[q][2] * Xb[..., 1]) + abs(lin[q][3] * Xb[..., 2]))[inner]
            tol = 8 * U * absB[q * 3 + d].reshape(so.fshape[d])[inner] + 6 * U * mag
            assert (np.abs(W[q * 3 + d].reshape(so.fshape[d])[inner] - want) <= tol).all(), (d, q)
            if q == d:
                assert (np.abs(Tv[d].reshape(so.fshape[d])[inner] - want) <= tol).all(), d


def test_form_function_takes_step_time_and_half_step_pressure_from_the_oracle():
    """step 0 reads p0 and the outlet pressure at t; a later step reads phalf and the outlet pressure at t - dt / 2 -- set up directly, without stepping"""
    case = sr.make_case((6, 5, 4), sr.SETS["outlet_hi_x"])
    g = case.grid()
    st = sr.random_state(g, 2)
    zeroV = [np.zeros(nf) for nf in g.nface]
    N = g.ncell
    so = case.oracle()
    so.step, so.t = 0, sr.T0
    m0 = so.form_function(st["v"], zeroV, st["p"], scale=False)[0]
    so.step, so.t, so.phalf = 3, sr.T0, st["phalf"]
    m3 = so.form_function(st["v"], zeroV, st["p"], scale=False)[0]
    G0, Gh = np.concatenate(g.apply_G(st["p"])), np.concatenate(g.apply_G(st["phalf"]))
    d = (m0 - m3) - (Gh - G0)            # what is left: cg (p_out(t - dt/2) - p_out(t)) in the outlet layer of the x component
    lay = so._layer(d[:N].reshape(so.cshape), 0, -1)
    xc, xf, n = _centres(g)[0], g.xf[0], g.n[0]
    h1, h2 = xf[n] - xc[n - 1], xc[n - 1] - xc[n - 2]
    cg = h2 / (h1 * (h1 + h2))
    dp = so._outlet(1, sr.T0 - 0.5 * sr.DT) - so._outlet(1, sr.T0)
    assert np.abs(dp).min() > 1e-4
    assert np.allclose(lay, cg * dp, rtol=1e-9, atol=1e-12 * np.abs(m0).max())
    rest = d.copy().reshape(3, *so.cshape)
    rest[0][..., -1] = 0.0
    assert np.abs(rest).max() <= 1e-13 * np.abs(m0).max()
