"""CPU reference of the implicit scalar diffusion (include/fluca_hip_implicit.h), built on tests/scalar_reference.py (sr): the operator
D(phi) = sr.rhs with V = 0, Gamma = 1, q = 0 and its operation-count bound; the same operator line by line (D_lines: fast enough for a Chebyshev
recurrence on a few hundred thousand cells, and held to sr.rhs by tests/test_scalar_implicit_host.py); the assembled I - c L (sparse) and d_bc;
omega, S, the Gershgorin interval, the step count and B_k; the Chebyshev recurrence in any number type (np.float64: the product's arithmetic,
np.longdouble: its exact twin); and the IMEX step -- explicit part by sr.step with Gamma = 0, implicit part by a sparse direct solve, refined in
long double.

Arrays as in sr: phi[k, j, i]; grid axis d is numpy axis 2 - d."""
import copy

import numpy as np

from tests import scalar_reference as sr

U = sr.U


def grid_problem(n, uniform, bcname, short_periodic=False, gamma=0.0, homogeneous_neumann=False):
    """The problem of tests/scalar_cases.py on n cells; an axis of one or two cells is uniform also on the stretched grid (the stretching needs
    three cells).  short_periodic: the axes of one or two cells are periodic whatever the set says.  homogeneous_neumann: the Neumann values are 0."""
    from tests import scalar_cases as sc
    kinds, vals = sc.BC_SETS[bcname]
    kinds, vals = list(kinds), list(vals)
    for d in range(3):
        if short_periodic and n[d] <= 2:
            kinds[2 * d] = kinds[2 * d + 1] = sr.PERIODIC
            vals[2 * d] = vals[2 * d + 1] = 0.0
    if homogeneous_neumann:
        vals = [0.0 if k == sr.NEUMANN else v for k, v in zip(kinds, vals)]
    xu = sc.faces(n, True)
    xf = xu if uniform else [xu[d] if n[d] <= 2 else a for d, a in enumerate(sc.faces(tuple(max(m, 3) for m in n), False))]
    return sr.Problem(xf, kinds, vals, gamma=gamma)


def with_gamma(P, gamma):
    Q = copy.copy(P)
    Q.gamma = float(gamma)
    return Q


def zero_velocity(P):
    return [np.zeros(s) for s in P.shapes()[1]]


def D(P, phi, dtype=np.float64, bounds=False):
    """D(phi) = sr.rhs with V = 0, Gamma = 1, q = 0.  bounds: -> (D, E), E U bounding the rounding error of a binary64 evaluation, cell by cell."""
    with np.errstate(invalid="ignore", divide="ignore"):      # (an axis of one cell between two boundaries: sr divides by the distance of two mirrored centres it never uses)
        out = sr.rhs(with_gamma(P, 1.0), phi, zero_velocity(P), None, dtype, bounds=bounds)
    return (out[0], out[1]) if bounds else out


def apply_bound(c, phi, Dv, E):
    """|binary64 phi - c D(phi) - exact| <= this U: D's own error times c, the product c D (one rounding on |c D|) and the difference (one on
    |phi - c D| <= |phi| + |c D|); a fused multiply-add drops the product's rounding, another order of the three axes is inside E."""
    return abs(c) * np.asarray(E, dtype=np.float64) + 2 * abs(c) * np.abs(np.asarray(Dv, dtype=np.float64)) + np.abs(np.asarray(phi, dtype=np.float64))


# ---- the 1-D rows ---------------------------------------------------------------------------------------------------------------------------------

def axis_rows(P, d, dtype=np.float64):
    """-> ic[f] (f = 0 .. n: 1 / distance across face f, a boundary face: centre -- face; a periodic axis: ic[n] = ic[0]), ih[a] = 1 / width"""
    xf, xc, n = P.xf[d].astype(dtype), P.xc[d].astype(dtype), P.n[d]
    inner = list(xc[1:] - xc[:-1])
    if P.periodic(d):
        seam = xc[0] - (xc[n - 1] - (xf[n] - xf[0]))      # the last centre a period BACK, as sr.axis_terms: forward, the sum would round at the size of the period
        dist = [seam] + inner + [seam]
    else:
        dist = [xc[0] - xf[0]] + inner + [xf[n] - xc[n - 1]]
    one = dtype(1)
    return np.array([one / x for x in dist], dtype=dtype), np.array([one / x for x in (xf[1:] - xf[:-1])], dtype=dtype)


def faces_with_partner(P, d):
    """-> (lo[a], hi[a]): does the face a / a + 1 of cell a have a CELL on the other side (interior, or periodic with more than one cell)"""
    n = P.n[d]
    if P.periodic(d):
        return np.full(n, n > 1), np.full(n, n > 1)
    a = np.arange(n)
    return a > 0, a < n - 1


def D_lines(P, phi, dtype=np.float64):
    """D(phi) by the operations the kernel performs: G = (difference) * ic, (G2 - G1) * ih, the axes added x, y, z"""
    ph = np.asarray(phi, dtype=dtype).reshape(P.shapes()[0])
    out = np.zeros_like(ph)
    for d in range(3):
        n, per = P.n[d], P.periodic(d)
        ic, ih = axis_rows(P, d, dtype)
        a = np.moveaxis(ph, 2 - d, 0)
        col = lambda v: v.reshape((-1,) + (1,) * 2)
        G = np.empty((n + 1,) + a.shape[1:], dtype=dtype)
        G[1:n] = (a[1:] - a[:-1]) * col(ic[1:n])
        if per:
            G[0] = (a[0] - a[n - 1]) * ic[0]
            G[n] = G[0]
        else:
            klo, khi, vlo, vhi = P.bc[2 * d], P.bc[2 * d + 1], dtype(P.val[2 * d]), dtype(P.val[2 * d + 1])
            G[0] = (a[0] - vlo) * ic[0] if klo == sr.DIRICHLET else vlo
            G[n] = (vhi - a[n - 1]) * ic[n] if khi == sr.DIRICHLET else vhi
        out = out + np.moveaxis((G[1:] - G[:-1]) * col(ih), 0, 2 - d)
    return out


def omega_max(P, d):
    """max_i omega_d(i): the off-diagonal magnitudes of row i of axis d per unit c, in the product's arithmetic"""
    ic, ih = axis_rows(P, d)
    lo, hi = faces_with_partner(P, d)
    return float(np.max((np.where(lo, ic[:-1], 0.0) + np.where(hi, ic[1:], 0.0)) * ih))


def S_of(P, c):
    return c * ((omega_max(P, 0) + omega_max(P, 1)) + omega_max(P, 2))


def interval(P, c):
    S = S_of(P, c)
    return 1.0 / (1.0 + S), (1.0 + 2.0 * S) / (1.0 + S)


def c_for_S(P, S):
    return S / S_of(P, 1.0)


def bound(emin, emax, k):
    """B_k = 2 s^k / (1 + s^2k), k even: s^k by repeated products with s^2, as fl_scalar_cheb_steps forms it"""
    sk = np.sqrt(emax / emin)
    sigma = (sk - 1.0) / (sk + 1.0)
    s2, pw = sigma * sigma, 1.0
    for _ in range(k // 2):
        pw *= s2
    return 2.0 * pw / (1.0 + pw * pw) if k else 1.0


def steps(emin, emax, rtol, maxit):
    """-> (k, B_k): the smallest even k with B_k <= rtol, capped at maxit rounded down to even"""
    cap = maxit - maxit % 2
    k = 0
    while bound(emin, emax, k) > rtol and k < cap:
        k += 2
    return k, bound(emin, emax, k)


# ---- the matrix -------------------------------------------------------------------------------------------------------------------------------------

def axis_matrix(P, d):
    """-> (L_d (n x n, dense), dbc_d (n)): the part of D along axis d, D_d(phi) = L_d phi + dbc_d on a line"""
    n, per = P.n[d], P.periodic(d)
    ic, ih = axis_rows(P, d)
    L, dbc = np.zeros((n, n)), np.zeros(n)
    lo, hi = faces_with_partner(P, d)
    for a in range(n):
        for side, f, nb, has in ((0, a, (a - 1) % n, lo[a]), (1, a + 1, (a + 1) % n, hi[a])):
            w = ic[f] * ih[a]
            if has:
                L[a, a] -= w
                L[a, nb] += w
            elif not per:
                kind, val = P.bc[2 * d + side], P.val[2 * d + side]
                if kind == sr.DIRICHLET:
                    L[a, a] -= w
                    dbc[a] += w * val
                else:                                   # Neumann: the gradient of the face is the value, along the +axis
                    dbc[a] += (val if side else -val) * ih[a]
    return L, dbc


def assemble(P, c):
    """-> (A = I - c L (scipy CSR, cells flattened as phi[k, j, i]), d_bc (flat), diag(A) as a field)"""
    import scipy.sparse as sp
    nx, ny, nz = P.n
    (Lx, bx), (Ly, by), (Lz, bz) = (axis_matrix(P, d) for d in range(3))
    I = lambda n: sp.identity(n, format="csr")
    L = sp.kron(I(nz), sp.kron(I(ny), sp.csr_matrix(Lx))) + sp.kron(I(nz), sp.kron(sp.csr_matrix(Ly), I(nx))) + sp.kron(sp.csr_matrix(Lz), I(ny * nx))
    dbc = bx[None, None, :] + by[None, :, None] + bz[:, None, None]
    A = (sp.identity(nx * ny * nz, format="csr") - c * L).tocsr()
    return A, dbc.reshape(-1), np.asarray(A.diagonal()).reshape(nz, ny, nx)


def diagonal(P, c, dtype=np.float64):
    """diag(I - c L) as a field, from the rows (the kernel's sum: 1 + c (dg_x + dg_y + dg_z), dg_d = (w1 + w2) ih)"""
    dg = []
    for d in range(3):
        ic, ih = axis_rows(P, d, dtype)
        lo, hi = faces_with_partner(P, d)
        if not P.periodic(d):
            lo, hi = lo.copy(), hi.copy()
            lo[0] = P.bc[2 * d] == sr.DIRICHLET
            hi[-1] = P.bc[2 * d + 1] == sr.DIRICHLET
        dg.append((np.where(lo, ic[:-1], dtype(0)) + np.where(hi, ic[1:], dtype(0))) * ih)
    return dtype(1) + dtype(c) * ((dg[0][None, None, :] + dg[1][None, :, None]) + dg[2][:, None, None])


def weights(P, c):
    """vol_c diag(A)_c: the weights of the norm in which k Chebyshev steps reduce the error by B_k"""
    return sr.volumes(P) * diagonal(P, c)


def wnorm(w, e):
    return float(np.sqrt((np.asarray(w, dtype=np.longdouble) * np.asarray(e, dtype=np.longdouble) ** 2).sum()))


def solve_exact(P, c, b, refine=2):
    """x with x - c D(x) = b: sparse direct in binary64, then `refine` corrections with the residual formed in long double -> long double field"""
    import scipy.sparse.linalg as spl
    A, dbc, _ = assemble(P, c)
    lu = spl.splu(A.tocsc())
    bb = np.asarray(b, dtype=np.longdouble).reshape(P.shapes()[0])
    x = lu.solve((np.asarray(b, dtype=np.float64).reshape(-1) + c * dbc)).reshape(bb.shape).astype(np.longdouble)
    for _ in range(refine):
        r = bb - (x - np.longdouble(c) * D_lines(P, x, np.longdouble))
        x = x + lu.solve(r.astype(np.float64).reshape(-1)).reshape(bb.shape)
    return x


# ---- the Chebyshev recurrence -------------------------------------------------------------------------------------------------------------------------

def coefficients(emin, emax, k):
    """(p_j, q_j), j = 1 .. k, of d_j = p_j d_{j-1} + q_j z_j (Saad, Algorithm 12.1), in binary64 as the host forms them"""
    theta, delta = 0.5 * (emax + emin), 0.5 * (emax - emin)
    sigma1 = theta / delta
    rho = 1.0 / sigma1
    out = [(0.0, 1.0 / theta)]
    for _ in range(1, k):
        rho_new = 1.0 / (2.0 * sigma1 - rho)
        out.append((rho_new * rho, 2.0 * rho_new / delta))
        rho = rho_new
    return out[:k]


def chebyshev(P, c, b, x0, k, dtype=np.float64, every=False, emin=None, emax=None):
    """k steps  r = b - H_c(x); d = p d + q r / diag; x = x + d  from x0 -> x_k (every: the list x_0 .. x_k)"""
    if emin is None:
        emin, emax = interval(P, c)
    shape = P.shapes()[0]
    x, bb = np.asarray(x0, dtype=dtype).reshape(shape), np.asarray(b, dtype=dtype).reshape(shape)
    dg, cc = diagonal(P, c, dtype), dtype(c)
    d, xs = None, [x]
    for p, q in coefficients(emin, emax, k):
        r = bb - (x - cc * D_lines(P, x, dtype))
        dn = dtype(q) * (r / dg)
        d = dn if d is None else dn + dtype(p) * d
        x = x + d
        xs.append(x)
    return xs if every else x


# ---- the IMEX step ------------------------------------------------------------------------------------------------------------------------------------

def imex_step(P, phi, V, dt, s, theta, q=None, bounds=False):
    """phi^{n+1} of fl_scalar_step_imex with an EXACT solve (long double field), P.gamma the diffusivity.
    -> (phi_new, phi_star, b) or, with bounds, (phi_new, phi_star, b, Bx): Bx(c) bounds the error of a binary64 evaluation of b (sr.step's derived
    bound of the explicit part; for theta < 1 the roundings of the explicit diffusion share and of the sum)."""
    P0 = with_gamma(P, 0.0)
    ld = np.longdouble
    if bounds:
        star, Bx = sr.step(P0, phi, V, dt, s, q, ld, bounds=True)
    else:
        star, Bx = sr.step(P0, phi, V, dt, s, q, ld), None
    c, ce = theta * dt * P.gamma, (1.0 - theta) * dt * P.gamma
    b = star
    if ce != 0.0:
        Dn, E = D(P, phi, ld, bounds=True)
        b = star + ld(ce) * Dn
        if bounds:      # D's error times ce, the product, the sum
            Bx = Bx + U * (ce * E + np.abs(ce * Dn) + np.abs(b)).astype(np.float64)
    new = solve_exact(P, c, b) if c != 0.0 else b
    return (new, star, b, Bx) if bounds else (new, star, b)
