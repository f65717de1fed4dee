"""CPU reference of the passive scalar transport (include/fluca_hip.h, fl_scalar_*), numpy, written from the scheme's definition and not from
the kernel: the limited second-order TVD face value of FlucaFDSecondOrderTVD, the right-hand side R, the s-stage second-order SSP Runge-Kutta
step (PETSc's -ts_type ssp, rks2) and the cfl / stats quantities, line by line along an axis: every quantity of a face is an array over the
faces of the axis (and over the other two axes), built from the cells -2 .. n+1 of the lines.

Arrays: phi[k, j, i] (nz, ny, nx); V = (Vx[k, j, fx], Vy[k, fy, i], Vz[fz, j, i]) with n faces on a periodic axis and n + 1 otherwise -- the
layouts of fl_poisson_rhs reshaped.  Grid axis d is numpy axis 2 - d.

Every function takes the number type: np.float64 restates the scheme in the product's precision, np.longdouble (64-bit mantissa on x86) serves
as the exact value the rounding-level bounds of the GPU tests are measured against.  rhs() also returns those bounds (see rhs).

reference_ghost: the reference's raw stencil reads, at an OUTFLOW boundary face, the cell beyond the boundary from a local vector whose ghost is
never filled -- zero.  With the switch on, that is restated (all six ex7 goldens are reproduced); off -- the default, and what the product
does -- a boundary face carries the boundary's own value for either flow direction.
"""
import numpy as np

DIRICHLET, NEUMANN, PERIODIC = 0, 1, 2
LIMITERS = ("superbee", "minmod", "mc", "vanleer", "vanalbada", "barthjesperson", "venkatakrishnan", "koren", "upwind", "sou", "quick")
BOUNDED = LIMITERS[:9]          # superbee .. koren and upwind: TVD
U = 2.0 ** -53                  # unit roundoff of binary64


def psi(limiter, r):
    """secondordertvdlimiter.c, operation by operation (PetscMin / PetscMax are comparisons)."""
    name = LIMITERS[limiter] if isinstance(limiter, (int, np.integer)) else limiter
    r = np.asarray(r)
    one = r.dtype.type(1)
    mn = lambda a, b: np.where(a < b, a, b)
    mx = lambda a, b: np.where(a < b, b, a)
    with np.errstate(all="ignore"):
        if name == "superbee":
            return mx(0 * one, mx(mn(2 * r, one), mn(r, 2 * one)))
        if name == "minmod":
            return mx(0 * one, mn(r, one))
        if name == "mc":
            return mx(0 * one, mn(mn(2 * r, (1 + r) / 2), 2 * one))
        if name == "vanleer":
            a = np.abs(r)
            return (r + a) / (1 + a)
        if name == "vanalbada":
            return np.where(r <= 0, 0 * one, (r * r + r) / (r * r + 1))
        if name == "barthjesperson":
            a, b = 4 * r / (1 + r), 4 / (1 + r)
            return np.where(r <= 0, 0 * one, (1 + r) / 2 * mn(one, mn(a, b)))
        if name == "venkatakrishnan":
            a = 4 * r * (3 * r + 1) / (11 * r * r + 4 * r + 1)
            b = 4 * (r + 3) / (r * r + 4 * r + 11)
            return np.where(r <= 0, 0 * one, (1 + r) / 2 * mn(a, b))
        if name == "koren":
            return mx(0 * one, mn(mn(2 * r, (1 + 2 * r) / 3), 2 * one))
        if name == "upwind":
            return 0 * r
        if name == "sou":
            return r + 0
        if name == "quick":
            return (3 + r) / 4
    raise ValueError(name)


# Rounded operations of each limiter (counted in psi above; comparisons, selections, |.|, and products with 2 or 4 or quotients by 2 or 4 are
# exact) and a Lipschitz constant of each (sup |psi'|; tests/test_scalar_reference.py checks them against difference quotients).
PSI_OPS = dict(superbee=0, minmod=0, mc=1, vanleer=3, vanalbada=5, barthjesperson=4, venkatakrishnan=16, koren=2, upwind=0, sou=0, quick=1)
PSI_LIP = dict(superbee=2.0, minmod=1.0, mc=2.0, vanleer=2.0, vanalbada=1.3, barthjesperson=2.0, venkatakrishnan=2.0, koren=2.0, upwind=0.0, sou=1.0, quick=0.25)


def psi_rslope(limiter, r):
    """|psi'(r) r|, the sensitivity of psi to a RELATIVE change of r, as the larger one-sided difference quotient over a relative step of 1e-6
    (a kink closer than that counts with its steeper side).  Bounded for the bounded limiters (<= 2), where sup |psi'| |r| is not."""
    name = LIMITERS[limiter] if isinstance(limiter, (int, np.integer)) else limiter
    r = np.asarray(r)
    d = r.dtype.type(1e-6)
    p = psi(name, r)
    return np.maximum(np.abs(psi(name, r * (1 + d)) - p), np.abs(psi(name, r * (1 - d)) - p)) / d


def psi_intermediate(limiter, r):
    """the largest magnitude among the intermediates of psi(r): one ulp of it per rounded operation bounds the rounding error of psi"""
    name = LIMITERS[limiter] if isinstance(limiter, (int, np.integer)) else limiter
    a = np.abs(np.asarray(r, dtype=np.float64))
    with np.errstate(all="ignore"):
        big = {"mc": (1 + a) / 2, "vanleer": np.maximum(2 * a, 1.0) , "vanalbada": a * a + a + 1, "barthjesperson": np.maximum(4.0, 1 + a) * 1.0,
               "venkatakrishnan": np.maximum(12 * a * a + 4 * a + 11, 4 * (a + 3)), "koren": (1 + 2 * a) / 3, "quick": (3 + a) / 4}.get(name)
    return np.zeros_like(a) if big is None else np.maximum(big, np.abs(psi(name, np.asarray(r, dtype=np.float64))))


class Problem:
    """grid (face coordinates xf[d], centres xc[d] or midpoints), boundary kinds bc[6] and values val[6], Gamma, limiter"""

    def __init__(self, xf, bc, val=(0,) * 6, gamma=0.0, limiter=0, xc=None):
        self.xf = [np.asarray(a, dtype=np.float64) for a in xf]
        self.n = tuple(len(a) - 1 for a in self.xf)
        self.xc = [(self.xf[d][:-1] + self.xf[d][1:]) / 2 if xc is None or xc[d] is None else np.asarray(xc[d], dtype=np.float64) for d in range(3)]
        self.bc, self.val = tuple(bc), tuple(float(v) for v in val)
        self.gamma, self.limiter = float(gamma), LIMITERS[limiter] if isinstance(limiter, (int, np.integer)) else limiter
        for d in range(3):
            assert (bc[2 * d] == PERIODIC) == (bc[2 * d + 1] == PERIODIC)

    def periodic(self, d):
        return self.bc[2 * d] == PERIODIC

    def nfaces(self, d):
        return self.n[d] if self.periodic(d) else self.n[d] + 1

    def shapes(self):
        nx, ny, nz = self.n
        return (nz, ny, nx), [(nz, ny, self.nfaces(0)), (nz, self.nfaces(1), nx), (self.nfaces(2), ny, nx)]

    def widths(self, d, dtype=np.float64):
        xf = self.xf[d].astype(dtype)
        return xf[1:] - xf[:-1]


def axis_terms(P, phi, V, d, dtype=np.float64, reference_ghost=False, limiter=None):
    """Along axis d, with the axis moved to the front: F[f], G[f] (face value and two-point gradient, f = 0 .. n, face n of a periodic axis
    being face 0 again), eF[f], eG[f] (bounds on the rounding error of a binary64 evaluation of them, in units of U, see rhs) and LF[f] (how
    much F can move per unit of sup-norm change of phi), V[f]."""
    name = P.limiter if limiter is None else limiter
    n, per = P.n[d], P.periodic(d)
    ph = np.moveaxis(np.asarray(phi, dtype=dtype), 2 - d, 0)
    Vd = np.moveaxis(np.asarray(V, dtype=dtype), 2 - d, 0)
    xf, xc = P.xf[d].astype(dtype), P.xc[d].astype(dtype)
    L = xf[n] - xf[0]
    klo, khi, vlo, vhi = P.bc[2 * d], P.bc[2 * d + 1], dtype(P.val[2 * d]), dtype(P.val[2 * d + 1])
    col = lambda a: a.reshape((-1,) + (1,) * (ph.ndim - 1))       # a 1-D array of the axis against the fields
    # the cells -2 .. n+1 (index + 2) and their centres: periodic images, or -- beyond a boundary -- 0 at a mirrored centre (what the reference's
    # unfilled ghost holds: read by reference_ghost only; the product's boundary rule replaces every use of them below)
    idx = np.arange(-2, n + 2)
    if per:
        # a face's distances are those of its image among the faces 0 .. n-1; the centre before face 0 is the last one, a period back
        # (xc[n-1] - L: the difference of two close numbers, exact -- an image shifted FORWARD, xc[0] + L, would round at the size of L and
        # spoil a small distance at the seam)
        E = ph[idx % n]
        before = np.concatenate([[xc[n - 1] - L], xc[:n - 1]])
        fb = np.arange(-1, n + 2) % n
        dcx = (xc - before)[fb]
        apn, amn = (xf[:n] - before)[fb[1:n + 2]], (xc - xf[:n])[fb[1:n + 2]]
    else:
        E = np.zeros((n + 4,) + ph.shape[1:], dtype=dtype)
        E[2:n + 2] = ph
        xce = np.concatenate([[2 * xf[0] - xc[1 % n], 2 * xf[0] - xc[0]], xc, [2 * xf[n] - xc[n - 1], 2 * xf[n] - xc[n - 2 if n > 1 else 0]]]).astype(dtype)
        dcx = xce[1:] - xce[:-1]
        apn, amn = xf - xce[1:n + 2], xce[2:n + 3] - xf
    # the gradients of the faces -1 .. n+1 (index + 1): face f lies between the cells f-1 and f
    Gx = (E[1:] - E[:-1]) / col(dcx)
    eGx = 4 * np.abs(Gx)            # the difference, the distance, its reciprocal (a table), the product: four roundings
    if not per:
        if klo == DIRICHLET:
            Gx[1] = (ph[0] - vlo) / (xc[0] - xf[0])
            eGx[1] = 4 * np.abs(Gx[1])
        else:
            Gx[1], eGx[1] = vlo, 0
        if khi == DIRICHLET:
            Gx[n + 1] = (vhi - ph[n - 1]) / (xf[n] - xc[n - 1])
            eGx[n + 1] = 4 * np.abs(Gx[n + 1])
        else:
            Gx[n + 1], eGx[n + 1] = vhi, 0
        Gx[0] = Gx[n + 2] = eGx[0] = eGx[n + 2] = 0
    Vf = Vd[np.arange(n + 1) % n] if per else Vd
    up = Vf > 0
    cm, cp = E[1:n + 2], E[2:n + 3]                       # the cells f-1 and f of the faces f = 0 .. n
    pu, pd = np.where(up, cm, cp), np.where(up, cp, cm)
    gc, gu = Gx[1:n + 2], np.where(up, Gx[0:n + 1], Gx[2:n + 3])
    e_gc, e_gu = eGx[1:n + 2], np.where(up, eGx[0:n + 1], eGx[2:n + 3])
    dc = col(dcx[1:n + 2])
    al = np.where(up, col(apn) / dc, col(amn) / dc)
    lip = PSI_LIP[name]
    with np.errstate(all="ignore"):
        guard = np.abs(gc) > 1e-30
        r = np.where(guard, gu / np.where(guard, gc, 1), dtype(1))
        ps = psi(name, r)
        F = pu + al * ps * (pd - pu)
        # rounding: r carries the relative errors of both gradients and of the quotient; psi that of r through |psi'(r) r| plus its own
        # operations; alpha (a table: difference, distance, quotient) 3, the two products and the difference 3; the final sum 1
        rel = lambda e, g: np.where(np.abs(g) > 0, e / np.where(np.abs(g) > 0, np.abs(g), 1), 0)
        rs = psi_rslope(name, r)
        e_ps = np.where(guard, rs * (rel(e_gu, gu) + rel(e_gc, gc) + 1), 0) + PSI_OPS[name] * psi_intermediate(name, r).astype(dtype)
        eF = np.abs(pd - pu) * np.abs(al) * (e_ps + 6 * np.abs(ps)) + np.abs(F)
        # sensitivity to phi (sup norm eps): pu, pd move by eps, pd - pu by 2 eps, either gradient by 2 eps / distance, r by (|dgu| + |r| |dgc|) / |gc|,
        # and |pd - pu| = |gc| dc, so |psi'| |dr| |pd - pu| <= 2 eps dc (|psi'| / dc_u + |psi' r| / dc) <= 2 eps (sup |psi'| dcmax / dcmin + |psi'(r) r|)
        LF = 1 + np.abs(al) * (2 * np.abs(ps) + 2 * (lip * _spacing_ratio(P, d) + rs))
    if not per:
        for f, kind, val, near, dist, sgn in ((0, klo, vlo, ph[0], xc[0] - xf[0], -1), (n, khi, vhi, ph[n - 1], xf[n] - xc[n - 1], 1)):
            # a boundary face carries the boundary's own value; reference_ghost: only on the inflow side
            if kind == DIRICHLET:
                own, e_own, l_own = val + 0 * near, 0 * near, 0 * near
            else:
                own = near + sgn * dist * val
                e_own, l_own = 2 * np.abs(dist * val) + np.abs(own), 1 + 0 * near
            if reference_ghost:
                out = up[f] if f == n else ~up[f]
                F[f], eF[f], LF[f] = np.where(out, F[f], own), np.where(out, eF[f], e_own), np.where(out, LF[f], l_own)
            else:
                F[f], eF[f], LF[f] = own, e_own, l_own
    return dict(F=F, G=Gx[1:n + 2], eF=eF, eG=eGx[1:n + 2], LF=LF, V=Vf)


def _spacing_ratio(P, d):
    xc, xf, n = P.xc[d], P.xf[d], P.n[d]
    dc = list(np.diff(xc))
    if P.periodic(d):
        dc.append(xc[0] + (xf[n] - xf[0]) - xc[n - 1])
    else:
        dc += [xc[0] - xf[0], xf[n] - xc[n - 1]]
    return max(dc) / min(dc)


def rhs(P, phi, V, q=None, dtype=np.float64, reference_ghost=False, bounds=False, limiter=None):
    """R(phi) (nz, ny, nx).  bounds=True: -> (R, E, A): E(c) U bounds the difference between a binary64 evaluation of R(c) -- in any order of
    the sums, with or without fused multiply-adds, with tabulated reciprocals of the distances -- and the exact value, to first order in U: every
    rounded operation contributes one U times the magnitude of its result, followed through the formula (the face value's part is in axis_terms);
    A(c): |R(phi + d)(c) - R(phi)(c)| <= A(c) max|d|."""
    R = np.zeros(P.shapes()[0], dtype=dtype)
    E = np.zeros_like(R)
    A = np.zeros_like(R)
    S = np.zeros_like(R)        # sum of the magnitudes of the three axis terms (and q): the sums over them round three times
    gam = dtype(P.gamma)
    for d in range(3):
        t = axis_terms(P, phi, V[d], d, dtype, reference_ghost, limiter)
        n = P.n[d]
        h = P.widths(d, dtype).reshape((n,) + (1,) * 2)
        ic = np.array([abs(1 / dtype(x)) for x in _face_distances(P, d)], dtype=dtype).reshape((n + 1,) + (1,) * 2)
        F0, F1, G0, G1, V0, V1 = t["F"][:-1], t["F"][1:], t["G"][:-1], t["G"][1:], t["V"][:-1], t["V"][1:]    # the faces a and a+1 of the cells a
        back = lambda x: np.moveaxis(x, 0, 2 - d)
        term = (gam * (G1 - G0) - (V1 * F1 - V0 * F0)) / h
        R += back(term)
        if bounds:
            mag = gam * (np.abs(G1) + np.abs(G0)) + np.abs(V1 * F1) + np.abs(V0 * F0)
            # the gradients' and face values' own errors; then: products 1, inner difference 1, outer difference 1, 1 / h (difference, reciprocal) 2,
            # the last product 1 -- six roundings on the magnitudes
            E += back((gam * (t["eG"][1:] + t["eG"][:-1]) + np.abs(V1) * t["eF"][1:] + np.abs(V0) * t["eF"][:-1] + 6 * mag) / h)
            S += back(np.abs(term))
            A += back((np.abs(V1) * t["LF"][1:] + np.abs(V0) * t["LF"][:-1] + gam * 2 * (ic[1:] + ic[:-1])) / h)
    if q is not None:
        qq = np.asarray(q, dtype=dtype).reshape(R.shape)
        R += qq
        S += np.abs(qq)
    if bounds:
        return R, E + 3 * S, A
    return R


def _face_distances(P, d):
    """distance between the centres either side of face f = 0 .. n (a boundary face: centre -- face)"""
    xc, xf, n = P.xc[d], P.xf[d], P.n[d]
    inner = list(np.diff(xc))
    if P.periodic(d):
        seam = xc[0] + (xf[n] - xf[0]) - xc[n - 1]
        return [seam] + inner + [seam]
    return [xc[0] - xf[0]] + inner + [xf[n] - xc[n - 1]]


def stage(P, c0, c1, c2, phin, w, V, q=None, dtype=np.float64, bounds=False, eps_in=0.0, **kw):
    """out = c0 phin + c1 w + c2 R(w).  bounds: -> (out, B) with |binary64 stage on a w that is off by at most eps_in - out| <= B (absolute)."""
    if not bounds:
        return dtype(c0) * np.asarray(phin, dtype=dtype) + dtype(c1) * np.asarray(w, dtype=dtype) + dtype(c2) * rhs(P, w, V, q, dtype, **kw)
    R, E, A = rhs(P, w, V, q, dtype, bounds=True, **kw)
    t0, t1, t2 = dtype(c0) * np.asarray(phin, dtype=dtype), dtype(c1) * np.asarray(w, dtype=dtype), dtype(c2) * R
    out = t0 + t1 + t2
    # the coefficients are rounded quotients (2), the products 1, the two sums 2: five on each magnitude is generous
    B = U * (abs(c2) * E + 5 * (np.abs(t0) + np.abs(t1) + np.abs(t2))) + (abs(c1) + abs(c2) * A) * eps_in
    return out, B


def step(P, phi, V, dt, s, q=None, dtype=np.float64, bounds=False, eps_in=0.0, **kw):
    """one rks2 step: w = phi; s - 1 times w += dt / (s - 1) R(w); phi' = ((s - 1) w + phi + dt R(w)) / s.
    bounds: -> (phi', B), B(c) bounding |binary64 step started from a phi that is off by at most eps_in - phi'| (stage bounds carried forward
    through A)."""
    ph = np.asarray(phi, dtype=dtype)
    w, eps, B = ph, eps_in, None
    for _ in range(s - 1):
        if bounds:
            w, B = stage(P, 0, 1, dt / (s - 1), 0 * ph, w, V, q, dtype, True, eps, **kw)
            eps = float(B.max())
        else:
            w = w + dtype(dt) / (s - 1) * rhs(P, w, V, q, dtype, **kw)
    if bounds:
        out, B = stage(P, 1 / s, (s - 1) / s, dt / s, ph, w, V, q, dtype, True, eps, **kw)
        return out, B + eps_in / s
    return ((s - 1) * w + ph + dtype(dt) * rhs(P, w, V, q, dtype, **kw)) / s


def cfl(P, V, dt, dtype=np.float64):
    """(max_c dt sum_d max(|V(f-)|, |V(f+)|) / h_d, max_c Gamma dt sum_d 2 / h_d^2), the sums in the order x, y, z"""
    adv = np.zeros(P.shapes()[0], dtype=dtype)
    dif = np.zeros_like(adv)
    for d in range(3):
        n, per = P.n[d], P.periodic(d)
        Vd = np.abs(np.moveaxis(np.asarray(V[d], dtype=dtype), 2 - d, 0))
        lo = Vd[:n]
        hi = np.concatenate([Vd[1:n], Vd[:1]]) if per else Vd[1:n + 1]
        h = P.widths(d, dtype).reshape((n, 1, 1))
        adv += np.moveaxis(np.maximum(lo, hi) / h, 0, 2 - d)
        dif += np.moveaxis(np.broadcast_to(2 / (h * h), lo.shape), 0, 2 - d)
    return float((dtype(dt) * adv).max()), float((dtype(P.gamma) * dtype(dt) * dif).max())


def volumes(P, dtype=np.float64):
    hx, hy, hz = (P.widths(d, dtype) for d in range(3))
    return (hx[None, None, :] * hy[None, :, None]) * hz[:, None, None]


def stats(P, phi, dtype=np.float64):
    ph = np.asarray(phi, dtype=dtype).reshape(P.shapes()[0])
    return float(ph.min()), float(ph.max()), (ph * volumes(P, dtype)).sum()


# ---- the reference's stencil text (fluca/tests/fd/ex7.c): 1-D line, element values -> the face value at face i

def ex7_text(limiter, i, left="dirichlet", right="dirichlet", drop_zero_constant=True):
    """stdout of ex7 -i <i> -flucafd_limiter <limiter> -flucafd_left_bc_type / -flucafd_right_bc_type: eight cells on [0, 1], phi = sin(pi x / 2),
    V = 1, boundary values 0 / 1 (Dirichlet) and pi / 2 / 0 (Neumann), as the reference prints the stencil FlucaFDGetStencil returns: the upwind
    cell with coefficient 1, the boundary's column where the ghost elimination leaves one, and the limited correction as a constant.
    drop_zero_constant=False keeps the constant column FlucaFD drops when it is zero."""
    from tests.flucafd_golden import fmt_g
    n = 8
    xf = np.linspace(0.0, 1.0, n + 1)
    xc = (np.arange(n) + 0.5) / n
    phi = np.sin(np.pi * xc / 2)
    kinds = dict(dirichlet=DIRICHLET, neumann=NEUMANN)
    bc = (kinds[left], kinds[right], PERIODIC, PERIODIC, PERIODIC, PERIODIC)
    val = (0.0 if left == "dirichlet" else np.pi / 2, 1.0 if right == "dirichlet" else 0.0, 0, 0, 0, 0)
    P = Problem([xf, np.array([0.0, 1.0]), np.array([0.0, 1.0])], bc, val, limiter=limiter)
    t = axis_terms(P, phi.reshape(1, 1, n), np.ones((1, 1, n + 1)), 0, reference_ghost=True)
    rows = []
    if i == 0:
        # V > 0 at the low boundary: the ghost cell is eliminated -- Dirichlet leaves the boundary's column alone, Neumann the first cell and the boundary
        if left == "dirichlet":
            rows.append("i=0, loc=LEFT, c=left_boundary, v=%s" % fmt_g(1.0))
        else:
            rows.append("i=0, loc=ELEMENT, c=0, v=%s" % fmt_g(1.0))
            rows.append("i=0, loc=LEFT, c=left_boundary, v=%s" % fmt_g(-(xc[0] - xf[0])))
    else:
        rows.append("i=%d, loc=ELEMENT, c=0, v=%s" % (i - 1, fmt_g(1.0)))
        const = float(t["F"][i].reshape(-1)[0] - phi[i - 1])
        if const != 0.0 or not drop_zero_constant:
            rows.append("constant, v=%s" % fmt_g(const))
    lines = ["Stencil at i=%d:" % i, "  ncols = %d" % len(rows)] + ["  col[%d]: %s" % (c, r) for c, r in enumerate(rows)]
    return "\n".join(lines) + "\n"
