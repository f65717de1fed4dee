"""References of the Boussinesq coupling (fl_momentum_add_buoyancy, fl_scalar_boundary_flux, NSSetGravity ...), numpy, written from the definitions:

  term / add_fused    the buoyancy term dt sum_s a_s,d (phi_s - ref_s) in long double, its magnitude, and the bits of the kernel's documented operation
                      order (include/fluca_hip.h) restated with tests/step_rhs.fused
  wall_fluxes         the twelve boundary fluxes from scalar_reference.axis_terms -- F, G, V on the boundary faces f = 0 and f = n times the face
                      areas -- with the bounds of a binary64 evaluation
  BuoyantStep         StepOracle whose form_function adds the term to momrhs (step_once reaches it through self.form_function)
"""
import numpy as np

from oracle import fluca_oracle as fo
from tests import scalar_reference as sr
from tests import step_rhs as sh

U = sr.U


def term(phis, accel, refs, dt, dtype=np.longdouble):
    """-> (T, M), both (3, N): T[d] = dt sum_s accel[s][d] (phi_s - ref_s), M[d] = |dt| sum_s |accel[s][d]| |phi_s - ref_s|"""
    n = np.asarray(phis[0]).size
    T, M = np.zeros((3, n), dtype=dtype), np.zeros((3, n), dtype=dtype)
    for d in range(3):
        for s, phi in enumerate(phis):
            x = np.asarray(phi, dtype=dtype).ravel() - dtype(refs[s])
            T[d] += dtype(accel[s][d]) * x
            M[d] += abs(dtype(accel[s][d])) * np.abs(x)
    return dtype(dt) * T, abs(dtype(dt)) * M


def add_fused(momrhs, phis, accel, refs, dt):
    """the kernel's operation order in binary64: x_s = phi_s - ref_s; t = a_0 x_0; t = fma(a_s, x_s, t); out = fma(dt, t, momrhs).  A component
    whose coefficients are all zero is returned as it came."""
    n = np.asarray(phis[0]).size
    out = np.array(momrhs, dtype=np.float64).reshape(3, n).copy()
    for d in range(3):
        if all(accel[s][d] == 0.0 for s in range(len(phis))):
            continue
        t = None
        for s, phi in enumerate(phis):
            x = np.asarray(phi, dtype=np.float64).ravel() - np.float64(refs[s])
            t = np.float64(accel[s][d]) * x if t is None else sh.fused(accel[s][d], x, t)
        out[d] = sh.fused(dt, t, out[d])
    return out


def add_fused_exact(momrhs_d, phis, accel_d, refs, dt, cells):
    """the same chain for component d at the given cells with every fused multiply-add rounded ONCE, in rational arithmetic (step_rhs.fused goes
    through the 64-bit significand of the long double and is off by a double rounding about once in 2^11 operations).  -> float64 array"""
    from fractions import Fraction as Fr
    out = np.empty(len(cells))
    for k, c in enumerate(cells):
        t = None
        for s, phi in enumerate(phis):
            x = np.float64(np.asarray(phi).ravel()[c]) - np.float64(refs[s])
            t = np.float64(accel_d[s]) * x if t is None else float(Fr(float(accel_d[s])) * Fr(float(x)) + Fr(float(t)))
        r = Fr(float(dt)) * Fr(float(t)) + Fr(float(momrhs_d[c]))
        # (a zero result: +0 after an exact cancellation; with a zero product the sign IEEE gives the sum of the two zeros)
        out[k] = float(r) if r != 0 else (0.0 if t != 0 else float(np.float64(dt) * np.float64(t) + np.float64(momrhs_d[c])))
    return out


def areas(P, d, dtype=np.longdouble):
    """A of the faces across axis d, shaped like a slice axis_terms(...)[f] (the axis moved to the front and taken away)"""
    hx, hy, hz = (P.widths(a, dtype) for a in range(3))
    if d == 0:
        return hz[:, None] * hy[None, :]            # (nz, ny)
    if d == 1:
        return hz[:, None] * hx[None, :]            # (nz, nx)
    return hy[:, None] * hx[None, :]                # (ny, nx)


def wall_fluxes(P, phi, V, dtype=np.longdouble, limiter=None):
    """-> (flux, bound), both (6, 2): flux[b] = (sum V F A, sum -Gamma G A) over the faces of boundary b along the +axis (0, 0 at a periodic end);
    bound[b]: what a binary64 evaluation may differ by -- U sum_f (|V| eF A + 3 |V F A|) for the convective part (the products V F, the area, their
    product), the analogue with Gamma eG for the diffusive part, and (faces - 1) U sum_f |term| for a sum taken in any order."""
    flux = np.zeros((6, 2), dtype=dtype)
    bound = np.zeros((6, 2), dtype=np.float64)
    gam = dtype(P.gamma)
    for d in range(3):
        if P.periodic(d):
            continue
        t = sr.axis_terms(P, phi, V[d], d, dtype, limiter=limiter)
        A = areas(P, d, dtype)
        n = P.n[d]
        for side, f in ((0, 0), (1, n)):
            b = 2 * d + side
            conv = t["V"][f] * t["F"][f] * A
            diff = -gam * t["G"][f] * A
            faces = conv.size
            eF, eG = np.broadcast_to(t["eF"][f], conv.shape), np.broadcast_to(t["eG"][f], conv.shape)
            flux[b] = conv.sum(), diff.sum()
            bound[b, 0] = float(U * (np.abs(t["V"][f]) * eF * A + 3 * np.abs(conv)).sum() + (faces - 1) * U * np.abs(conv).sum())
            bound[b, 1] = float(U * (gam * eG * A + 3 * np.abs(diff)).sum() + (faces - 1) * U * np.abs(diff).sum())
    return flux, bound


def budget(flux):
    """sum_d (flux_lo,d - flux_hi,d), flux = convective + diffusive: what sum_c R(phi)(c) vol(c) - sum_c q vol telescopes to"""
    f = np.asarray(flux)
    return sum((f[2 * d, 0] + f[2 * d, 1]) - (f[2 * d + 1, 0] + f[2 * d + 1, 1]) for d in range(3))


def slack(bound):
    """a bound in absolute terms: the 2^-10 share for second-order terms and the long-double reference's own rounding (scalar_cases.rhs_slack)"""
    return np.asarray(bound, dtype=np.float64) * (1 + 2.0 ** -10) + np.finfo(np.float64).tiny


class BuoyantStep(fo.StepOracle):
    """StepOracle with momrhs += dt sum_s a_s,d (phi_s - ref_s).  scalars: a list of (phi, beta, ref) read when form_function runs (the caller
    replaces the list's fields between steps: the term uses phi^n); gravity: g[3]."""

    def __init__(self, *a, gravity=(0.0, 0.0, 0.0), scalars=(), **kw):
        super().__init__(*a, **kw)
        self.gravity, self.scalars = tuple(gravity), list(scalars)

    def buoyancy(self):
        N = self.g.ncell
        act = [(phi, beta, ref) for phi, beta, ref in self.scalars if beta != 0.0]
        if not act or not any(self.gravity):
            return np.zeros(3 * N), np.zeros(3 * N)
        accel = [[-beta * gd for gd in self.gravity] for _, beta, _ in act]
        T, M = term([phi for phi, _, _ in act], accel, [ref for _, _, ref in act], self.dt, np.float64)
        return T.ravel(), M.ravel()

    def form_function(self, v0, V0, p0, scale=True):
        momrhs, interprhs, W, sc = super().form_function(v0, V0, p0, scale)
        T, M = self.buoyancy()
        if sc is not None:
            sc = dict(v=sc["v"] + M, V=sc["V"])
        return momrhs + T, interprhs, W, sc
