"""Helper of tests/test_ibm_scalar_host.py and tests/test_gpu_ibm_scalar*.py (no GPU): fl_ibm_scalar_force / fl_ibm_scalar_rate
(include/fluca_hip_ibm_scalar.h) restated in numpy long double on the support and the weights of tests/ibm_reference.py, and the rate through
tests/ibm_force_reference.py's split sum.

    for k = 1 .. npass:   Phi = interp(phi),  q = T - Phi,  Q (+)= q,  phi += spread(q, dV)

Nothing is rounded to double between the passes (ibm_reference.interp / spread take double fields; the two functions below are their formulas on a
long-double field).

The bound a correctly built fp64 evaluation stays within, u = 2^-53, K = ibm_reference.ulp_factor(n) -- the bound of the existing IBM tests, carried
through the passes, nothing fitted.  M = the largest |phi^(k)| and |T| over all passes (reference), D = max over cells of sum_l dV_l w_l / V_cell,
e_k = max over cells of |phi_fp64^(k) - phi_ref^(k)|, e_0 = 0.  Both delta functions have weights >= 0 that sum to at most 1, so interpolating a field
that is off by e gives a value off by at most e, next to the K u M of tests/test_ibm_regimes.py; q = T - Phi rounds once a value <= 2 M:

    dq_k <= e_(k-1) + (K + 2) u M

Spreading q_fp64 is within test_ibm_regimes' u (K B + (m + 1) (|phi| + B)) of the exact spread of q_fp64, B = sum_l |q_l| dV_l / V_cell over the m
markers that reach the cell (with M for |phi|, and B of the reference's q enlarged by dq_k), and the exact spread of an error dq is at most D dq:

    e_k <= e_(k-1) + D dq_k + max_cell u (K B_k + (m + 1) (M + B_k))
    |Q_fp64 - Q_ref| <= sum_k dq_k + npass u max|Q|-so-far

times 1 + 2^-10 for second-order terms.  With one pass and e_0 = 0 this is the existing spread bound plus the term for q's own error."""
import numpy as np

from tests import ibm_force_reference as fr
from tests import ibm_reference as ref

LD = ref.LD
U53 = 2.0 ** -53


class Geometry:
    """support cells, weights and target-cell volumes of a marker set, formed once (long double)"""

    def __init__(self, n, xf, periodic, kind, X):
        self.n, self.xf = tuple(n), xf
        self.ncell = n[0] * n[1] * n[2]
        self.cell, self.ok, self.W = ref._support(n, xf, periodic, kind, X)
        self.L = self.cell.shape[0]
        self.vol = ref.cell_volumes(n, xf, np.arange(self.ncell))

    def interp(self, phi):
        phi = np.asarray(phi, dtype=LD).reshape(-1)
        return (self.W * np.where(self.ok, phi[self.cell], LD(0))).reshape(self.L, -1).sum(axis=1)

    def spread(self, q, dV):
        """the field sum_l q_l dV_l w_l / V_cell (long double, all cells)"""
        out = np.zeros(self.ncell, dtype=LD)
        FdV = np.asarray(q, dtype=LD) * np.asarray(dV, dtype=np.float64).astype(LD)
        lidx = np.broadcast_to(np.arange(self.L)[:, None, None, None], self.cell.shape)[self.ok]
        np.add.at(out, self.cell[self.ok], self.W[self.ok] * FdV[lidx])
        return out / self.vol

    def reached(self):
        out = np.zeros(self.ncell, dtype=bool)
        out[self.cell[self.ok]] = True
        return out

    def markers_per_cell(self):
        return np.bincount(self.cell[self.ok], minlength=self.ncell)

    def load(self, a):
        """sum over the markers reaching a cell of a_l / V_cell, no weights (test_ibm_regimes' B for a = |F| dV), double"""
        lidx = np.broadcast_to(np.arange(self.L)[:, None, None, None], self.cell.shape)[self.ok]
        return np.bincount(self.cell[self.ok], weights=np.asarray(a, dtype=np.float64)[lidx], minlength=self.ncell) / self.vol.astype(np.float64)


def force(geo, T, dV, phi, npass):
    """-> phi_out (ncell), Q (L) long double, and the per-pass lists q, phis (phis[0] = phi, phis[k] after pass k)"""
    T = np.asarray(T, dtype=np.float64).astype(LD)
    phi = np.asarray(phi, dtype=np.float64).astype(LD).reshape(-1)
    Q, qs, phis = np.zeros(geo.L, dtype=LD), [], [phi]
    for _ in range(npass):
        q = T - geo.interp(phi)
        Q = Q + q
        phi = phi + geo.spread(q, dV)
        qs.append(q)
        phis.append(phi)
    return phi, Q, qs, phis


def defect(geo, T, phi):
    """max_l |T_l - interp(phi)_l| as a double"""
    d = np.abs(np.asarray(T, dtype=np.float64).astype(LD) - geo.interp(phi))
    return float(d.max()) if d.size else 0.0


def bounds(geo, T, dV, qs, phis):
    """(bound on max_cell |phi_fp64 - phi_ref|, bound on max_l |Q_fp64 - Q_ref|) after len(qs) passes: the recursion of the module docstring"""
    K = ref.ulp_factor(geo.n)
    T = np.asarray(T, dtype=np.float64)
    M = max([float(np.abs(p).max()) for p in phis] + [float(np.abs(T).max()) if T.size else 0.0])
    D = float(geo.spread(np.ones(geo.L), dV).max()) if geo.L else 0.0
    m = geo.markers_per_cell()
    e, sdq, Qabs, Q = 0.0, 0.0, 0.0, np.zeros(geo.L, dtype=LD)
    for q in qs:
        dq = e + (K + 2) * U53 * M
        B = geo.load((np.abs(q).astype(np.float64) + dq) * np.asarray(dV, dtype=np.float64))
        e = e + D * dq + float((U53 * (K * B + (m + 1) * (M + B))).max())
        sdq += dq
        Q = Q + q
        Qabs = max(Qabs, float(np.abs(Q).max()) if geo.L else 0.0)
    slack = 1 + 2.0 ** -10
    return e * slack, (sdq + len(qs) * U53 * (Qabs + sdq)) * slack


def rate(Q, dV, body=None, nbody=1):
    """rate[b] = the split sum of the terms Q_l dV_l (each product rounded once) over the markers of body b, one exponent for the whole group; NaN for
    every body when a term is not finite"""
    t = np.asarray(Q, dtype=np.float64) * np.asarray(dV, dtype=np.float64)
    ids = np.zeros(t.size, dtype=np.int64) if body is None else np.asarray(body, dtype=np.int64)
    if not np.all(np.isfinite(t)):
        return np.full(nbody, np.nan)
    E = fr.group_exponent(t)
    return np.array([float(fr.split_sum(t[ids == b], E)) for b in range(nbody)])
