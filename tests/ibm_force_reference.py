"""Helper of tests/test_ibm_force_host.py and tests/test_gpu_ibm_force.py (no GPU): fl_ibm_force (include/fluca_hip.h) restated in numpy.

  terms        F_c dV and ((r x F)_c) dV with the roundings the header names: every product, difference and quotient rounded once (numpy's
               element-wise operations never fuse), r the minimum image on a periodic axis
  exact_sum    the sum of a row of terms as a rational number (fractions.Fraction: a double is a rational)
  bound        L 2^(E-61) + 1/2 ulp(result): what the split drops plus the one rounding at the end
  split_sum    the order-independent sum itself: t = hi + mid + tail, hi = rint(t / u1) u1, mid = rint((t - hi) / u2) u2, u1 = 2^(E-30),
               u2 = 2^(E-60); the hi and the mid parts add up exactly in ANY order (np.sum's pairwise order here), one rounding at the end
"""
import math
from fractions import Fraction

import numpy as np


def terms(X, F, dV, about, period=(None, None, None)):
    """X, F: (3, L); dV: (L,); about: (3,) or, one reference point per marker, (3, L) -> (force terms (3, L), torque terms (3, L))"""
    X, F, dV = np.asarray(X, dtype=np.float64), np.asarray(F, dtype=np.float64), np.asarray(dV, dtype=np.float64)
    about = np.asarray(about, dtype=np.float64)
    if about.ndim == 1:
        about = about[:, None]
    r = X - about
    for d in range(3):
        if period[d] is not None:
            P = np.float64(period[d])
            r[d] = r[d] - P * np.rint(r[d] / P)
    tf = F * dV
    tt = np.stack([(r[(c + 1) % 3] * F[(c + 2) % 3] - r[(c + 2) % 3] * F[(c + 1) % 3]) * dV for c in range(3)])
    return tf, tt


def exponent(tmax):
    """E with tmax < 2^E (tmax > 0, finite)"""
    return math.frexp(float(tmax))[1]


def group_exponent(t):
    """E of a group of terms, None when all of them are zero (or there are none)"""
    t = np.asarray(t, dtype=np.float64)
    tmax = float(np.abs(t).max()) if t.size else 0.0
    return exponent(tmax) if tmax > 0.0 else None


def split(t, E):
    """(hi, mid) of every term"""
    t = np.asarray(t, dtype=np.float64)
    u1, u2 = math.ldexp(1.0, E - 30), math.ldexp(1.0, E - 60)
    hi = np.rint(t / u1) * u1
    mid = np.rint((t - hi) / u2) * u2
    return hi, mid


def split_sum(t, E):
    """the order-independent sum of the terms t (any shape; summed over the last axis) with the group's exponent E"""
    t = np.asarray(t, dtype=np.float64)
    if E is None or t.shape[-1] == 0:
        return np.zeros(t.shape[:-1])
    hi, mid = split(t, E)
    return hi.sum(axis=-1) + mid.sum(axis=-1)


def split_sum_parts(parts, E):
    """the same sum formed per part ("rank") first and the partial sums added afterwards, hi and mid apart: what the all-reduces do"""
    H, M = 0.0, 0.0
    for p in parts:
        if np.asarray(p).shape[-1]:
            hi, mid = split(p, E)
            H, M = H + hi.sum(axis=-1), M + mid.sum(axis=-1)
    return H + M


def exact_sum(row):
    return sum((Fraction(float(v)) for v in np.asarray(row).ravel()), Fraction(0))


def ulp(x):
    x = abs(float(x))
    return math.ulp(x) if x > 0.0 else 0.0


def bound(L, E, result):
    """|result - exact| <= L 2^(E-61) + 1/2 ulp(result), as a Fraction; L = the markers of ALL bodies and ranks that were split with E"""
    if E is None:
        return Fraction(0)
    return L * Fraction(2) ** (E - 61) + Fraction(ulp(result)) / 2


def reference(X, F, dV, about, period=(None, None, None), body=None, nbody=1):
    """force, torque (nbody, 3) by the split sum, and per entry the exact sums and the bounds: dict(force, torque, exact_force, exact_torque,
    bound_force, bound_torque, abs_force, abs_torque); about: (nbody, 3)"""
    X = np.asarray(X, dtype=np.float64)
    L = X.shape[1]
    about = np.asarray(about, dtype=np.float64).reshape(nbody, 3)
    ids = np.zeros(L, dtype=np.int64) if body is None else np.asarray(body, dtype=np.int64)
    tf, tt = terms(X, F, dV, about[ids].T if L else np.zeros((3, 0)), period)
    out = {}
    for name, t in (("force", tf), ("torque", tt)):
        E = group_exponent(t)
        val = np.zeros((nbody, 3))
        exact = [[Fraction(0)] * 3 for _ in range(nbody)]
        bnd = [[Fraction(0)] * 3 for _ in range(nbody)]
        absum = np.zeros((nbody, 3))
        if not np.all(np.isfinite(t)):      # a non-finite term: the whole group is NaN, no exact sum to compare with
            out[name], out["exact_" + name], out["bound_" + name], out["abs_" + name], out["E_" + name] = np.full((nbody, 3), np.nan), None, None, None, None
            continue
        for b in range(nbody):
            tb = t[:, ids == b]
            val[b] = split_sum(tb, E)
            for c in range(3):
                exact[b][c] = exact_sum(tb[c])
                bnd[b][c] = bound(L, E, val[b, c])
                absum[b, c] = math.fsum(np.abs(tb[c]))
        out[name], out["exact_" + name], out["bound_" + name], out["abs_" + name], out["E_" + name] = val, exact, bnd, absum, E
    return out


def within(ref, name, got):
    """the largest |got - exact| / bound over the entries of `name` (force / torque); <= 1 is within the bound (an entry whose bound is zero must be exact)"""
    worst = 0.0
    got = np.asarray(got, dtype=np.float64).reshape(-1, 3)
    for b in range(got.shape[0]):
        for c in range(3):
            err = abs(Fraction(float(got[b, c])) - ref["exact_" + name][b][c])
            bd = ref["bound_" + name][b][c]
            worst = max(worst, float(err / bd) if bd > 0 else (0.0 if err == 0 else math.inf))
    return worst
