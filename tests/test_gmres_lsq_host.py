"""fluca_amd/csrc/fl_gmres_lsq.h on the host: the Givens least-squares update that momentum_gmres (fl_mom_solve.hip) and schur_solve_var (fl_abf.hip)
share.  tests/plugins/gmres_lsq_check.cpp (plain g++ against the header alone, no HIP) prints, with %a, the residual estimate after every column
and the final y; the judgement is here, twice over:

  against numpy -- every estimate is the least-squares residual norm of the leading block, and y solves the triangular system of a QR factorisation of
      H, both within 64 ulp of beta: a rounding bound for a sweep of at most five Givens rotations in double, not a measurement;
  against a line-for-line transcription of the loop momentum_gmres carried before the header existed (numpy float64, hypot from the same libm)
      -- every printed number bit for bit.

Three inputs: a fixed-seed 6 x 5 Hessenberg matrix; a 4 x 3 one whose last subdiagonal entry is zero (the happy breakdown: d > 0 through a alone);
the 2 x 1 zero column, which takes the d == 0 branch (cs = 1, sn = 0).  For that last input the triangular factor is the 1 x 1 zero matrix: the
least-squares problem has no unique y and its residual is beta whatever y is, while the loop -- then as now -- reports the estimate 0 and divides
g[0] = beta by zero.  No numpy figure exists to hold y against, and the estimate is NOT the least-squares residual (0 against beta = 1); the test
pins what the loop does there, bit for bit against the transcription, and says so instead of asserting the numpy comparison.  The drivers reach
that branch only with an operator that maps a Krylov vector to zero, which A = I + ... and S do not."""
import ctypes
import ctypes.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.hypot.restype = ctypes.c_double
_libm.hypot.argtypes = [ctypes.c_double, ctypes.c_double]


def _hessenberg(seed, k):
    H = np.triu(np.random.default_rng(seed).standard_normal((k + 1, k)), -1)
    return np.ascontiguousarray(H)


def _inputs():
    general = _hessenberg(20240607, 5)
    happy = _hessenberg(7, 3)
    happy[3, 2] = 0.
    return {"6x5 fixed seed": (general, 1.75), "4x3 zero last subdiagonal": (happy, 0.3), "2x1 zero column": (np.zeros((2, 1)), 1.)}


INPUTS = _inputs()


@pytest.fixture(scope="module")
def check():
    out = os.path.join(ROOT, "tests", "plugins", "gmres_lsq_check")
    src = os.path.join(ROOT, "tests", "plugins", "gmres_lsq_check.cpp")
    deps = [src, os.path.join(ROOT, "fluca_amd", "csrc", "fl_gmres_lsq.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", out, src])
    return out


def _run(check, H, beta):
    k = H.shape[1]
    text = "%d %s\n" % (k, float(beta).hex()) + "\n".join(" ".join(float(v).hex() for v in row) for row in H) + "\n"
    lines = subprocess.check_output([check], input=text, text=True).split("\n")
    est = [np.float64(float.fromhex(l.split()[1])) for l in lines if l.startswith("E ")]
    y = [np.float64(float.fromhex(l.split()[1])) for l in lines if l.startswith("Y ")]
    assert len(est) == k and len(y) == k
    return est, y


def _parent_loop(Hin, beta):
    """The rotations, the update of g and the back-substitution as momentum_gmres had them in the commit before fl_gmres_lsq.h (restart = k, one cycle
    of k columns, no convergence test), statement for statement."""
    restart = Hin.shape[1]
    H, cs, sn = np.zeros((restart + 1) * restart), np.zeros(restart), np.zeros(restart)
    g, hcol, y = np.zeros(restart + 1), np.zeros(restart + 1), np.zeros(restart)
    est = []
    with np.errstate(all="ignore"):
        g[:] = 0.
        g[0] = beta
        for k in range(restart):
            hcol[:k + 2] = Hin[:k + 2, k]
            for i in range(k):
                t = cs[i] * hcol[i] + sn[i] * hcol[i + 1]
                hcol[i + 1] = -sn[i] * hcol[i] + cs[i] * hcol[i + 1]
                hcol[i] = t
            d = np.float64(_libm.hypot(hcol[k], hcol[k + 1]))
            cs[k] = hcol[k] / d if d > 0. else 1.
            sn[k] = hcol[k + 1] / d if d > 0. else 0.
            hcol[k] = d
            hcol[k + 1] = 0.
            g[k + 1] = -sn[k] * g[k]
            g[k] = cs[k] * g[k]
            for i in range(k + 1):
                H[i * restart + k] = hcol[i]
            est.append(np.fabs(g[k + 1]))
        k = restart
        for i in range(k - 1, -1, -1):
            t = g[i]
            for j in range(i + 1, k):
                t -= H[i * restart + j] * y[j]
            y[i] = t / H[i * restart + i]
    return est, list(y)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_bit_for_bit_against_the_loop_it_replaced(check, name):
    H, beta = INPUTS[name]
    est, y = _run(check, H, beta)
    pest, py = _parent_loop(H, beta)
    assert [v.tobytes() for v in est] == [np.float64(v).tobytes() for v in pest], (name, est, pest)
    assert [v.tobytes() for v in y] == [np.float64(v).tobytes() for v in py], (name, y, py)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_against_numpy(check, name):
    H, beta = INPUTS[name]
    k = H.shape[1]
    est, y = _run(check, H, beta)
    bound = 64. * np.spacing(np.float64(beta))
    rhs = np.zeros(k + 1)
    rhs[0] = beta
    if np.linalg.matrix_rank(H) < k:
        # the d == 0 branch (see the module's docstring): what the loop yields there, stated rather than compared
        assert name == "2x1 zero column" and est == [0.] and np.isinf(y[0]) and y[0] > 0.
        return
    for j in range(k):
        A, b = H[:j + 2, :j + 1], rhs[:j + 2]
        r = b - A @ np.linalg.lstsq(A, b, rcond=None)[0]
        want = np.linalg.norm(r)
        print(name, "column", j, "estimate", est[j], "numpy", want, "difference", abs(est[j] - want), "bound", bound)
        assert abs(est[j] - want) <= bound, (name, j)
    Q, R = np.linalg.qr(H, mode="complete")
    res = R[:k, :k] @ np.array(y) - (Q.T @ rhs)[:k]
    print(name, "triangular system residual", np.abs(res).max(), "bound", bound)
    assert np.abs(res).max() <= bound, name
    if name == "4x3 zero last subdiagonal":   # an exact fit: the last estimate is 0 up to the bound, through d = |a| > 0
        assert H[k, k - 1] == 0. and est[-1] <= bound
