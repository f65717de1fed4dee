"""How the Krylov solves stop, named: one case per (solver family, way of stopping), built with the oracle only.

Every solve of the library ends through a small device-side state machine (converged_default, cg_fin_apply, the BiCGStab / Chebyshev scalar
kernels, the host loops of GMRES and MG-PCG, finish_stats, fl_poisson::poisoned).  The parity suite drives it to two outcomes, "met rtol" (2)
and "ran into maxit" (-3).  STOPS names a case for every other outcome the public API can reach; each case carries the grid, the boundary types,
the recipe of its right-hand side, the solver options, what the oracle must return (reason, iterations) and, for a stop decided by a threshold
inside a solve, the margin by which the oracle's own history decides it (the ratios of the last two history values to the threshold).
tests/test_ksp_stops.py checks the table against the oracle on the CPU -- the condition that keeps a GPU case from passing by accident;
tests/test_gpu_ksp_stops.py runs the cases through the C-ABI.

Parts (the letters of the test names):
  A  reasons at iteration 0: b = 0, maxit = 0, a NaN / an Inf in b, dtol = 0.5, atol above the first norm
  B  CONVERGED_ATOL against CONVERGED_RTOL in mid-solve, with a zero and with a non-zero initial guess
  C  DIVERGED_DTOL in mid-solve, inside a polling window, with x-updates owed to the direction ring
  D  the momentum Chebyshev on its default interval without a norm is watched: DIVERGED_DTOL, never garbage after maxit steps
  E  the handle after a bad solve (in the GPU test only: it needs no oracle, a fresh handle is the reference)
  F  DIVERGED_INDEFINITE_MAT
  G  several ranks"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import fluca_oracle as fo
from tests.gpu_common import stretched_faces
from tests.launch_regimes import BY_NAME, CAVITY, CHANNEL, CHEB2_MIN_CELLS, SLAB

CG, BCGS, CHEB, GMRES = fo.KSP_CG, fo.KSP_BCGS, fo.KSP_CHEBYSHEV, fo.KSP_GMRES
NOPC, JACOBI, MG = 0, 1, 2                                   # fl_ksp_opts.pc
PRE, UNPRE, NATURAL, NONORM = fo.NORM_PRECONDITIONED, fo.NORM_UNPRECONDITIONED, fo.NORM_NATURAL, fo.NORM_NONE

# include/fluca_hip.h (KSPConvergedReason)
RTOL, ATOL, ITS = 2, 3, 4
DIV_ITS, DIV_DTOL, DIV_BREAKDOWN, DIV_INDEFINITE_PC, DIV_NANORINF, DIV_INDEFINITE_MAT = -3, -4, -5, -8, -9, -10

KAPPA = 1e-3
SMALL = (24, 20, 16)      # the smallest grid that still takes the production paths of CG, single-reduction CG, BiCGStab and GMRES
FUSED = (40, 32, 28)      # 35 840 cells: at or above CHEB2_MIN_CELLS, the Chebyshev steps come in pairs (k_cheb2); MG-PCG smooths with them
assert FUSED[0] * FUSED[1] * FUSED[2] >= CHEB2_MIN_CELLS > SMALL[0] * SMALL[1] * SMALL[2]
MOM3 = BY_NAME["mom_unmapped"].n             # (130, 37, 43): the smallest grid of tests/test_gpu_momentum_regimes.py that takes k_mom3 (ny > 8)
MOM2 = BY_NAME["mom_stored_one_plane"].n     # (300, 8, 100): ny = 8, every product is k_mom2 + a vector update
MOM_BC = {MOM3: tuple(CAVITY), MOM2: tuple(SLAB)}

HIST_RTOL = 1e-9          # histories against the oracle: what tests/test_gpu_rank_regimes.py uses
X_RTOL = 1e-9             # x of a converging solve stopped at the oracle's iteration, relative to max |x|: what tests/test_gpu_cg_xflush.py uses
RING_DEPTHS = (2, 8, 16)  # cg_xdepth: a stop at an iteration that is a multiple of the depth leaves no x-update owed
MARGIN = 1.15             # a threshold stop: the oracle's two straddling history values lie at least 15 % on either side of the threshold
X_NOISE_FACTOR = 100.0    # x at the stop of a diverging solve: this many times the oracle's own answer to a 1e-16 perturbation of b


# ------------------------------------------------------------------------------------------------ the problems

@functools.lru_cache(maxsize=4)
def poisson(n, bc):
    """(oracle grid, S) on the stretched grid of n cells"""
    g = fo.Grid(n, stretched_faces(n), bc, KAPPA)
    return g, g.assemble_S()


def has_nullspace(bc):
    return fo.BC_PRESSURE_OUTLET not in bc


def cell(n, where):
    """index of the cell next to a wall ("x-", "x+", ... "z+": the middle of that face of the box) or in the middle of the grid ("in")"""
    ijk = [n[0] // 2, n[1] // 2, n[2] // 2]
    if where != "in":
        ax = "xyz".index(where[0])
        ijk[ax] = 0 if where[1] == "-" else n[ax] - 1
    return ijk[0] + n[0] * (ijk[1] + n[1] * ijk[2])


WHERE = ("x-", "x+", "y-", "y+", "z-", "z+", "in")


def poison(b, n, recipe):
    """recipe[1:] = ("nan" | "inf", where) puts one non-finite entry into a copy of b (the first component of a velocity vector)"""
    b = b.copy()
    if len(recipe) > 1:
        b[cell(n, recipe[2])] = np.nan if recipe[1] == "nan" else np.inf
    return b


@functools.lru_cache(maxsize=16)
def _poisson_rhs(n, bc, kind):
    g, S = poisson(n, bc)
    if kind == "zero":
        return np.zeros(g.ncell)
    p = np.random.default_rng(1).uniform(-1.0, 1.0, g.ncell)
    if has_nullspace(bc):
        p -= p.mean()
    b = S.mult(p)
    if kind == "inconsistent":            # not mean-free: on CAVITY (a singular S) without the null-space removal CG and BiCGStab diverge
        b = b + 0.05 * np.abs(b).max()
    return b


def poisson_rhs(n, bc, recipe):
    return poison(_poisson_rhs(n, bc, recipe[0]), n, recipe)


def momentum_state(g, vmag=0.5, seed=23):
    """tests/test_gpu_momentum_cheb.py::_state: CFL-sized convection beside a viscous part of the same size"""
    rng = np.random.default_rng(seed)
    V0 = [vmag * rng.uniform(-1, 1, g.nface[d]) for d in range(3)]
    v0 = vmag * rng.uniform(-1, 1, 3 * g.ncell)
    hmin = min(np.diff(g.xf[d]).min() for d in range(3))
    dt, rho = 0.4 * hmin, 1.3
    mu = 0.8 * rho * hmin * hmin / dt
    return V0, v0, dt, rho, mu


@functools.lru_cache(maxsize=2)
def momentum(n):
    """the oracle side of the momentum block on the stretched grid n: grid, state, W = B v0"""
    g = fo.Grid(n, stretched_faces(n), MOM_BC[n], KAPPA)
    V0, v0, dt, rho, mu = momentum_state(g)
    return SimpleNamespace(g=g, V0=V0, v0=v0, dt=dt, rho=rho, mu=mu, W=g.apply_B(v0))


@functools.lru_cache(maxsize=4)
def momentum_A(n, weight=1.0):
    """A = I + weight dt C - (mu dt / 2 rho) L: what Momentum.set_coefficients(1, weight dt, -mu dt / 2 rho) makes of the state"""
    s = momentum(n)
    return s.g.assemble_momentum(1.0, weight * s.dt, -0.5 * s.mu * s.dt / s.rho, s.V0, s.W)


def momentum_interval(A):
    """fl_momentum_chebyshev_interval: [max(1 - g, 0.9 / mean a_ii), 1 + g], g the Gershgorin radius of D^-1 A"""
    radius = A.gershgorin(fo.PC_JACOBI) - 1.0
    return max(1.0 - radius, 0.9 / A.diag().mean()), 1.0 + radius


@functools.lru_cache(maxsize=8)
def _momentum_rhs(n, kind):
    N = 3 * momentum(n).g.ncell
    return np.zeros(N) if kind == "zero" else np.random.default_rng(7).standard_normal(N)


def momentum_rhs(n, recipe):
    return poison(_momentum_rhs(n, recipe[0]), n, recipe)


@functools.lru_cache(maxsize=2)
def momentum_guess(n):
    """the non-zero initial guess of part B: the converged answer, off by 1e-3 of its size"""
    A = momentum_A(n)
    b = _momentum_rhs(n, "random")
    xo, _ = A.solve(b, ksp=BCGS, pc=JACOBI, nullspace=False, rtol=1e-13, maxit=1000, history=False)
    return xo + 1e-3 * np.linalg.norm(xo) / np.sqrt(xo.size) * np.random.default_rng(9).standard_normal(xo.size)


# ------------------------------------------------------------------------------------------------ the cases

class Stop:
    """name; part (a letter); handle: "poisson" | "momentum"; n, bc; rhs: the recipe (kind[, "nan" | "inf", where]); opts: fl_ksp_opts fields
    (what Poisson.solve / Momentum.solve take); reason, iters: what the oracle must return (iters None: not fixed by the table);
    threshold: None, or (which, value, k): the stop is decided at iteration k by history[k] crossing value ("atol", "rtol": from above; "dtol":
    value x history[0] from below); weight: the convection weight of a momentum case; guess: the solve starts from momentum_guess;
    oracle: False where no oracle restates the solver (MG-PCG: reason and iterations follow from the rule of the part)"""

    def __init__(self, name, part, handle, n, bc, rhs, opts, reason, iters, threshold=None, weight=1.0, guess=False, oracle=True, xtol=None):
        self.name, self.part, self.handle, self.n, self.bc, self.rhs, self.opts = name, part, handle, tuple(n), tuple(bc), tuple(rhs), dict(opts)
        self.reason, self.iters, self.threshold, self.weight, self.guess, self.oracle, self.xtol = reason, iters, threshold, weight, guess, oracle, xtol

    def __repr__(self):
        return self.name

    def b(self):
        return poisson_rhs(self.n, self.bc, self.rhs) if self.handle == "poisson" else momentum_rhs(self.n, self.rhs)


def interval(case):
    """(emin, emax) of a Chebyshev case as numbers, or (0, 0) = the solver's default"""
    iv = case.opts.get("interval")
    if iv is None:
        return 0.0, 0.0
    g, S = poisson(case.n, case.bc)
    lam = S.gershgorin(case.opts.get("pc", JACOBI))
    return iv * 0.1 * lam, iv * 1.1 * lam


def gpu_opts(case):
    """the keyword arguments of Poisson.solve / Momentum.solve"""
    kw = {k: v for k, v in case.opts.items() if k != "interval"}
    if "interval" in case.opts:
        kw["emin"], kw["emax"] = interval(case)
    if case.handle == "poisson":
        kw.setdefault("remove_nullspace", int(has_nullspace(case.bc)))
    if case.guess:
        kw["initial_guess_nonzero"] = 1
    return kw


_ORACLE = {}


def oracle_solve(case, b=None, **override):
    """(x, info) of the oracle on the case (cached when nothing is overridden); info["history"][k] is the monitored norm of iteration k"""
    key = case.name
    if b is None and not override and key in _ORACLE:
        return _ORACLE[key]
    o = dict(case.opts, **override)
    kw = dict(rtol=o.get("rtol", 1e-5), atol=o.get("atol", 1e-50), dtol=o.get("dtol", 1e5), maxit=o.get("maxit", 10000))
    ksp, pc = o.get("type", CG if case.handle == "poisson" else BCGS), o.get("pc", JACOBI)
    bb = case.b() if b is None else b
    if case.handle == "poisson":
        S = poisson(case.n, case.bc)[1]
        emin, emax = interval(case)
        x, info = S.solve(bb, ksp=ksp, pc=pc, norm=o.get("norm_type", PRE), nullspace=bool(o.get("remove_nullspace", has_nullspace(case.bc))),
                          emin=emin, emax=emax, single_reduction=bool(o.get("cg_single_reduction", 0)), **kw)
    else:
        A = momentum_A(case.n, case.weight)
        x0 = None
        if case.guess:
            # KSPConvergedDefault with a non-zero guess tests against the norm of the right-hand side: the solve from zero on the shifted system
            # A d = b - A x0 to the absolute tolerance max(rtol || M b ||, atol); reason 3 only where the norm is below atol itself
            x0 = momentum_guess(case.n)
            dinv = 1.0 / A.diag() if pc == JACOBI and o.get("norm_type", PRE) != UNPRE else 1.0
            bnorm = float(np.linalg.norm(dinv * bb))
            user_atol = kw["atol"]
            kw.update(rtol=0.0, atol=max(kw["rtol"] * bnorm, user_atol))
            bb = bb - A.mult(x0)
        if ksp == GMRES:
            x, info = fo.gmres(A, bb, pc=pc, **kw)
        else:
            emin, emax = (0.0, 0.0)
            norm = o.get("norm_type", PRE)
            if ksp == CHEB:
                emin, emax = momentum_interval(A)
                if norm == NONORM:       # watched: the preconditioned norm, no convergence test
                    norm = PRE
                    kw.update(rtol=0.0, atol=0.0)
            x, info = A.solve(bb, ksp=ksp, pc=pc, norm=norm, nullspace=False, emin=emin, emax=emax, **kw)
            if ksp == CHEB and o.get("norm_type", PRE) == NONORM and info["reason"] == DIV_ITS:
                info["reason"] = ITS
        if case.guess:
            x = x0 + x
            if info["reason"] == ATOL and not info["rnorm"] < user_atol:
                info["reason"] = RTOL
            info["rnorm0"] = bnorm
    if b is None and not override:
        _ORACLE[key] = (x, info)
    return x, info


def margins(case, history):
    """of a threshold stop at iteration k: (threshold / the value that met it, the value before / threshold) for a test passed from above (atol, rtol),
    the reciprocals for dtol; both > 1 where the history decides the stop, and by how much"""
    which, value, k = case.threshold
    t = value * history[0] if which in ("dtol", "rtol") else value
    lo, hi = (history[k - 1], history[k]) if which == "dtol" else (history[k], history[k - 1])
    return t / lo, hi / t


def x_noise(case, seeds=range(5)):
    """the largest change of the oracle's x at the stop, relative to max |x|, under relative noise of 1e-16 on b"""
    b = case.b()
    x, info = oracle_solve(case)
    worst = 0.0
    for seed in seeds:
        bp = b * (1.0 + 1e-16 * np.random.default_rng(seed).standard_normal(b.size))
        xp, ip = oracle_solve(case, b=bp)
        assert (ip["reason"], ip["iters"]) == (info["reason"], info["iters"]), (case, seed)
        worst = max(worst, float(np.abs(xp - x).max() / np.abs(x).max()))
    return worst


def overflow_stop(case, scale, dtol):
    """(reason, iterations) of the oracle on scale x b with the divergence test out of reach: the norm overflows before anything else stops the solve"""
    _, info = oracle_solve(case, b=scale * case.b(), dtol=dtol)
    return info["reason"], info["iters"]


def _families_A():
    """(tag, handle, grid, bc, options): every solver family of fl_poisson_solve and fl_momentum_solve, the legal preconditioners and norms"""
    out = []
    for pc, pn in ((NOPC, "none"), (JACOBI, "jacobi")):
        for norm, nn in ((PRE, "pre"), (UNPRE, "unpre"), (NATURAL, "natural")):
            out.append((f"cg-{pn}-{nn}", "poisson", SMALL, CAVITY, dict(type=CG, pc=pc, norm_type=norm)))
        out.append((f"cgsr-{pn}", "poisson", SMALL, CAVITY, dict(type=CG, pc=pc, cg_single_reduction=1)))
        out.append((f"bcgs-{pn}", "poisson", SMALL, CHANNEL, dict(type=BCGS, pc=pc)))
        for norm, nn in ((PRE, "pre"), (UNPRE, "unpre"), (NONORM, "nonorm")):
            out.append((f"cheb-{pn}-{nn}", "poisson", FUSED, CHANNEL, dict(type=CHEB, pc=pc, norm_type=norm, interval=1.0)))
    out.append(("cgsr-jacobi-unpre", "poisson", SMALL, CAVITY, dict(type=CG, pc=JACOBI, cg_single_reduction=1, norm_type=UNPRE)))
    out.append(("mg", "poisson", FUSED, CAVITY, dict(type=CG, pc=MG)))
    for n, tag in ((MOM3, "mom3"), (MOM2, "mom2")):
        out.append((f"{tag}-bcgs", "momentum", n, MOM_BC[n], dict(type=BCGS, pc=JACOBI)))
        out.append((f"{tag}-gmres", "momentum", n, MOM_BC[n], dict(type=GMRES, pc=JACOBI)))
        out.append((f"{tag}-cheb", "momentum", n, MOM_BC[n], dict(type=CHEB, pc=JACOBI)))
    out.append(("mom3-bcgs-none", "momentum", MOM3, MOM_BC[MOM3], dict(type=BCGS, pc=NOPC)))
    out.append(("mom3-cheb-nonorm", "momentum", MOM3, MOM_BC[MOM3], dict(type=CHEB, pc=JACOBI, norm_type=NONORM)))
    return out


def _stop_A(tag, handle, n, bc, o, what, rhs, extra, reason):
    return Stop(f"A-{tag}-{what}", "A", handle, n, bc, rhs, {**o, "maxit": 40, **extra}, reason, 0, oracle=o["pc"] != MG)


def _part_A():
    out = []
    for tag, handle, n, bc, o in _families_A():
        nonorm = o.get("norm_type") == NONORM
        kind = "consistent" if handle == "poisson" else "random"
        mk = functools.partial(_stop_A, tag, handle, n, bc, o)
        if nonorm:
            # nothing is tested between the steps of KSP_NORM_NONE: the one stop at iteration 0 is maxit = 0, CONVERGED_ITS.  (The momentum
            # Chebyshev on its default interval is watched all the same: part D.)
            out.append(mk("maxit0", (kind,), dict(maxit=0), ITS))
            continue
        out.append(mk("zero", ("zero",), {}, ATOL))
        out.append(mk("maxit0", (kind,), dict(maxit=0), DIV_ITS))
        out.append(mk("nan", (kind, "nan", "in"), {}, DIV_NANORINF))
        out.append(mk("inf", (kind, "inf", "x+"), {}, DIV_NANORINF))
        out.append(mk("dtol", (kind,), dict(dtol=0.5), DIV_DTOL))
        out.append(mk("atol", (kind,), dict(atol=1e30), ATOL))
    return out


# B: reason 3 against reason 2 in mid-solve.  With atol = 1e-50 the relative test stops the solve at K2 (reason 2); with atol the geometric mean of
# the oracle's history[K3 - 1] and history[K3] (K3 about half-way) the absolute one stops it at K3 (reason 3).  rtol is KSP's default 1e-5 except for
# the Poisson BiCGStab: under the default it runs 50 iterations through two near-breakdowns (the norm rises thirtyfold at iterations 22 and 39), the
# range where tests/test_gpu_ksp.py lets the iteration count drift; rtol = 1.0911e-3 stops it at iteration 10, before that range, and the case is
# held to the same tolerances as every other.  From a non-zero guess (the momentum block only) the host code re-labels the reason:
# rtol = 1e-7 of || M b || reaches 2, rtol = 1e-30 under the atol of the table reaches 3.
# The margins of all these stops are at least B_MARGIN: seven orders above the 1e-9 to which the histories agree.
B_MARGIN = 1.01
#       tag           handle      grid   bc       options                      rtol       K2  K3  atol
_B = [("cg",         "poisson",  SMALL, CAVITY,  dict(type=CG, pc=JACOBI),    1e-5,      81, 40, 7.391300e-03),
      ("bcgs",       "poisson",  SMALL, CHANNEL, dict(type=BCGS, pc=JACOBI),  1.0911e-3, 10, 5,  4.128e-01),
      ("mom3-bcgs",  "momentum", MOM3,  None,    dict(type=BCGS, pc=JACOBI),  1e-5,      5,  2,  6.377913e+00),
      ("mom3-gmres", "momentum", MOM3,  None,    dict(type=GMRES, pc=JACOBI), 1e-5,      9,  4,  2.100251e+00),
      ("mom3-cheb",  "momentum", MOM3,  None,    dict(type=CHEB, pc=JACOBI),  1e-5,      10, 5,  1.886014e+00),
      ("mom2-bcgs",  "momentum", MOM2,  None,    dict(type=BCGS, pc=JACOBI),  1e-5,      6,  3,  8.557865e-01)]
#             tag           grid  options                      K2 K3 atol
_B_GUESS = [("mom3-bcgs",  MOM3, dict(type=BCGS, pc=JACOBI),  4, 2, 6.915480e-03),
            ("mom3-gmres", MOM3, dict(type=GMRES, pc=JACOBI), 7, 3, 9.313879e-03),
            ("mom3-cheb",  MOM3, dict(type=CHEB, pc=JACOBI),  8, 4, 7.350917e-03),
            ("mom2-bcgs",  MOM2, dict(type=BCGS, pc=JACOBI),  4, 2, 8.016313e-03)]
B_GUESS_RTOL = 1e-7


def _part_B():
    out = []
    for tag, handle, n, bc, o, rtol, k2, k3, atol in _B:
        bc = MOM_BC[n] if bc is None else bc
        rhs = ("consistent",) if handle == "poisson" else ("random",)
        out.append(Stop(f"B-{tag}-rtol", "B", handle, n, bc, rhs, dict(o, maxit=200, rtol=rtol, atol=1e-50), RTOL, k2, threshold=("rtol", rtol, k2)))
        out.append(Stop(f"B-{tag}-atol", "B", handle, n, bc, rhs, dict(o, maxit=200, rtol=rtol, atol=atol), ATOL, k3, threshold=("atol", atol, k3)))
    for tag, n, o, k2, k3, atol in _B_GUESS:
        out.append(Stop(f"B-{tag}-guess-rtol", "B", "momentum", n, MOM_BC[n], ("random",), dict(o, maxit=200, rtol=B_GUESS_RTOL, atol=1e-50), RTOL, k2,
                        threshold=("guess-rtol", B_GUESS_RTOL, k2), guess=True))
        out.append(Stop(f"B-{tag}-guess-atol", "B", "momentum", n, MOM_BC[n], ("random",), dict(o, maxit=200, rtol=1e-30, atol=atol), ATOL, k3,
                        threshold=("atol", atol, k3), guess=True))
    return out


# C: DIVERGED_DTOL in mid-solve.  CAVITY without the null-space removal, b = S p + 0.05 max |S p| (not mean-free): CG and BiCGStab diverge.  dtol is
# the geometric mean of the oracle's two straddling ratios history[K - 1] / history[0] and history[K] / history[0]; K is no multiple of a ring
# depth (the single-reduction CG and BiCGStab keep no ring), check_every stays at its default 16, so up to 15 queued launches follow the stop and
# up to 7 x-updates are owed at the default depth.  Chebyshev: CHANNEL, the interval a half / a quarter of gershgorin x (0.1, 1.1), KSP's default dtol.
# noise: the largest relative change of the oracle's x at the stop under a 1e-16 relative perturbation of b (x_noise, five seeds), measured with
# the oracle alone; the GPU's x may differ from the oracle's by X_NOISE_FACTOR times that.
#       tag          grid   bc       rhs             options                                                        dtol      K   noise
_C = [("pcg",       SMALL, CAVITY,  "inconsistent", dict(type=CG, pc=JACOBI, remove_nullspace=0),                   4.01629,  5,  2.3e-15),
      ("cg",        SMALL, CAVITY,  "inconsistent", dict(type=CG, pc=NOPC, remove_nullspace=0),                     3.60454,  9,  2.3e-15),
      ("cgsr",      SMALL, CAVITY,  "inconsistent", dict(type=CG, pc=JACOBI, remove_nullspace=0, cg_single_reduction=1), 1.5315, 4, 6.4e-15),
      ("bcgs",      SMALL, CAVITY,  "inconsistent", dict(type=BCGS, pc=JACOBI, remove_nullspace=0),                 2.68172,  13, 1.2e-11),
      ("cheb-half", FUSED, CHANNEL, "consistent",   dict(type=CHEB, pc=JACOBI, interval=0.5),                       1e5,      13, 1.1e-15),
      ("cheb-quarter", FUSED, CHANNEL, "consistent", dict(type=CHEB, pc=JACOBI, interval=0.25),                     1e5,      7,  6.0e-16)]
# F: the same inconsistent system under KSP's default dtol reaches DIVERGED_INDEFINITE_MAT: the stretched grid makes S non-symmetric, and p . S p of
# the direction after iteration K is negative by far more than rounding (indefinite_margin: -1.5e-4 and -1.2e-2 of |p| |S p|; the table needs 1e-8)
#       tag     options                                         K   noise
_F = [("cg",   dict(type=CG, pc=NOPC, remove_nullspace=0),     20, 1.6e-13),
      ("pcg",  dict(type=CG, pc=JACOBI, remove_nullspace=0),   5,  2.3e-15)]
F_MARGIN = 1e-8


def indefinite_margin(case):
    """a numpy restatement of CG with S.mult on the case: (the iterations done when p . S p <= 0, p . S p / (|p| |S p|) there)"""
    g, S = poisson(case.n, case.bc)
    b = case.b()
    dinv = 1.0 / S.diag() if case.opts["pc"] == JACOBI else np.ones(g.ncell)
    x, r = np.zeros_like(b), b.copy()
    z = dinv * r
    beta, betaold, p = r @ z, 1.0, z.copy()
    for it in range(1000):
        if it:
            p = z + (beta / betaold) * p
        betaold = beta
        w = S.mult(p)
        dpi = p @ w
        if dpi <= 0.0:
            return it, dpi / (np.linalg.norm(p) * np.linalg.norm(w))
        a = beta / dpi
        x += a * p
        r -= a * w
        z = dinv * r
        beta = r @ z
    return None, None


def _part_CF():
    out = []
    for tag, n, bc, rhs, o, dtol, k, noise in _C:
        out.append(Stop(f"C-{tag}", "C", "poisson", n, bc, (rhs,), dict(o, maxit=60, dtol=dtol), DIV_DTOL, k, threshold=("dtol", dtol, k), xtol=noise))
    for tag, o, k, noise in _F:
        out.append(Stop(f"F-{tag}", "F", "poisson", SMALL, CAVITY, ("inconsistent",), dict(o, maxit=60), DIV_INDEFINITE_MAT, k, xtol=noise))
    return out


# D: fl_mom_solve.hip promises that KSPCHEBYSHEV on the default interval with -ksp_norm_type none is never left unwatched.  The operator is
# A = I + weight dt C - (mu dt / 2 rho) L (Momentum.set_coefficients): at the weights below the diagonal of A changes sign, the spectrum of D^-1 A
# leaves the heuristic interval and the oracle's Chebyshev on that interval (preconditioned norm, no convergence test, dtol 1e5) crosses dtol at
# step K; at weight 1 the same recurrence converges, and 20 steps end with CONVERGED_ITS.
D_MAXIT, D_BENIGN_STEPS = 400, 20
#       tag     grid  weight  K
_D = [("mom3", MOM3, 10.0,   133),
      ("mom2", MOM2, 8.0,    89)]


def _part_D():
    out = []
    o = dict(type=CHEB, pc=JACOBI, norm_type=NONORM)
    for tag, n, w, k in _D:
        out.append(Stop(f"D-{tag}-diverges", "D", "momentum", n, MOM_BC[n], ("random",), dict(o, maxit=D_MAXIT), DIV_DTOL, k, threshold=("dtol", 1e5, k), weight=w))
        out.append(Stop(f"D-{tag}-benign", "D", "momentum", n, MOM_BC[n], ("random",), dict(o, maxit=D_BENIGN_STEPS), ITS, D_BENIGN_STEPS))
    return out


STOPS = _part_A() + _part_B() + _part_CF() + _part_D()
STOP = {c.name: c for c in STOPS}
assert len(STOP) == len(STOPS)

# the reasons of include/fluca_hip.h the table reaches, and those it cannot reach through the public API: BREAKDOWN needs an inner product that is
# exactly zero (b = 0 ends in CONVERGED_ATOL first), INDEFINITE_PC a negative r . z (Jacobi on a positive diagonal and the multigrid cycle
# on these problems give none; fl_poisson_create refuses kappa <= 0)
REACHED = (RTOL, ATOL, ITS, DIV_ITS, DIV_DTOL, DIV_NANORINF, DIV_INDEFINITE_MAT)
UNREACHED = (DIV_BREAKDOWN, DIV_INDEFINITE_PC)


# the CG cases whose stop leaves x-updates owed to the direction ring (the single-reduction CG keeps none)
def ring_cases():
    return [c for c in STOPS if c.part in "CF" and c.opts["type"] == CG and not c.opts.get("cg_single_reduction")]


def cases(part, handle=None):
    return [c for c in STOPS if c.part == part and (handle is None or c.handle == handle)]
