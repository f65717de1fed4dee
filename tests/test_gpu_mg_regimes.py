"""-m gpu: the multigrid-preconditioned CG (FL_PC_MG, fl_mg.hip) in the launch plans that 256^3 - 512^3 grids take, against the oracle's
restatement of the same cycle (MgOracle).

Every level of every grid of tests/test_gpu_mg.py takes the small_ry1 plan: there the one-pass residual + restriction (k_bcgs_st MODE 11) never
runs, k_mg_prolong_lin_cc has one x block and k_mg_restrict, k_mg_pwd and k_mg_dots take one grid-stride trip.  The mg_* regimes of
tests/launch_regimes.py and production_256 reach what the product runs at full size (tests/test_launch_regimes.py checks that on the CPU): the
one-pass kernel with 8 and with 4 waves, the two-pass fallback on an 8-wave level, k_mg_prolong_lin_cc with three x blocks and a partial last one
and a short last z chunk, k_mg_prolong_lin_tile<false> with a last z chunk of one plane, the grid-stride kernels over several trips and both
coarse solves.  Every case runs on a uniform grid and on one stretched in all three axes: on the uniform grid every restriction weight is 1/2
and every prolongation weight 1/4, so a kernel that reads the weight of the wrong cell is wrong only on the stretched one.

The cycle is a preconditioner, and a wrong one still converges: the iterates are compared after a fixed number of iterations."""
import numpy as np
import pytest

from oracle import fluca_oracle as fo
from tests.gpu_common import CAVITY_BOX, dev, host, mean_free_rhs
from tests.launch_regimes import CAVITY, CHANNEL, REGIMES, XPER
from tests.test_gpu_launch_regimes import _grid, _relmax, handles  # noqa: F401  (the fixture)
from tests.test_gpu_mg import _bounds

pytestmark = pytest.mark.gpu

MG = [r for r in REGIMES if r.mg]
BCNAME = {tuple(CAVITY): "cavity", tuple(CHANNEL): "channel", tuple(XPER): "xper"}
CASES = [(r, bc, s) for r in MG for bc in r.bcs for s in (False, True)]
IDS = [f"{r.name}-{BCNAME[tuple(bc)]}-{'stretched' if s else 'uniform'}" for r, bc, s in CASES]

TOL = 1e-10          # x_1 .. x_3 and the residual norms, relative: the bound of the CG regime tests (tests/test_gpu_launch_regimes.py)
COARSE_RTOL = 1e-2   # the coarsest level's Jacobi-PCG stops there (vcycle, MgOracle.vcycle)

# the oracle side of one case at a time (the hierarchy of a 17 M-cell grid: about 3 GB)
_LAST = {}


def _problem(reg, bc, stretched):
    """(MgOracle with the product's eigenvalue bounds and tri-linear prolongation, right-hand side b = S p, whether S has a null space)"""
    key = (reg.name, tuple(bc), stretched)
    if _LAST.get("key") != key:
        _LAST.clear()
        g = _grid(reg.n, bc, stretched)
        ns = fo.BC_PRESSURE_OUTLET not in bc
        mg = fo.MgOracle(g, nullspace=ns, prolong="linear", record_coarse=True)
        mg.bounds = _bounds(mg)
        _, b = mean_free_rhs(mg.S[0], g.ncell)
        _LAST.update(key=key, mg=mg, b=b, ns=ns)
    return _LAST["mg"], _LAST["b"], _LAST["ns"]


def _open(hs, g, stretched):
    from fluca_amd.poisson import Poisson
    hs.append(Poisson(g.n, g.xf, g.bc, g.kappa) if stretched else Poisson.uniform(g.n, CAVITY_BOX, g.bc, g.kappa))
    return hs[-1]


def _mg_solve(P, bd, ns, **kw):
    x, info = P.solve(bd, history=True, type=0, pc=2, remove_nullspace=int(ns), **kw)
    return host(x), info


def _knob(name, value):
    from fluca_amd import capi
    capi.check(capi.lib.fl_tuning_set(name.encode(), value))


@pytest.mark.parametrize("reg,bc,stretched", CASES, ids=IDS)
def test_mg_pcg_iterates_match_oracle(reg, bc, stretched, handles):  # noqa: F811
    """x after 1, 2 and 3 MG-PCG iterations and the residual norms, element by element against MgOracle.  The coarsest solves of the oracle stop
    far enough from their tolerance that a device that rounds differently takes the same number of iterations there.  The three smoothing steps
    from zero in one sweep (cheb_zero3 = 1, the default) give the x_3 of the separate first step.  And the comparison sees a change of the cycle:
    the piecewise-constant prolongation (mg_prolong = 0) misses the oracle's tri-linear x_1 by far more than the tolerance."""
    mg, b, ns = _problem(reg, bc, stretched)
    assert [g.n for g in mg.grids] == [lv["n"] for lv in reg.mg]
    P = _open(handles, mg.grids[0], stretched)
    xs = []
    mg.coarse_stops.clear()
    _, io = mg.pcg(b, rtol=0.0, atol=0.0, maxit=3, iterates=xs)
    assert io["iters"] == 3 and io["reason"] == -3 and len(xs) == 3
    assert len(mg.coarse_stops) == 4                     # one coarsest solve per cycle
    margin = min(abs(q / COARSE_RTOL - 1.0) for _, qs in mg.coarse_stops for q in qs)
    bd = dev(b)
    dx, dh, xg = [], [], {}
    for k in (1, 2, 3):
        xg[k], info = _mg_solve(P, bd, ns, rtol=0.0, atol=0.0, maxit=k)
        assert info["iters"] == k and info["reason"] == -3, (k, info["iters"], info["reason"])
        dx.append(_relmax(xg[k], xs[k - 1]))
        dh.append(float(np.abs(info["history"] / io["history"][:k + 1] - 1.0).max()))
    try:
        _knob("cheb_zero3", 0)
        zero3 = _relmax(_mg_solve(P, bd, ns, rtol=0.0, atol=0.0, maxit=3)[0], xg[3])
        _knob("cheb_zero3", 1)
        _knob("mg_prolong", 0)
        miss = _relmax(_mg_solve(P, bd, ns, rtol=0.0, atol=0.0, maxit=1)[0], xs[0])
    finally:
        _knob("cheb_zero3", 1)
        _knob("mg_prolong", 1)
    print(f"\n[mg] {reg.name} {BCNAME[tuple(bc)]} {'stretched' if stretched else 'uniform'}: x_k {['%.2e' % d for d in dx]} "
          f"history {['%.2e' % d for d in dh]} coarse-stop margin {margin:.3e} (reasons {[r for r, _ in mg.coarse_stops]}) "
          f"cheb_zero3 {zero3:.2e} constant-prolongation miss {miss:.2e}")
    assert margin >= 1e-6, mg.coarse_stops
    assert max(dx) <= TOL and max(dh) <= TOL, (dx, dh)
    assert zero3 <= 1e-10, zero3
    assert miss >= 100 * TOL, miss


@pytest.mark.parametrize("reg", MG, ids=[r.name for r in MG])
def test_mg_pcg_converges_like_the_oracle(reg, handles):  # noqa: F811
    """a solve to rtol 1e-8 on the uniform grid: the iteration count of the oracle within one, and an answer that solves the system"""
    mg, b, ns = _problem(reg, reg.bcs[0], False)
    P = _open(handles, mg.grids[0], False)
    xo, io = mg.pcg(b, rtol=1e-8, maxit=100)
    xg, ig = _mg_solve(P, dev(b), ns, rtol=1e-8, maxit=100)
    res = np.linalg.norm(b - mg.S[0].mult(xg)) / np.linalg.norm(b)
    print(f"\n[mg] {reg.name} converged: {ig['iters']} iterations (oracle {io['iters']}), ||b - S x|| / ||b|| = {res:.2e}, "
          f"x against the oracle's {np.linalg.norm(xg - xo) / np.linalg.norm(xo):.2e}")
    assert ig["reason"] == io["reason"] == 2 and abs(ig["iters"] - io["iters"]) <= 1, (ig["iters"], io["iters"], ig["reason"], io["reason"])
    assert res <= 1e-6, res
