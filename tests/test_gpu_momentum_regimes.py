"""-m gpu: the momentum kernels in the launch plan that 256^3 - 512^3 grids take, against the oracle's assembled A.

k_mom3 (a state handed over with v0), k_mom2 (the stored fields; every state when ny <= 8) and k_mom_pw3 (the vector updates of BiCGStab and
Chebyshev) all walk the t2 tiling of fl_momentum_create: 128 x 8 tiles, z chunks, an XCD-contiguous block order when the blocks are a multiple
of 8.  The grids of tests/test_gpu_momentum*.py all take chunks of 3 - 15 planes, none of them short, in the plain block order.  The grids here
are the mom_* regimes of tests/launch_regimes.py (tests/test_launch_regimes.py checks on the CPU that each still takes its plan): chunks of 55
planes with a shorter last one, a last chunk of one plane, the remap on and off, x tiles of one column, y tiles of one row, periodic seams across
tiles and chunks.  Every grid is stretched in all three axes, so that no two columns, rows or planes share their numbers: a kernel that reads
the table entry of the wrong one is wrong here (tests/test_launch_regimes.py checks that on the CPU).  Fixed, small iteration counts: the
oracle's CSR Krylov loops are the cost."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import fluca_oracle as fo
from tests.gpu_common import dev, host
from tests.launch_regimes import BY_NAME, CAVITY, CHANNEL, REGIMES, SLAB, XPER, launch_plans
from tests.test_gpu_launch_regimes import handles  # noqa: F401  (the fixture)
from tests.test_gpu_momentum import _boundary_vbc, _close, _pair
from tests.test_gpu_momentum_cheb import _state

pytestmark = pytest.mark.gpu

MOM = [r for r in REGIMES if r.name.startswith("mom_")]
CASES = [(r, bc) for r in MOM for bc in r.bcs]
BCNAME = {tuple(CAVITY): "cavity", tuple(CHANNEL): "channel", tuple(XPER): "xper", tuple(SLAB): "slab"}
IDS = [f"{r.name}-{BCNAME[tuple(bc)]}" for r, bc in CASES]

# the oracle side of a (grid, boundary types) for the whole module: the state and A (3.5 M cells in all)
_PROBLEMS = {}


def _problem(reg, bc, g):
    """random V0 and v0 of a CFL / viscous state Chebyshev converges on, W = B v0 + vbc, A = I + dt C - (mu dt / 2 rho) L"""
    key = (reg.name, tuple(bc))
    if key not in _PROBLEMS:
        V0, v0, dt, rho, mu = _state(g, 0.5)
        vbc = _boundary_vbc(g, np.random.default_rng(29))
        W = [b + c for b, c in zip(g.apply_B(v0), vbc)]
        A = g.assemble_momentum(1.0, dt, -0.5 * mu * dt / rho, V0, W)
        _PROBLEMS[key] = SimpleNamespace(V0=V0, v0=v0, vbc=vbc, W=W, dt=dt, rho=rho, mu=mu, A=A)
    return _PROBLEMS[key]


def _open(hs, reg, bc):
    """(Momentum, oracle grid, problem) on the stretched grid of the regime, once its plan is checked to be the one the regime is meant to reach"""
    got = launch_plans(reg.n)
    wrong = {k: (v, got[k]) for k, v in reg.expect.items() if got[k] != v}
    assert not wrong, f"regime {reg.name} {reg.n} left its plan ({reg.reaches}); field: (expected, got) {wrong}"
    P, M, g = _pair(reg.n, bc, True)
    hs += [P, M]
    return M, g, _problem(reg, bc, g)


def _set_state(M, s, W, with_v0):
    M.set_state(s.dt, s.rho, s.mu, [dev(a) for a in s.V0], W, v0=dev(s.v0) if with_v0 else None)


def _block_ends(g, d):
    """mask of the faces at the ends of axis d in a face array of axis d: face 0, and face n[d] where the axis is not periodic"""
    shape = [g.n[2], g.n[1], g.n[0]]
    shape[2 - d] = g.nf[d]
    m = np.zeros(shape, dtype=bool)
    ends = [slice(None)] * 3
    for f in ((0,) if g.periodic[d] else (0, g.n[d])):
        ends[2 - d] = f
        m[tuple(ends)] = True
    return m.ravel()


@pytest.mark.parametrize("reg,bc", CASES, ids=IDS)
def test_products_match_the_assembled_rows(reg, bc, handles):  # noqa: F811
    """k_face_interp and k_face_interp_ends against B v0 + vbc; then apply, diagonal and row sums (A 1) against A.mult, A.diag: for the stored
    fields (k_mom2), the state with v0 (k_mom3; k_mom2 when ny = 8) and the state with v0 whose stored fields hold the block-end faces only"""
    M, g, s = _open(handles, reg, bc)
    A = s.A
    v = np.random.default_rng(11).standard_normal(3 * g.ncell)
    want = (A.mult(v), A.diag(), A.mult(np.ones(3 * g.ncell)))
    v0d, vbcd, vd = dev(s.v0), [dev(a) for a in s.vbc], dev(v)
    Wd = M.interp_faces(v0d, vbcd)
    for q in range(9):
        assert np.abs(host(Wd[q]) - s.W[q]).max() <= 2e-13 * max(1.0, np.abs(s.W[q]).max()), q
    # k_mom3 reads the stored fields on the block-end faces only; with ny <= 8 k_mom2 reads them whole, and the ends-only call writes them whole
    fly = reg.n[1] > 8
    junk = [torch.full((g.nface[d],), 1e300, dtype=torch.float64, device="cuda") for c in range(3) for d in range(3)]
    We = M.interp_faces(v0d, vbcd, ends_only=True, out=junk)
    for q in range(9):
        got, ends = host(We[q]), _block_ends(g, q % 3) if fly else np.ones(g.nface[q % 3], dtype=bool)
        assert np.abs(got[ends] - s.W[q][ends]).max() <= 2e-13 * max(1.0, np.abs(s.W[q]).max()), q
        assert np.all(got[~ends] == 1e300), q                                      # the inner entries are not written
    res = {}
    for name, W, with_v0 in (("stored", Wd, False), ("v0", Wd, True), ("ends", We, True)):
        _set_state(M, s, W, with_v0)
        res[name] = (host(M.apply(vd)), host(M.diagonal()), host(M.rowsum()))
        for got, w in zip(res[name], want):
            _close(got, w)
    # the same table numbers and the same two products per face value in the same order: the two kernels agree to the last rounding of the sums
    for got, w in zip(res["v0"], res["stored"]):
        assert np.abs(got - w).max() <= 4e-15 * np.abs(w).max()
    # and what the state with v0 does not read cannot change its products
    for got, w in zip(res["ends"], res["v0"]):
        assert np.array_equal(got, w)


@pytest.mark.parametrize("reg,bc", CASES, ids=IDS)
def test_gershgorin_bound_and_chebyshev_interval(reg, bc, handles):  # noqa: F811
    """OUT == 3 (the Jacobi-scaled row sums of |a_ij|) of both kernels, reduced over the grid: 1 + radius against the oracle's max_i sum_j |a_ij| / |a_ii|"""
    M, g, s = _open(handles, reg, bc)
    G = s.A.gershgorin(fo.PC_JACOBI)
    dmean = s.A.diag().mean()
    Wd = M.interp_faces(dev(s.v0), [dev(a) for a in s.vbc])
    for with_v0 in (False, True):
        _set_state(M, s, Wd, with_v0)
        radius = M.gershgorin()
        assert abs((1.0 + radius) - G) <= 1e-12 * G, (with_v0, radius, G)
        emin, emax = M.chebyshev_interval()
        assert emax == 1.0 + radius and abs(emin - max(1.0 - radius, 0.9 / dmean)) <= 1e-12, (with_v0, emin, emax)


def _state_with_v0(M, s):
    _set_state(M, s, M.interp_faces(dev(s.v0), [dev(a) for a in s.vbc]), True)


@pytest.mark.parametrize("reg,bc", CASES, ids=IDS)
@pytest.mark.parametrize("pc", [fo.PC_JACOBI, fo.PC_NONE], ids=["jacobi", "none"])
def test_bicgstab_iterates_match_the_oracle(reg, bc, pc, handles):  # noqa: F811
    """5 BiCGStab iterations: the products with their inner products (DOT partial sums over t2blocks) and k_mom_pw3's updates"""
    M, g, s = _open(handles, reg, bc)
    _state_with_v0(M, s)
    b = np.random.default_rng(7).standard_normal(3 * g.ncell)
    xo, io = s.A.solve(b, ksp=fo.KSP_BCGS, pc=pc, nullspace=False, rtol=0.0, atol=0.0, maxit=5)
    xg, ig = M.solve(dev(b), history=True, pc=pc, rtol=0.0, atol=0.0, maxit=5)
    assert ig["iters"] == io["iters"] == 5 and ig["reason"] == io["reason"], (ig, io["iters"], io["reason"])
    assert np.allclose(ig["history"], io["history"][:6], rtol=1e-9, atol=0), (ig["history"], io["history"])
    assert np.linalg.norm(host(xg) - xo) <= 1e-9 * np.linalg.norm(xo)


@pytest.mark.parametrize("reg,bc", CASES, ids=IDS)
def test_chebyshev_steps_match_the_oracle(reg, bc, handles):  # noqa: F811
    """KSPCHEBYSHEV + PCJACOBI, 12 steps on the default interval with the preconditioned norm (the step fused into k_mom3, OUT == 4, and k_cheb_fin over
    t2blocks; k_mom2 + k_mom_pw3 when ny = 8), then 7 unmonitored steps without a preconditioner on an explicit interval"""
    M, g, s = _open(handles, reg, bc)
    _state_with_v0(M, s)
    A = s.A
    b = np.random.default_rng(5).standard_normal(3 * g.ncell)
    emin, emax = M.chebyshev_interval()
    xo, io = A.solve(b, ksp=fo.KSP_CHEBYSHEV, pc=fo.PC_JACOBI, norm=fo.NORM_PRECONDITIONED, nullspace=False, rtol=0.0, atol=0.0, maxit=12,
                     emin=emin, emax=emax)
    xg, ig = M.solve(dev(b), type=fo.KSP_CHEBYSHEV, pc=fo.PC_JACOBI, norm_type=fo.NORM_PRECONDITIONED, rtol=0.0, atol=0.0, maxit=12, history=True,
                     check_every=5)
    assert ig["iters"] == io["iters"] == 12 and ig["reason"] == io["reason"], (ig, io["iters"], io["reason"])
    assert np.allclose(ig["history"], io["history"], rtol=1e-8, atol=1e-13 * io["history"][0]), (ig["history"], io["history"])
    assert np.linalg.norm(host(xg) - xo) <= 1e-9 * np.linalg.norm(xo)
    lam = A.gershgorin(fo.PC_NONE)
    xo, io = A.solve(b, ksp=fo.KSP_CHEBYSHEV, pc=fo.PC_NONE, norm=fo.NORM_NONE, nullspace=False, maxit=7, emin=0.1 * lam, emax=1.1 * lam)
    xg, ig = M.solve(dev(b), type=fo.KSP_CHEBYSHEV, pc=fo.PC_NONE, norm_type=fo.NORM_NONE, maxit=7, emin=0.1 * lam, emax=1.1 * lam)
    assert ig["iters"] == io["iters"] == 7 and ig["reason"] == io["reason"] == 4
    assert np.linalg.norm(host(xg) - xo) <= 1e-10 * np.linalg.norm(xo)


GUESS_CASES = [(r, bc) for r, bc in CASES if r in (BY_NAME["mom_three_tiles"], BY_NAME["mom_pairs_one_plane"])]


@pytest.mark.parametrize("reg,bc", GUESS_CASES, ids=[f"{r.name}-{BCNAME[tuple(bc)]}" for r, bc in GUESS_CASES])
def test_chebyshev_from_a_nonzero_guess(reg, bc, handles):  # noqa: F811
    """-ksp_initial_guess_nonzero: the fused step starts from x0 (y holds x_{k-1}).  The recurrence is affine, so 12 steps from x0 on b are x0 plus 12
    steps from zero on b - A x0: the oracle's iterates on the shifted system give the correction the GPU must have made."""
    M, g, s = _open(handles, reg, bc)
    _state_with_v0(M, s)
    A = s.A
    rng = np.random.default_rng(13)
    b, x0 = rng.standard_normal(3 * g.ncell), rng.standard_normal(3 * g.ncell)
    emin, emax = M.chebyshev_interval()
    do, io = A.solve(b - A.mult(x0), ksp=fo.KSP_CHEBYSHEV, pc=fo.PC_JACOBI, nullspace=False, rtol=0.0, atol=0.0, maxit=12, emin=emin, emax=emax)
    xg, ig = M.solve(dev(b), x=dev(x0), initial_guess_nonzero=1, type=fo.KSP_CHEBYSHEV, pc=fo.PC_JACOBI, rtol=0.0, atol=0.0, maxit=12,
                     history=True, check_every=5)
    assert ig["iters"] == io["iters"] == 12 and ig["reason"] == io["reason"], (ig, io["iters"], io["reason"])
    assert np.allclose(ig["history"], io["history"], rtol=1e-8, atol=1e-13 * io["history"][0]), (ig["history"], io["history"])
    assert np.linalg.norm((host(xg) - x0) - do) <= 1e-9 * np.linalg.norm(do)
