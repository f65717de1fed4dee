"""-m gpu: the hot kernels in the launch plans the product runs at 256^3 - 512^3, against the CPU oracle.

The grids are those of tests/launch_regimes.py (tests/test_launch_regimes.py checks on the CPU that each still reaches its plan): 8-wave
tiles whose last tile is partial in x and y, ragged z chunks, periodic seams that join a partial tile to tile 0 or cross a chunk seam,
k_project_six waves that take several grid-stride trips, k_schur_var at its full 128 blocks per XCD with and without a fixed x segment.
The toy grids of the other parity tests reach none of these."""
import numpy as np
import pytest

from oracle import fluca_oracle as fo
from tests.gpu_common import CAVITY_BOX, dev, host, mean_free_rhs, stretched_faces
from tests.launch_regimes import BY_NAME, CAVITY, CHANNEL, XPER, launch_plans, six_trips

pytestmark = pytest.mark.gpu

STD, MID = BY_NAME["cg_standard_ragged"], BY_NAME["cg_mid_ragged"]
BCNAME = {tuple(CAVITY): "cavity", tuple(CHANNEL): "channel", tuple(XPER): "xper"}

# one oracle grid and one assembled S per (grid, boundary types) for the whole module (16.8 M cells: 1.3 s and 2 s to build on 8 threads)
_GRIDS, _MATS = {}, {}


def _grid(n, bc, stretched=False):
    """stretched: the faces of stretched_faces (every axis stretched towards both ends) instead of the uniform cavity box"""
    key = (tuple(n), tuple(bc)) + (("stretched",) if stretched else ())
    if key not in _GRIDS:
        _GRIDS[key] = fo.Grid(n, stretched_faces(n), bc, 1e-3) if stretched else fo.Grid.uniform(n, CAVITY_BOX, bc, 1e-3)
    return _GRIDS[key]


def _S(n, bc):
    key = (tuple(n), tuple(bc))
    if key not in _MATS:
        _MATS[key] = _grid(n, bc).assemble_S()
    return _MATS[key]


@pytest.fixture
def handles():
    """the handles a test opens, closed when it ends, passed or failed"""
    hs = []
    yield hs
    for h in reversed(hs):
        h.close()


def _poisson(hs, n, bc, kappa=1e-3):
    from fluca_amd.poisson import Poisson
    hs.append(Poisson.uniform(n, CAVITY_BOX, bc, kappa))
    return hs[-1]


def _relmax(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def _id(reg, bc, *rest):
    return "-".join([reg.name, BCNAME[tuple(bc)]] + [str(r) for r in rest])


CG_CASES = [(STD, CAVITY, fo.PC_JACOBI), (STD, CAVITY, fo.PC_NONE), (STD, XPER, fo.PC_JACOBI), (MID, CHANNEL, fo.PC_JACOBI), (MID, XPER, fo.PC_JACOBI)]


@pytest.mark.parametrize("reg,bc,pc", CG_CASES, ids=[_id(*c) for c in CG_CASES])
def test_cg_iterates_match_oracle(reg, bc, pc, handles):
    """k_cg_A + k_cg_Bq on the 8-wave plans: x after 1, 2, 3, 8, 11 iterations (odd and even: the x-updates are batched in pairs), the first
    residual norms, and a converged solve."""
    assert launch_plans(reg.n)["cg.nw"] == 8
    g, S = _grid(reg.n, bc), _S(reg.n, bc)
    nullspace = fo.BC_PRESSURE_OUTLET not in bc
    _, b = mean_free_rhs(S, g.ncell)
    P = _poisson(handles, reg.n, bc)
    bd = dev(b)
    kw = dict(pc=pc, remove_nullspace=int(nullspace))
    for k in (1, 2, 3, 8, 11):
        xo, io = S.solve(b, pc=pc, nullspace=nullspace, rtol=0.0, atol=0.0, maxit=k, history=False)
        xg, ig = P.solve(bd, rtol=0.0, atol=0.0, maxit=k, **kw)
        assert ig["iters"] == io["iters"] == k and ig["reason"] == io["reason"] == -3, (k, ig, io["iters"], io["reason"])
        assert _relmax(host(xg), xo) <= 1e-10, (k, _relmax(host(xg), xo))
    if pc == fo.PC_JACOBI and not (reg is MID and bc == XPER):   # a converged solve (167 - 236 iterations) on all but one Jacobi case
        xo, io = S.solve(b, pc=pc, nullspace=nullspace, rtol=1e-6, maxit=5000)
        xg, ig = P.solve(bd, rtol=1e-6, maxit=5000, history=True, **kw)
        assert ig["reason"] == io["reason"] == 2 and abs(ig["iters"] - io["iters"]) <= 1, (ig["iters"], io["iters"])
        assert np.allclose(ig["history"][:5], io["history"][:5], rtol=1e-9, atol=0)
        assert np.linalg.norm(b - S.mult(host(xg))) <= 1.5 * np.linalg.norm(b - S.mult(xo)) + 1e-12 * np.linalg.norm(b)
    else:
        _, io = S.solve(b, pc=pc, nullspace=nullspace, rtol=0.0, atol=0.0, maxit=5)
        _, ig = P.solve(bd, rtol=0.0, atol=0.0, maxit=5, history=True, **kw)
        assert np.allclose(ig["history"][:6], io["history"][:6], rtol=1e-9, atol=0)
    # the operator alone: k_apply against the assembled rows
    p = np.random.default_rng(7).standard_normal(g.ncell)
    y = S.mult(p)
    assert np.abs(host(P.apply(dev(p))) - y).max() <= 1e-12 * np.abs(y).max()


CHEB_CASES = [(STD, XPER), (MID, CHANNEL)]


@pytest.mark.parametrize("reg,bc", CHEB_CASES, ids=[_id(*c) for c in CHEB_CASES])
def test_fused_chebyshev_matches_oracle(reg, bc, handles):
    """k_cheb2 in its clamped plan (the default cheb_fuse picks it on these grids) and, for the odd step, k_cheb_st on the 8-wave tiles:
    7 steps (three fused pairs and a single step) and 20, against the oracle's KSPCHEBYSHEV + PCJACOBI."""
    assert launch_plans(reg.n)["cheb2.clamp"] == 1
    g, S = _grid(reg.n, bc), _S(reg.n, bc)
    nullspace = fo.BC_PRESSURE_OUTLET not in bc
    if nullspace:
        _, b = mean_free_rhs(S, g.ncell)
    else:
        b = np.random.default_rng(5).standard_normal(g.ncell)
    lam = S.gershgorin(fo.PC_JACOBI)
    emin, emax = 0.1 * lam, 1.1 * lam
    P = _poisson(handles, reg.n, bc)
    for steps in (7, 20):
        xo, io = S.solve(b, ksp=fo.KSP_CHEBYSHEV, pc=fo.PC_JACOBI, norm=fo.NORM_NONE, nullspace=nullspace, maxit=steps, emin=emin, emax=emax,
                         history=False)
        xg, ig = P.solve(dev(b), type=2, pc=fo.PC_JACOBI, norm_type=fo.NORM_NONE, remove_nullspace=int(nullspace), maxit=steps, emin=emin,
                         emax=emax, check_every=100, profile=1)
        assert ig["reason"] == io["reason"] == 4 and ig["iters"] == io["iters"] == steps
        assert ig["kernel_launches"] == steps // 2, ig                  # the fused kernel ran: one launch per pair of steps
        assert _relmax(host(xg), xo) <= 1e-12, (steps, _relmax(host(xg), xo))


def test_bicgstab_history_on_the_mid_plan(handles):
    """Jacobi-BiCGStab (k_bcgs_pw on tile_plan, the stencil sweeps on the mid plan of plan_cg_A): 5 iterations against the oracle."""
    reg, bc = MID, CHANNEL
    g, S = _grid(reg.n, bc), _S(reg.n, bc)
    b = np.random.default_rng(9).standard_normal(g.ncell)
    xo, io = S.solve(b, ksp=fo.KSP_BCGS, pc=fo.PC_JACOBI, nullspace=False, rtol=0.0, atol=0.0, maxit=5)
    P = _poisson(handles, reg.n, bc)
    xg, ig = P.solve(dev(b), type=1, pc=fo.PC_JACOBI, remove_nullspace=0, rtol=0.0, atol=0.0, maxit=5, history=True, check_every=5)
    assert ig["iters"] == io["iters"] == 5 and ig["reason"] == io["reason"], (ig, io["iters"], io["reason"])
    m = min(len(ig["history"]), len(io["history"]))
    assert m >= 5 and np.allclose(ig["history"][:m], io["history"][:m], rtol=1e-9, atol=0)


PROJ_CASES = [(STD, XPER), (MID, CHANNEL)]


@pytest.mark.parametrize("reg,bc", PROJ_CASES, ids=[_id(*c) for c in PROJ_CASES])
def test_projection_of_all_six_arrays_over_several_trips(reg, bc, handles):
    """k_project_six where a wave walks the grid stride more than once (1.3 and 5.1 trips): against Gst p and G p of the oracle, and bit for bit
    against k_project_all on subsets of the arrays (tests/test_gpu_poisson.py::test_projection_of_all_six_arrays at toy sizes)."""
    assert six_trips(launch_plans(reg.n)) > 1
    g = _grid(reg.n, bc)
    P = _poisson(handles, reg.n, bc)
    rng = np.random.default_rng(11)
    p = rng.standard_normal(g.ncell)
    Vf = [rng.standard_normal(nf) for nf in g.nface]
    vs = [rng.standard_normal(g.ncell) for _ in range(3)]
    Vd, vd = [dev(a) for a in Vf], [dev(a) for a in vs]
    P.project(dev(p), v=vd, V=Vd)
    Gst = g.apply_gst(p)
    for d in range(3):
        ref = Vf[d] - Gst[d]
        assert abs(host(Vd[d]) - ref).max() <= 1e-12 * max(1.0, abs(ref).max()), d
    del Gst
    Gc = g.apply_G(p)
    for d in range(3):
        ref = vs[d] - Gc[d]
        assert abs(host(vd[d]) - ref).max() <= 1e-12 * max(1.0, abs(ref).max()), d
    del Gc
    V2, v2 = [dev(a) for a in Vf], [dev(a) for a in vs]
    P.project(dev(p), v=(v2[0], None, None), V=(None, V2[1], None))
    P.project(dev(p), v=(None, v2[1], v2[2]), V=(V2[0], None, V2[2]))
    for d in range(3):
        assert np.array_equal(host(V2[d]), host(Vd[d])), d
        assert np.array_equal(host(v2[d]), host(vd[d])), d


SCHUR_CASES = [(STD, XPER), (BY_NAME["schur_fixed_seg"], CAVITY), (BY_NAME["schur_general"], XPER)]


@pytest.mark.parametrize("reg,bc", SCHUR_CASES, ids=[_id(*c) for c in SCHUR_CASES])
def test_schur_complement_at_128_blocks_per_xcd(reg, bc, handles):
    """k_schur_var (DIAG and ROWSUM) at its full launch of 128 blocks per XCD: against the oracle's composition fo.abf_schur_apply and the
    seven-kernel composition of the device (schur_var_fused = 0)."""
    from fluca_amd import capi
    from fluca_amd.poisson import Momentum
    assert launch_plans(reg.n)["schur.per_xcd"] == 128
    g = _grid(reg.n, bc)
    P = _poisson(handles, reg.n, bc)
    M = Momentum(P)
    handles.append(M)
    # a momentum state whose row sums stay away from zero: the device forms diag(A) and A 1 itself, in another order than the oracle, and near a
    # zero row sum that rounding is amplified by 1 / a (the random fields of tests/test_gpu_momentum.py put row sums within 1e-5 of zero on grids
    # this large).  The convective part of a row sum grows like |V0| / h: the amplitude follows the finest spacing.
    amp = 75 * min((hi - lo) / m for (lo, hi), m in zip(CAVITY_BOX, reg.n))
    rng = np.random.default_rng(3)
    V0 = [amp * rng.standard_normal(g.nface[d]) for d in range(3)]
    W = [amp * rng.standard_normal(g.nface[d]) for c in range(3) for d in range(3)]
    dt, rho, mu = g.kappa, 1.0, 0.05
    M.set_state(dt, rho, mu, [dev(a) for a in V0], [dev(a) for a in W])
    A = g.assemble_momentum(1.0, dt, -0.5 * mu * dt / rho, V0, W)
    del V0, W
    ainvs = {kind: fo.abf_ainv(A, kind) for kind in (fo.AINV_DIAG, fo.AINV_ROWSUM)}
    del A
    p = np.random.default_rng(17).standard_normal(g.ncell)
    pd = dev(p)
    for kind, ainv in ainvs.items():
        assert np.abs(1.0 / ainv).min() >= 0.25 and np.abs(1.0 / ainv - 1.0).max() > 1e-2, kind   # well conditioned, and not the ID type
        M.set_ainv_types(schur=kind)
        want = fo.abf_schur_apply(g, ainv, p)
        got = host(M.schur_apply(pd))
        assert _relmax(got, want) <= 2e-10, (kind, _relmax(got, want))
        capi.check(capi.lib.fl_tuning_set(b"schur_var_fused", 0))
        try:
            comp = host(M.schur_apply(pd))
        finally:
            capi.check(capi.lib.fl_tuning_set(b"schur_var_fused", 1))
        assert _relmax(got, comp) <= 1e-12, (kind, _relmax(got, comp))
