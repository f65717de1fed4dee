"""-m gpu: the DIAG / ROWSUM Schur product S p = D ((-T) a^-1 kappa G - (-R)) p (abfpc.c:151-171) formed in ONE pass on several ranks
(k_schur_var_ring, fl_schur_var.hip): the two-deep ghost layers of p, the ring of a^-1 and the widened 1-D rows make a rank's product the
one-rank product of the global grid bit for bit.  In-process rank grids (tests/inproc.py): one handle per rank on its own thread, in-memory wire."""
import ctypes as C

import numpy as np
import pytest

from oracle import fluca_oracle as fo
from tests import inproc
from tests import interior_ranks
from tests.gpu_common import O, PER, SYM, V, stretched_faces

pytestmark = pytest.mark.gpu

BOX = [(0.0, 1.0), (0.0, 1.0), (0.0, 0.5)]

# (n, rank grid, ownership ranges, boundary types): uneven splits; every case puts walls / outlets / symmetry planes / a split periodic axis on
# rank faces
CASES = [
    ((13, 9, 8), (2, 1, 1), ([5, 8], [9], [8]), [PER, PER, V, O, SYM, V]),            # x periodic across the two ranks (same peer on both sides)
    ((9, 13, 11), (1, 2, 2), ([9], [6, 7], [4, 7]), [V, O, SYM, V, PER, PER]),         # y split between a symmetry plane and a wall, z periodic split
    ((12, 11, 10), (2, 2, 2), ([5, 7], [6, 5], [3, 7]), [O, V, SYM, O, PER, PER]),     # config 5's rank grid
    # three ranks on each axis in turn (tests/interior_ranks.py): the ring of a^-1 and the widened rows of the middle block come from two owners
    *interior_ranks.SCHUR,
]
STALE = (2, 5)      # the cases that go on to a second momentum state on the same handles


def _knob(name, value):
    from fluca_amd import capi
    capi.check(capi.lib.fl_tuning_set(name.encode(), int(value)))


class _Problem:
    def __init__(self, n, ranks, own, bc):
        self.n, self.ranks, self.own, self.bc = n, ranks, own, bc
        self.xf = stretched_faces(n, BOX)
        self.g = fo.Grid(n, self.xf, bc, 1e-3)
        self.periodic = [bc[0] == PER, bc[2] == PER, bc[4] == PER]
        g = self.g
        self.shp = (n[2], n[1], n[0])
        self.fshape = [(n[2], n[1], g.nf[0]), (n[2], g.nf[1], n[0]), (g.nf[2], n[1], n[0])]
        rng = np.random.default_rng(41)
        self.V0 = [8.0 * rng.standard_normal(g.nface[d]) for d in range(3)]
        self.W = [8.0 * rng.standard_normal(g.nface[d]) for c in range(3) for d in range(3)]
        self.p = rng.standard_normal(g.ncell)
        self.mu = 0.05
        self.states = [(g.kappa, 1.0), (3.0 * g.kappa, 1.3)]   # (dt, rho): the second is the "next time step" of the stale-ring check

    def A(self, s):
        dt, rho = self.states[s]
        return self.g.assemble_momentum(1.0, dt, -0.5 * self.mu * dt / rho, self.V0, self.W)

    def decomp(self, rank):
        from fluca_amd import capi
        from tests import mp_common as mpc
        if rank is None:
            return None
        d = mpc.decomp_of(capi, self.n, self.ranks, rank)
        for a in range(3):
            d.len[a] = self.own[a][d.coord[a]]
            d.lo[a] = sum(self.own[a][:d.coord[a]])
        return d


def _blocks(pb, d):
    from tests import mp_common as mpc
    if d is None:
        return (lambda a: np.ascontiguousarray(a), lambda a, ax: np.ascontiguousarray(a))
    cell = lambda a: np.ascontiguousarray(a.reshape(pb.shp)[mpc.block(d)]).ravel()
    face = lambda a, ax: np.ascontiguousarray(a.reshape(pb.fshape[ax])[mpc.face_block(d, ax, pb.periodic)]).ravel()
    return cell, face


def _session(R, pb, rank):
    """this rank's Poisson + Momentum (R None: the undecomposed grid) on its own stream"""
    import torch
    from fluca_amd.poisson import Momentum, Poisson
    d = pb.decomp(rank)
    P = Poisson(pb.n, pb.xf, pb.bc, pb.g.kappa, decomp=d)
    s = torch.cuda.Stream()
    P.set_stream(s)
    if R is not None:
        R.attach(P.h)
    return P, Momentum(P), d, s


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")


def _product_worker(R, pb, kind, nstates):
    """S p of this rank's block for the states 0 .. nstates-1, one after the other on the same handle"""
    import torch
    P, M, d, s = _session(R, pb, None if R is None else R.rank)
    cell, face = _blocks(pb, d)
    out = []
    with torch.cuda.stream(s):
        M.set_ainv_types(schur=kind)
        for st in range(nstates):
            dt, rho = pb.states[st]
            M.set_state(dt, rho, pb.mu, [_dev(face(pb.V0[a], a)) for a in range(3)], [_dev(face(pb.W[c * 3 + a], a)) for c in range(3) for a in range(3)])
            y = M.schur_apply(_dev(cell(pb.p)))
            a = M.diagonal() if kind == fo.AINV_DIAG else M.rowsum()      # what a^-1 is the reciprocal of
            s.synchronize()
            out.append(y.cpu().numpy())
            a = a.cpu().numpy()
            out.extend(a.reshape(3, -1))
    M.close()
    P.close()
    lo = [0, 0, 0] if d is None else [d.lo[a] for a in range(3)]
    ln = list(pb.n) if d is None else [d.len[a] for a in range(3)]
    return dict(lo=lo, ln=ln, y=out)


def _gather(pb, parts, st):
    """the blocks of entry st of the ranks' lists -> the global array"""
    y = np.full(pb.shp, np.nan)
    for r in parts:
        lo, ln = r["lo"], r["ln"]
        y[lo[2]:lo[2] + ln[2], lo[1]:lo[1] + ln[1], lo[0]:lo[0] + ln[0]] = r["y"][st].reshape(ln[2], ln[1], ln[0])
    assert not np.isnan(y).any(), "the blocks do not tile the grid"
    return y.ravel()


def _run(pb, kind, nstates, fused):
    """per state: the gathered S p and the three components of diag(A) / A 1"""
    size = int(np.prod(pb.ranks))
    _knob("schur_var_fused", fused)
    try:
        multi = inproc.run_threads(size, _product_worker, pb, kind, nstates)
    finally:
        _knob("schur_var_fused", 1)
    return [[_gather(pb, multi, 4 * st + c) for c in range(4)] for st in range(nstates)]


def _same_bits(pb, got, one):
    """got == one bit for bit wherever the inputs are: the momentum diagonal / row sums (k_mom*, not part of this product) of a rank's block may
    differ from the undecomposed grid's in the last bit (the launch plan follows the block's shape); S p of a cell reads a^-1 of its neighbours
    along each axis, so the cells next to such an entry are held to 1e-15 relative instead.  Returns the number of such cells."""
    y, ya = got[0], one[0]
    moved = np.zeros(pb.shp, dtype=bool)
    for c in range(3):
        m = (got[1 + c] != one[1 + c]).reshape(pb.shp)
        moved |= m | np.roll(m, 1, axis=2 - c) | np.roll(m, -1, axis=2 - c)
    moved = moved.ravel()
    assert moved.sum() <= pb.g.ncell // 4, moved.sum()                  # most cells are compared bit for bit
    assert np.array_equal(y[~moved], ya[~moved]), np.abs(y - ya)[~moved].max()
    assert np.abs(y - ya).max() <= 1e-15 * np.abs(ya).max()
    return int(moved.sum())


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("kind", [fo.AINV_DIAG, fo.AINV_ROWSUM])
def test_decomposed_fused_product_equals_the_one_rank_product_bit_for_bit(case, kind):
    """The gathered product of the ranks == the one-rank fused product of the global grid, bit for bit wherever a^-1 is (_same_bits); the
    composition of seven kernels on the same ranks differs from it in round-off only; both match the oracle's dense S.  Then another momentum state on the same handles (the next
    time step): the product follows it -- the ring of a^-1 is not stale."""
    pb = _Problem(*CASES[case])
    nst = 2 if case in STALE else 1
    one = _product_worker(None, pb, kind, nst)["y"]
    one = [one[4 * st:4 * st + 4] for st in range(nst)]
    fused = _run(pb, kind, nst, 1)
    comp = _run(pb, kind, 1, 0)[0][0]
    moved = _same_bits(pb, fused[0], one[0])
    print(f"case {case} {pb.n} on {pb.ranks}, kind {kind}: {moved} of {pb.g.ncell} cells held to 1e-15, the others bit for bit")
    assert not np.array_equal(comp, fused[0][0])                     # the composition on the same ranks: another order of the same sums
    scale = np.abs(one[0][0]).max()
    assert np.abs(comp - one[0][0]).max() <= 1e-12 * scale
    ainv = fo.abf_ainv(pb.A(0), kind)
    assert np.abs(1.0 / ainv - 1.0).max() > 1e-2
    want = fo.abf_schur_dense(pb.g, ainv) @ pb.p
    assert np.abs(fused[0][0] - want).max() <= 2e-10 * np.abs(want).max()
    if nst > 1:
        assert np.abs(one[1][0] - one[0][0]).max() > 1e-3 * scale          # the second state changes S
        _same_bits(pb, fused[1], one[1])
        want = fo.abf_schur_apply(pb.g, fo.abf_ainv(pb.A(1), kind), pb.p)
        assert np.abs(fused[1][0] - want).max() <= 2e-10 * np.abs(want).max()


def _solve_worker(R, pb, rhs):
    """PCApply_ABF with schurainv = DIAG: this rank's p and the Schur solve's iterations"""
    import torch
    from fluca_amd import capi
    from fluca_amd.poisson import KspOptions
    P, M, d, s = _session(R, pb, R.rank)
    cell, face = _blocks(pb, d)
    with torch.cuda.stream(s):
        dt, rho = pb.states[0]
        M.set_state(dt, rho, pb.mu, [_dev(face(pb.V0[a], a)) for a in range(3)], [_dev(face(pb.W[c * 3 + a], a)) for c in range(3) for a in range(3)])
        M.set_ainv_types(schur=fo.AINV_DIAG)
        v, Vf, p, info = M.abf_apply(_dev(np.concatenate([cell(c) for c in rhs.reshape(3, -1)])),
                                     momentum=KspOptions(type=capi.KSP_BCGS, rtol=1e-12, maxit=500), schur=KspOptions(rtol=1e-10, maxit=400, remove_nullspace=0))
        s.synchronize()
        y = p.cpu().numpy()
    M.close()
    P.close()
    return dict(lo=[d.lo[a] for a in range(3)], ln=[d.len[a] for a in range(3)], y=[y], info=info[1])


def test_diag_schur_solve_on_the_2x2x2_rank_grid():
    """schur_solve_var (flexible GMRES on S, the ID Schur solve as preconditioner) to rtol 1e-10 on config 5's rank grid with the fused
    product: the oracle's single-domain answer to 1e-6, and the iterations of the same solve with the composition, within one."""
    pb = _Problem(*CASES[2])
    rhs = np.random.default_rng(8).standard_normal(3 * pb.g.ncell)
    runs = []
    for fused in (1, 0):
        _knob("schur_var_fused", fused)
        try:
            parts = inproc.run_threads(8, _solve_worker, pb, rhs)
        finally:
            _knob("schur_var_fused", 1)
        assert all(r["info"]["reason"] > 0 for r in parts), parts[0]["info"]
        runs.append((_gather(pb, parts, 0), parts[0]["info"]["iters"]))
    A = pb.A(0)
    vs, _ = A.solve(rhs, ksp=fo.KSP_BCGS, pc=fo.PC_JACOBI, nullspace=False, rtol=1e-12, maxit=500)
    srhs = pb.g.rhs(*pb.g.apply_T(vs))
    po = np.linalg.solve(fo.abf_schur_dense(pb.g, fo.abf_ainv(A, fo.AINV_DIAG)), srhs)
    assert np.linalg.norm(runs[0][0] - po) <= 1e-6 * np.linalg.norm(po)
    assert abs(runs[0][1] - runs[1][1]) <= 1, (runs[0][1], runs[1][1])


# ------------------------------------------------------------------------------------------------ two time steps through the C host mirror

def _step_run(R, n, ranks):
    """NSSolve of the C host mirror, -ns_pc_abf_schur_ainv_type diag: a channel with a VELOCITY inlet, an outlet, walls in y and a periodic
    span; two steps.  R None: one rank."""
    from fluca_amd import capi, hostapi as H
    P = C.c_void_p
    L = (1.5, 1.0, 0.75)
    rank, size = (0, 1) if R is None else (R.rank, R.size)
    rk = ranks if size > 1 else (1, 1, 1)
    mesh = P()
    assert H.lib.MeshCartCreate3d(0, 0, 1, n[0], n[1], n[2], rk[0], rk[1], rk[2], None, None, None, C.byref(mesh)) == 0
    assert H.lib.MeshSetRank(mesh, rank, size) == 0
    assert H.lib.MeshSetUp(mesh) == 0
    assert H.lib.MeshCartSetUniformCoordinates(mesh, 0., L[0], 0., L[1], 0., L[2]) == 0
    ns = P()
    assert H.lib.NSCreate(C.byref(ns)) == 0 and H.lib.NSSetType(ns, b"cnlinear") == 0 and H.lib.NSSetMesh(ns, mesh) == 0
    assert H.lib.NSSetDensity(ns, 1.0) == 0 and H.lib.NSSetViscosity(ns, 0.05) == 0

    @H.BCFunc
    def inlet(dim, t, x, val, ctx):
        val[0], val[1], val[2] = 4.0 * x[1] * (L[1] - x[1]) / L[1] ** 2 * (1.0 + 0.3 * np.sin(2 * np.pi * x[2] / L[2])), 0.0, 0.0
        return 0

    @H.BCFunc
    def wall(dim, t, x, val, ctx):
        val[0] = val[1] = val[2] = 0.0
        return 0

    @H.BCFunc
    def outlet(dim, t, x, val, ctx):
        val[0] = 0.1 * x[1]
        return 0

    bcs = [H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=inlet), H.NSBoundaryCondition(type=H.NS_BC_PRESSURE_OUTLET, pressure=outlet),
           H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=wall), H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=wall),
           H.NSBoundaryCondition(type=H.NS_BC_PERIODIC), H.NSBoundaryCondition(type=H.NS_BC_PERIODIC)]
    for b in range(6):
        assert H.lib.NSSetBoundaryCondition(ns, b, bcs[b]) == 0
    argc, av = H.argv("-ns_time_step_size", 5e-3, "-ns_max_steps", 2, "-ns_ksp_rtol", 1e-10, "-ns_abf_schur_ksp_rtol", 1e-12, "-ns_abf_momentum_ksp_rtol", 1e-12,
                      "-ns_pc_abf_schur_ainv_type", "diag", "-ns_pc_abf_upper_ainv_type", "diag")
    assert H.lib.NSSetFromOptions(ns, argc, av) == 0 and H.lib.NSSetUp(ns) == 0
    hp = P()
    assert H.lib.NSGetPoisson(ns, C.byref(hp)) == 0
    if R is not None:
        R.attach(hp)
    assert H.lib.NSSolve(ns) == 0
    sz = (C.c_int64 * 4)()
    assert H.lib.NSGetLocalSizes(ns, sz) == 0
    cc = [C.c_int64() for _ in range(6)]
    assert H.lib.MeshCartGetCorners(mesh, *[C.byref(q) for q in cc]) == 0
    v, p, Vp = P(), P(), (C.c_void_p * 3)()
    assert H.lib.NSGetSolutionArrays(ns, C.byref(v), Vp, C.byref(p)) == 0

    def get(ptr, m):
        out = np.empty(m)
        capi.check(capi.lib.fl_memcpy_d2h(0, out.ctypes.data_as(C.c_void_p), ptr, m * 8))
        return out

    res = dict(lo=[q.value for q in cc[:3]], ln=[q.value for q in cc[3:]], v=get(v, 3 * sz[0]), p=get(p, sz[0]))
    H.lib.NSDestroy(C.byref(ns))
    H.lib.MeshDestroy(C.byref(mesh))
    return res


def test_two_diag_time_steps_on_two_ranks_match_one_rank():
    """Two NSSteps with -ns_pc_abf_schur_ainv_type diag (and the upper factor's DIAG) on a 2 x 1 x 1 rank grid, the Schur products fused on
    both ranks: v and p of the undecomposed run to 1e-9."""
    n, ranks = (24, 16, 12), (2, 1, 1)

    def gather(parts):
        v, p = np.full((3, n[2], n[1], n[0]), np.nan), np.full((n[2], n[1], n[0]), np.nan)
        for r in parts:
            lo, ln = r["lo"], r["ln"]
            sl = (slice(lo[2], lo[2] + ln[2]), slice(lo[1], lo[1] + ln[1]), slice(lo[0], lo[0] + ln[0]))
            v[(slice(None),) + sl] = r["v"].reshape(3, ln[2], ln[1], ln[0])
            p[sl] = r["p"].reshape(ln[2], ln[1], ln[0])
        assert not (np.isnan(v).any() or np.isnan(p).any())
        return v, p

    v2, p2 = gather(inproc.run_threads(2, _step_run, n, ranks))
    v1, p1 = gather(inproc.run_threads(1, lambda R: _step_run(None, n, ranks)))
    assert np.abs(v1).max() > 0.5
    assert np.linalg.norm(v2 - v1) <= 1e-9 * np.linalg.norm(v1)
    assert np.linalg.norm(p2 - p1) <= 1e-9 * np.linalg.norm(p1)
