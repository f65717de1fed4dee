"""-m gpu: the flow solver on INTERIOR ranks -- three and four ranks per axis, so that a block has a neighbour on both sides of an axis and the
two are different ranks -- against the single-domain CPU oracle.  The rank grids are those of tests/interior_ranks.py (what each is there to
reach stands there; tests/test_interior_ranks.py checks on the CPU that each really has such a rank); every case runs on one host thread and
one handle per rank over the in-process wire (tests/inproc.py), at most six handles, with a wire time limit of 30 s so that a pairing mistake is
reported per rank and not left to a hung test.

The workers and the tolerances are those of the two-rank tests, each named where it is used: tests/test_gpu_config5.py (_operator_worker,
_smoother_worker, _mirror_run), tests/test_gpu_ibm_owner.py (_owner_worker, _geometry), tests/test_gpu_ibm_migrate.py (the calls),
tests/test_gpu_ibm_force.py (_grid_worker), the sessions of tests/test_gpu_schur_var_multirank.py for the momentum block with the figures of
tests/test_gpu_multirank.py::_momentum_worker, tests/test_gpu_momentum.py and tests/test_gpu_momentum_cheb.py.  The three-rank cases of the
DIAG / ROWSUM Schur product run in tests/test_gpu_schur_var_multirank.py, the interior block in an 8-wave plan (ranks_std_z3) in
tests/test_gpu_rank_regimes.py.

No two-rank test asserts that apply, diagonal, rhs or project of the Poisson handle give the one-rank bits (the launch plan follows the block's
shape), so none is asserted here either; owner-rank spreading against the replicated path, a migrated set against a fresh one and fl_ibm_force
against one rank are bit for bit, as on two ranks."""
import numpy as np
import pytest

from oracle import fluca_oracle as fo
from tests import inproc
from tests import interior_ranks as ir

pytestmark = pytest.mark.gpu

WIRE = 30.0


def _threads(case, fn, *args):
    return inproc.run_threads(case.size, fn, case, *args, wire_timeout=WIRE)


def _knob(name, value):
    from fluca_amd import capi
    capi.check(capi.lib.fl_tuning_set(name.encode(), int(value)))


# ------------------------------------------------------------------------------------------------ A. operator and Krylov solvers

@pytest.mark.parametrize("name", ir.OPERATOR)
def test_operator_and_krylov_solvers_on_interior_ranks(name):
    """tests/test_gpu_config5.py::_operator_worker unchanged: apply (1e-12), diagonal (1e-13), rhs -- fl_fill_hifaces sends the first face plane to
    the low neighbour and receives from the high one, two different ranks under one tag -- and project (1e-12 max(1, scale)); CG, single-reduction
    CG and BiCGStab to rtol 1e-10 / 1e-10 / 1e-11: the oracle's reason, its iterations +-2 (BiCGStab +-max(3, its / 10)), the history head to
    1e-9, the solution to 1e-6."""
    from tests import test_gpu_config5 as C5
    case = ir.BY_NAME[name]
    ref = C5._reference(case)
    assert all(_threads(case, C5._operator_worker, ref))


def _plan_worker(R, case, planes, b):
    """the communicator's counts against fl_halo_plan; fl_poisson_gst_bc on all six boundaries; one CG solve to rtol 1e-10 with its history"""
    import torch
    from tests import mp_common as mpc
    from tests import test_gpu_config5 as C5
    P, d, s = C5._handle(R, case)
    out = {}
    with torch.cuda.stream(s):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        plan = ir.halo_plan(case, R.rank)
        info = P.comm_info()
        assert info["nranks"] == R.size and info["rank"] == R.rank
        assert info["messages"] == len(plan) and info["neighbours"] == len({m[0] for m in plan}), (info, plan)
        for ax in ir.interior_axes(case, R.rank):      # an interior rank: two messages of that axis, to two different ranks
            peers = [m[0] for m in plan if m[1] // 2 == ax]
            assert len(peers) == 2 and peers[0] != peers[1], (R.rank, ax, plan)
        out["interior"] = bool(ir.interior_axes(case, R.rank))
        blk = mpc.block(d)      # (z, y, x) slices
        for b6 in range(6):
            ax, side = b6 // 2, b6 % 2
            keep = [k for k, a in enumerate((2, 1, 0)) if a != ax]          # the plane's axes in (z, y, x) order
            pb = np.ascontiguousarray(planes[b6][tuple(blk[k] for k in keep)])
            Vd = torch.zeros(P.nface[ax], dtype=torch.float64, device="cuda")
            P.gst_bc(b6, dev(pb), Vd)
            s.synchronize()
            shape = [d.len[2], d.len[1], d.len[0]]
            shape[2 - ax] = P.nface[ax] // (P.ncell // d.len[ax])
            got = Vd.cpu().numpy().reshape(shape)
            touches = d.coord[ax] == (d.ranks[ax] - 1 if side else 0)
            want = np.zeros(shape)
            if case.bc[b6] == ir.O and touches:          # only the rank that touches the outlet writes, into the outlet's face layer
                sl = [slice(None)] * 3
                sl[2 - ax] = shape[2 - ax] - 1 if side else 0
                want[tuple(sl)] = case.g.gst_bc_coeff(ax, side) * pb
            assert np.allclose(got, want, rtol=1e-15, atol=0), ("gst_bc", R.rank, b6)          # tests/test_gpu_poisson.py's figure
        xg, ig = P.solve(dev(C5._blk(case, d, b)), history=True, remove_nullspace=int(case.nullspace), rtol=1e-10, maxit=4000, check_every=8)
        s.synchronize()
        out.update(x=xg.cpu().numpy(), iters=ig["iters"], reason=ig["reason"], hist=np.asarray(ig["history"]))
    P.close()
    return out


@pytest.mark.parametrize("name", ir.OPERATOR)
def test_outlet_vector_and_overlapped_exchange_on_interior_ranks(name):
    """The communicator holds fl_halo_plan's messages (two of the split axis on the middle rank); fl_poisson_gst_bc writes coeff * p_b on the one
    rank that touches an outlet and nothing on a rank in the middle of the axis (1e-15, tests/test_gpu_poisson.py).  Then a CG solve to rtol 1e-10
    with the exchange of r hidden behind k_cg_Bq (overlap = 1: the ghosts of two different peers are formed as r - alpha q from the q kept on both
    block ends, two transfers per axis on the second stream) and after it (0): the same iterations and reason, the history to 1e-9, x to 1e-10
    (tests/test_gpu_multirank.py::test_overlapped_exchange_changes_nothing holds two ranks to 1e-12; seen here: printed)."""
    from tests import test_gpu_config5 as C5
    case = ir.BY_NAME[name]
    rng = np.random.default_rng(7)
    n = case.n
    planes = [rng.standard_normal([m for k, m in enumerate((n[2], n[1], n[0])) if (2, 1, 0)[k] != b6 // 2]) for b6 in range(6)]
    # the right-hand side of the operator test, on which the oracle's CG gets to 1e-10 also where a stretched axis makes S symmetric in the
    # volume-weighted inner product only (on x3_channel KSPCG stalls short of 1e-10 on other right-hand sides, on the oracle as on the GPU)
    ref = C5._reference(case)
    b, io = ref["b"], ref["cg"][1]
    assert io["reason"] == 2
    runs = {}
    for ov in (1, 0):
        _knob("overlap", ov)
        try:
            runs[ov] = _threads(case, _plan_worker, planes, b)
        finally:
            _knob("overlap", 1)
    assert any(r["interior"] for r in runs[1])
    xmax = max(np.abs(r["x"]).max() for r in runs[1])
    for rank, (a, c) in enumerate(zip(runs[1], runs[0])):
        assert a["iters"] == c["iters"] and a["reason"] == c["reason"] == 2, (rank, a["iters"], c["iters"], a["reason"], c["reason"])
        assert abs(a["iters"] - io["iters"]) <= 2, (a["iters"], io["iters"])
        dh, dx = np.abs(a["hist"] / c["hist"] - 1).max(), np.abs(a["x"] - c["x"]).max() / xmax
        if rank == 0:
            print(f"{name}: overlap 1 against 0, {a['iters']} iterations, history {dh:.2e}, x {dx:.2e}")
        assert np.allclose(a["hist"], c["hist"], rtol=1e-9, atol=0), (rank, dh)
        assert dx <= 1e-10, (rank, dx)
        assert np.array_equal(a["hist"], runs[1][0]["hist"])          # every rank reports the same history


# ------------------------------------------------------------------------------------------------ B. fused smoother and multigrid

@pytest.mark.parametrize("name", ir.SMOOTHER)
def test_fused_smoother_and_multigrid_on_interior_ranks(name):
    """tests/test_gpu_config5.py::_smoother_worker unchanged: fl_fill_ghosts_deep with two messages per split axis (the edge cells of x3y2 in two hops
    through an interior block) -- Chebyshev sweeps of 2 and 7 steps with cheb_fuse 0 and 2 against the oracle to 1e-11, fused against unfused to
    1e-13, one launch per pair of steps -- and MG-PCG with two levels against MgOracle with the tri-linear prolongation (on z3_mg it reaches
    across both rank faces of the middle block; on the two others y and z are halved and x is not).  Every rank reports the same kernels."""
    from tests import test_gpu_config5 as C5
    case = ir.BY_NAME[name]
    ref = C5._smoother_reference(case, 2)
    res = _threads(case, C5._smoother_worker, ref, 2, (0, 2))
    assert all(r == res[0] for r in res), res


def test_fuse_decision_is_collective_on_three_uneven_blocks():
    """tests/test_gpu_config5.py::test_fuse_decision_is_collective_on_an_uneven_split on three ranks: with the default cheb_fuse = 1 the blocks of
    32768, 31744 and 32768 cells (tests/test_interior_ranks.py asserts the straddle) must take one decision, and it is "not fused": the middle
    rank objects, the two outer ranks would have fused."""
    from tests import test_gpu_config5 as C5
    case = ir.VOTE
    ref = C5._smoother_reference(case, 2)
    res = _threads(case, C5._smoother_worker, ref, 2, (1,))
    assert res[0] == res[1] == res[2], res
    assert res[0][2][1] == 2 and res[0][7][1] == 7, res


# ------------------------------------------------------------------------------------------------ C. the momentum block

class _MomentumProblem:
    """The state of tests/test_gpu_momentum_cheb.py::_state (CFL-sized convection beside a viscous part of the same size, so that D^-1 A is
    diagonally dominant and KSPCHEBYSHEV has its interval) on a case whose kappa is dt / rho, with every oracle answer the ranks are compared
    with -- all of it computed before the rank threads start."""

    def __init__(self, case, with_v0):
        hmin = min(float(np.diff(xf).min()) for xf in case.xf)
        self.dt, self.rho = 0.4 * hmin, 1.3
        self.mu = 0.8 * self.rho * hmin * hmin / self.dt
        self.case = case = case.with_kappa(self.dt / self.rho)
        self.with_v0 = with_v0
        g = case.g
        N = g.ncell
        rng = np.random.default_rng(23)
        self.V0 = [0.4 * rng.uniform(-1, 1, g.nface[d]) for d in range(3)]
        self.v0 = 0.4 * rng.uniform(-1, 1, 3 * N)
        self.W = g.apply_B(self.v0)
        self.A = A = g.assemble_momentum(1.0, self.dt, -0.5 * self.mu * self.dt / self.rho, self.V0, self.W)
        self.v = rng.standard_normal(3 * N)
        self.Av, self.diag, self.rowsum = A.mult(self.v), A.diag(), A.mult(np.ones(3 * N))
        self.G = A.gershgorin(fo.PC_JACOBI)
        radius = self.G - 1.0
        self.emin, self.emax = max(1.0 - radius, 0.9 / self.diag.mean()), 1.0 + radius
        self.b = rng.standard_normal(3 * N)
        self.bcgs = A.solve(self.b, ksp=fo.KSP_BCGS, pc=fo.PC_JACOBI, nullspace=False, rtol=1e-8, maxit=300)
        self.cheb = A.solve(self.b, ksp=fo.KSP_CHEBYSHEV, pc=fo.PC_JACOBI, norm=fo.NORM_PRECONDITIONED, nullspace=False, rtol=1e-8, maxit=400,
                            emin=self.emin, emax=self.emax)
        self.xconv, _ = A.solve(self.b, ksp=fo.KSP_BCGS, pc=fo.PC_JACOBI, nullspace=False, rtol=1e-13, maxit=1000)
        self.guess = self.xconv + 1e-3 * np.linalg.norm(self.xconv) / np.sqrt(self.xconv.size) * rng.standard_normal(self.xconv.size)
        # PCApply_ABF composed from the oracle's operators and Krylov restatements (tests/test_gpu_momentum.py::test_pcapply_abf_matches_composed_oracle)
        self.momrhs = rng.standard_normal(3 * N)
        self.interprhs = [1e-2 * rng.standard_normal(g.nface[d]) for d in range(3)]
        if case.nullspace:      # no flux through the walls: a singular S needs a right-hand side without a constant component
            for d in range(3):
                if not g.periodic[d]:
                    a = self.interprhs[d].reshape(case.fshape[d])
                    sl = [slice(None)] * 3
                    sl[2 - d] = [0, -1]
                    a[tuple(sl)] = 0.0
        vs, self.i0 = A.solve(self.momrhs, ksp=fo.KSP_BCGS, pc=fo.PC_JACOBI, nullspace=False, rtol=1e-10, maxit=500)
        Vs = g.apply_T(vs, self.interprhs)
        self.srhs = g.rhs(*Vs)
        # kspS: KSPCG as in the one-rank test -- except where the oracle's own CG does not get to 1e-10: on a stretched axis S is symmetric only in
        # the volume-weighted inner product, and on x3_channel CG stalls at 1e-9 of the initial residual.  There both sides run BiCGStab, as the
        # host mirror does on the channel (-ns_abf_schur_ksp_type bcgs), with BiCGStab's iteration band of tests/test_gpu_config5.py
        self.schur_ksp = fo.KSP_CG
        self.po, self.i1 = case.S.solve(self.srhs, ksp=fo.KSP_CG, pc=fo.PC_JACOBI, nullspace=case.nullspace, rtol=1e-10, maxit=5000)
        if self.i1["reason"] <= 0:
            self.schur_ksp = fo.KSP_BCGS
            self.po, self.i1 = case.S.solve(self.srhs, ksp=fo.KSP_BCGS, pc=fo.PC_JACOBI, nullspace=case.nullspace, rtol=1e-10, maxit=5000)
        assert self.i0["reason"] == 2 and self.i1["reason"] == 2
        self.v_ref = vs - np.concatenate(g.apply_G(self.po))
        self.V_ref = [a - c for a, c in zip(Vs, g.apply_gst(self.po))]

    # what tests/test_gpu_schur_var_multirank.py::_session / _blocks read
    n = property(lambda self: self.case.n)
    xf = property(lambda self: self.case.xf)
    bc = property(lambda self: self.case.bc)
    g = property(lambda self: self.case.g)
    shp = property(lambda self: self.case.shp)
    fshape = property(lambda self: self.case.fshape)
    periodic = property(lambda self: self.case.periodic)

    def decomp(self, rank):
        return self.case.decomp(rank)


def _momentum_worker(R, case, pb):
    import torch
    from fluca_amd import capi
    from fluca_amd.poisson import KspOptions
    from tests import test_gpu_schur_var_multirank as T
    P, M, d, s = T._session(R, pb, R.rank)
    cell, face = T._blocks(pb, d)
    N = pb.g.ncell
    loc3 = lambda v: np.concatenate([cell(v[c * N:(c + 1) * N]) for c in range(3)])
    dev = T._dev
    out = dict(lo=[int(d.lo[a]) for a in range(3)], ln=[int(d.len[a]) for a in range(3)])
    with torch.cuda.stream(s):
        host = lambda t: (s.synchronize(), t.cpu().numpy())[1]
        v0d = dev(loc3(pb.v0))
        # cnl->v0interp = B v0: the ghost layers of v0 come from two different ranks
        Wd = M.interp_faces(v0d)
        for q in range(9):
            assert np.abs(host(Wd[q]) - face(pb.W[q], q % 3)).max() <= 2e-13 * np.abs(pb.v0).max(), ("interp_faces", R.rank, q)
        V0d = [dev(face(pb.V0[a], a)) for a in range(3)]
        if pb.with_v0:
            # the ends-only form into arrays of junk: what it writes is B v0, what it leaves alone stays; the state with v0 reads nothing else
            junk = [torch.full((P.nface[q % 3],), 1e300, dtype=torch.float64, device="cuda") for q in range(9)]
            We = M.interp_faces(v0d, ends_only=True, out=junk)
            left = 0
            for q in range(9):
                got, want = host(We[q]), face(pb.W[q], q % 3)
                kept = got == 1e300
                left += int(kept.sum())
                assert np.abs(got - want)[~kept].max() <= 2e-13 * np.abs(pb.v0).max(), ("interp_faces_ends", R.rank, q)
            out["ends_left_alone"] = left
            M.set_state(pb.dt, pb.rho, pb.mu, V0d, We, v0=v0d)
        else:
            M.set_state(pb.dt, pb.rho, pb.mu, V0d, Wd)

        def close(got, want, what):
            err = np.abs(host(got) - loc3(want)).max()
            assert err <= 2e-13 * np.abs(want).max(), (what, R.rank, err)

        close(M.apply(dev(loc3(pb.v))), pb.Av, "apply")
        close(M.diagonal(), pb.diag, "diagonal")
        close(M.rowsum(), pb.rowsum, "rowsum")
        radius = M.gershgorin()
        assert abs((1.0 + radius) - pb.G) <= 1e-12 * pb.G, (radius, pb.G)
        emin, emax = M.chebyshev_interval()
        assert emax == 1.0 + radius and abs(emin - max(1.0 - radius, 0.9 / pb.diag.mean())) <= 1e-12, (emin, emax, pb.emin, pb.emax)
        bd = dev(loc3(pb.b))
        x, out["bcgs"] = M.solve(bd, history=True, rtol=1e-8, maxit=300)
        out["x_bcgs"] = host(x)
        x, out["cheb"] = M.solve(bd, type=fo.KSP_CHEBYSHEV, pc=fo.PC_JACOBI, norm_type=fo.NORM_PRECONDITIONED, rtol=1e-8, maxit=400, history=True, check_every=5,
                                 emin=pb.emin, emax=pb.emax)
        out["x_cheb"] = host(x)
        for ksp in (fo.KSP_BCGS, fo.KSP_CHEBYSHEV):          # tests/test_gpu_momentum_cheb.py::test_solve_from_a_nonzero_initial_guess, (b)
            kw = dict(type=ksp, pc=fo.PC_JACOBI, rtol=1e-7, maxit=400, check_every=3)
            _, ip = M.solve(bd, **kw)
            x, ig = M.solve(bd, x=dev(loc3(pb.guess)), initial_guess_nonzero=1, **kw)
            out["guess", ksp] = (ip, ig, host(x))
        v, Vf, p, info = M.abf_apply(dev(loc3(pb.momrhs)), [dev(face(pb.interprhs[a], a)) for a in range(3)], None,
                                     momentum=KspOptions(type=capi.KSP_BCGS, rtol=1e-10, maxit=500),
                                     schur=KspOptions(type=pb.schur_ksp, rtol=1e-10, maxit=5000, remove_nullspace=int(pb.case.nullspace)))
        out.update(v=host(v), V=[host(a) for a in Vf], p=host(p), abf=info)
    M.close()
    P.close()
    return out


def _cells(case, parts, key, ncomp):
    a = np.full((ncomp,) + case.shp, np.nan)
    for r in parts:
        lo, ln = r["lo"], r["ln"]
        a[:, lo[2]:lo[2] + ln[2], lo[1]:lo[1] + ln[1], lo[0]:lo[0] + ln[0]] = r[key].reshape(ncomp, ln[2], ln[1], ln[0])
    assert not np.isnan(a).any(), "the blocks do not tile the grid"
    return a.ravel()


@pytest.mark.parametrize("with_v0", [False, True], ids=["stored", "v0"])
@pytest.mark.parametrize("name", ir.MOMENTUM)
def test_momentum_block_on_interior_ranks(name, with_v0):
    """The momentum block where both ends of a block are rank faces (k_mom3 / k_mom2 read the stored fields there: with v0 the state holds nothing
    else, formed by the ends-only interpolation into arrays of junk): interp_faces, apply, diagonal and rowsum against the assembled A to 2e-13
    (tests/test_gpu_multirank.py::_momentum_worker, tests/test_gpu_momentum.py), the Gershgorin radius and the default Chebyshev interval to 1e-12;
    BiCGStab to rtol 1e-8 (the oracle's reason, iterations within max(2, its / 6), six history entries to 1e-6, x to 1e-5) and Chebyshev (the oracle's
    iterations, history to 1e-8, x to 1e-9: tests/test_gpu_momentum_cheb.py), both again from a guess close to the answer (fewer iterations, x to
    50 rtol); fl_abf_apply with the ID types against the composed oracle (p 1e-6, v and V 1e-7, the iteration counts: tests/test_gpu_momentum.py)."""
    from tests.step_rhs import gather
    pb = _MomentumProblem(ir.BY_NAME[name], with_v0)
    case = pb.case
    res = _threads(case, _momentum_worker, pb)
    if with_v0 and min(b[1] for b in case.blocks()) > 8:
        assert all(r["ends_left_alone"] > 0 for r in res)          # the inner entries are left alone (ny > 8)
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    r0 = res[0]
    # BiCGStab from zero
    xo, io = pb.bcgs
    ig = r0["bcgs"]
    assert all(r["bcgs"]["iters"] == ig["iters"] and r["bcgs"]["reason"] == ig["reason"] for r in res)
    assert ig["reason"] == io["reason"] and abs(ig["iters"] - io["iters"]) <= max(2, io["iters"] // 6), (ig["iters"], ig["reason"], io["iters"], io["reason"])
    m = min(len(ig["history"]), len(io["history"]), 6)
    assert np.allclose(ig["history"][:m], io["history"][:m], rtol=1e-6)
    e_b = rel(_cells(case, res, "x_bcgs", 3), xo)
    # Chebyshev from zero
    xo, io = pb.cheb
    ig = r0["cheb"]
    assert io["reason"] > 0 and ig["reason"] == io["reason"] and ig["iters"] == io["iters"], (ig["iters"], ig["reason"], io["iters"], io["reason"])
    assert np.allclose(ig["history"][:io["iters"] + 1], io["history"][:io["iters"] + 1], rtol=1e-8, atol=1e-13 * io["history"][0])
    e_c = rel(_cells(case, res, "x_cheb", 3), xo)
    print(f"{name} v0={with_v0}: BiCGStab {r0['bcgs']['iters']} iterations, x {e_b:.2e}; Chebyshev {ig['iters']} iterations, x {e_c:.2e}")
    assert e_b <= 1e-5 and e_c <= 1e-9, (e_b, e_c)
    # from a guess
    for ksp in (fo.KSP_BCGS, fo.KSP_CHEBYSHEV):
        ip, ig, _ = r0["guess", ksp]
        assert ip["reason"] == 2 and ig["reason"] == 2 and 0 < ig["iters"] < ip["iters"], (ksp, ig["iters"], ip["iters"])
        for r in res:
            r["xg"] = r["guess", ksp][2]
        e = rel(_cells(case, res, "xg", 3), pb.xconv)
        assert e <= 50 * 1e-7, (ksp, e)
    # PCApply_ABF
    info = r0["abf"]
    assert info[0]["reason"] == pb.i0["reason"] and info[1]["reason"] == pb.i1["reason"]
    band = max(3, pb.i1["iters"] // (20 if pb.schur_ksp == fo.KSP_CG else 10))
    assert abs(info[0]["iters"] - pb.i0["iters"]) <= 2 and abs(info[1]["iters"] - pb.i1["iters"]) <= band, (info, pb.i0["iters"], pb.i1["iters"])
    v, Vf, p = gather(res, case.g)
    po = pb.po
    if case.nullspace:
        p, po = p - p.mean(), po - po.mean()
    figs = dict(p=rel(p, po), v=rel(v, pb.v_ref), V=[float(np.linalg.norm(Vf[d] - pb.V_ref[d]) / max(np.linalg.norm(pb.V_ref[d]), 1e-30)) for d in range(3)])
    print(f"{name} v0={with_v0}: fl_abf_apply against the composed oracle {figs}, iterations {info[0]['iters']} / {info[1]['iters']}")
    assert figs["p"] <= 1e-6 and figs["v"] <= 1e-7 and max(figs["V"]) <= 1e-7, figs
    assert np.linalg.norm(case.g.rhs(*Vf)) <= 1e-7 * np.linalg.norm(pb.srhs)


# ------------------------------------------------------------------------------------------------ E. IBM on interior ranks

def _ibm_run(name, kind):
    from tests import test_gpu_ibm_owner as OW
    case = ir.BY_NAME[name]
    h, X = ir.spacing(case), ir.markers(name)
    ref = OW._reference(case, h, X, kind)
    res = _threads(case, OW._owner_worker, ref, kind, True)
    assert all(r["create_rc"] == 0 for r in res), [r["create_rc"] for r in res]
    return case, ref, res


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", ir.IBM)
def test_replicated_and_owner_rank_markers_on_interior_ranks(name, kind):
    """tests/test_gpu_ibm_owner.py::_owner_worker unchanged, on a body whose supports straddle both faces of the middle block: the middle rank sends
    ghost copies to -1 and +1 of the split axis and adds the partial sums returned by two different peers.  Owner-rank and replicated interp and
    spread against the oracle (rtol 1e-12), conservation; owner-rank spreading equals the replicated path bit for bit; selections, copy counts and
    the bytes on the wire are those of numpy geometry; no all-reduce on the owner-rank path."""
    from tests import test_gpu_ibm_owner as OW
    case, ref, res = _ibm_run(name, kind)
    OW._against_oracle(case, ref, res)
    assert all(r["update_same"] for r in res)
    L = ref["X"][0].size
    owner, copies = OW._geometry(case, kind, ref["X"])
    for rank, r in enumerate(res):
        assert np.allclose(r["U_rep"], ref["U"], rtol=1e-12, atol=1e-13), ("replicated interp", rank)
        assert np.array_equal(r["f"], r["f_rep"]), (rank, np.abs(r["f"] - r["f_rep"]).max())
        assert np.allclose(r["U"], r["U_rep"][:, r["sel"]], rtol=1e-12, atol=1e-13), rank
        assert np.array_equal(r["sel"], np.nonzero(owner == rank)[0]), rank
        ghosts = sum(1 for _, to, _ in copies if to == rank)
        sent = sum(1 for l, _, _ in copies if owner[l] == rank)
        assert r["counts"] == [int((owner == rank).sum()), ghosts, sent, 8 * ghosts, 32 * sent], (rank, r["counts"], ghosts, sent)
        assert r["interp_wire"]["allreduces"] == 0 and r["spread_wire"]["allreduces"] == 0 and r["rep_interp_wire"]["allreduces"] == 1
        assert r["interp_wire"]["bytes"] == 3 * r["counts"][3] and r["spread_wire"]["bytes"] == r["counts"][4]
        assert r["interp_wire"]["exchanges"] <= 1 and r["spread_wire"]["exchanges"] <= 1
    assert any(not np.array_equal(r["f"], r["f0"]) for r in res)
    ncopies = sum(r["counts"][2] for r in res)
    assert ncopies == len(copies) == sum(r["counts"][1] for r in res) > 0
    assert sum(r["interp_wire"]["bytes"] for r in res) == 24 * ncopies and sum(r["spread_wire"]["bytes"] for r in res) == 32 * ncopies
    # the middle rank holds copies of both neighbours' markers and has copies on both
    pairs = {(int(owner[l]), to) for l, to, _ in copies}
    assert {(0, 1), (2, 1), (1, 0), (1, 2)} <= pairs, pairs


def _migrate_worker(R, case, path, ref, kind):
    """an owned set at path[0] migrates to path[1], then to path[2]; after each call its numbers, counts, interp and spread, and those of a set
    created afresh on the same handle at the same positions"""
    import torch
    from fluca_amd import capi
    from tests import test_gpu_ibm_migrate as MG
    from tests.test_gpu_config5 import _blk
    lib = capi.lib
    P, d, s = MG._open(R, case)
    out = dict(calls=[])
    with torch.cuda.stream(s):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        m, rc, gid = MG._select_create(torch, capi, P, kind, [dev(a) for a in path[0]])
        assert rc == 0, rc
        attr = torch.stack([8.0 * gid.double() + a for a in range(3)]).reshape(-1).contiguous()
        for k in (1, 2):
            Xd = [dev(a) for a in path[k]]
            rc, Lnew, moved = MG._migrate(lib, m, [t[gid].contiguous() for t in Xd], 3, attr)
            assert rc == 0, (k, rc)
            Xf, gid, attr = MG._fetch(torch, lib, m, Lnew, 3)
            U, f, f0b = MG._apply(torch, capi, case, d, m, ref, gid, dev)
            mf, rc, sel = MG._select_create(torch, capi, P, kind, Xd)
            assert rc == 0, rc
            Uf, ff, _ = MG._apply(torch, capi, case, d, mf, ref, sel, dev)
            out["calls"].append(dict(gid=gid.cpu().numpy(), X=[t.cpu().numpy() for t in Xf], attr=attr.cpu().numpy().reshape(3, Lnew), moved=moved,
                                     counts=MG._counts(capi, m), U=U, f=f, f0=f0b, sel=sel.cpu().numpy(), fresh_counts=MG._counts(capi, mf), U_fresh=Uf, f_fresh=ff))
            lib.fl_ibm_destroy(mf)
        lib.fl_ibm_destroy(m)
        out["vol"] = _blk(case, d, ref["vol"])
    P.close()
    return out


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", ir.IBM)
def test_markers_migrate_out_of_and_through_the_middle_block(name, kind):
    """fl_ibm_migrate with leavers in both directions and arrivals from both sides in one call (the middle rank's markers within a cell of its two
    faces leave to the low and to the high neighbour while markers of both arrive), then a call that carries one marker on from rank 1 to rank 2,
    having come from rank 0 (tests/test_interior_ranks.py asserts both of the path).  After each call: every rank's numbers are the ascending list
    of the markers it owns by geometry, positions and attributes travelled bit for bit, moved[] and the copy counts are the geometric ones, and the
    set equals a fresh fl_ibm_owned_select + fl_ibm_create_owned at the new positions bit for bit (numbers, counts, interp, spread); after the
    last call interp and spread agree with the oracle (tests/test_gpu_ibm_owner.py's tolerances)."""
    from tests import test_gpu_ibm_owner as OW
    case = ir.BY_NAME[name]
    path, runner = ir.migration_path(name)
    ref = OW._reference(case, ir.spacing(case), path[2], kind)
    res = _threads(case, _migrate_worker, path, ref, kind)
    own = [OW._geometry(case, kind, X)[0] for X in path]
    for k in (1, 2):
        now, copies = OW._geometry(case, kind, path[k])
        prev = own[k - 1]
        for rank, r in enumerate(res):
            c = r["calls"][k - 1]
            mine = np.nonzero(now == rank)[0]
            assert np.array_equal(c["gid"], mine), (k, rank)
            for a in range(3):
                assert np.array_equal(c["X"][a], path[k][a][mine]) and np.array_equal(c["attr"][a], 8.0 * mine + a), (k, rank, a)
            assert c["moved"] == [int(((prev == rank) & (now != rank)).sum()), int(((prev != rank) & (now == rank)).sum())], (k, rank, c["moved"])
            ghosts = sum(1 for _, to, _ in copies if to == rank)
            sent = sum(1 for l, _, _ in copies if now[l] == rank)
            assert c["counts"] == [mine.size, ghosts, sent, 8 * ghosts, 32 * sent], (k, rank, c["counts"], ghosts, sent)
            assert np.array_equal(c["sel"], c["gid"]) and c["fresh_counts"] == c["counts"], (k, rank)
            assert np.array_equal(c["U"], c["U_fresh"]), (k, rank, np.abs(c["U"] - c["U_fresh"]).max())
            assert np.array_equal(c["f"], c["f_fresh"]), (k, rank, np.abs(c["f"] - c["f_fresh"]).max())
    first = res[1]["calls"][0]["moved"]
    assert first[0] >= 24 and first[1] >= 20, first          # the middle rank: both groups of leavers, both groups of arrivals (and the runner)
    assert runner in res[1]["calls"][0]["gid"] and runner in res[2]["calls"][1]["gid"]          # 0 -> 1 in call 1, 1 -> 2 in call 2
    last = [dict(sel=r["calls"][1]["gid"], U=r["calls"][1]["U"], f=r["calls"][1]["f"], f0=r["calls"][1]["f0"], vol=r["vol"]) for r in res]
    OW._against_oracle(case, ref, last)


@pytest.mark.parametrize("name", ir.IBM)
def test_force_and_torque_on_interior_ranks_give_the_bits_of_one_and_of_two_ranks(name):
    """fl_ibm_force (tests/test_gpu_ibm_force.py::_grid_worker unchanged) of the body, two bodies with interleaved ids and one body, as a replicated
    and as an owned set: the same bits on every rank of the three / four rank grid, of the two-rank split of the same grid and on one rank, which
    are the bits of the numpy split sum (tests/ibm_force_reference.py)."""
    from tests import ibm_force_reference as fr
    from tests import test_gpu_ibm_force as FO
    case = ir.BY_NAME[name]
    h, X = ir.spacing(case), ir.markers(name)
    L = X[0].size
    rng = np.random.default_rng(11)
    sets = {"body": (X, rng.standard_normal((3, L)), rng.uniform(0.5, 1.5, L) * h ** 3, np.arange(L) % 2)}
    one, two = case.on_ranks((1, 1, 1)), case.on_ranks(tuple(min(r, 2) for r in case.ranks))
    res1 = inproc.run_threads(1, FO._grid_worker, one, sets, None, None)[0]
    res2 = inproc.run_threads(two.size, FO._grid_worker, two, sets, None, None, wire_timeout=WIRE)
    resn = _threads(case, FO._grid_worker, sets, None, None)
    period = tuple(case.box[a][1] - case.box[a][0] if case.periodic[a] else None for a in range(3))
    _, F, dV, ids = sets["body"]
    for nb, tag, body in ((2, "", ids), (1, ", one body", None)):
        want = res1["body", "replicated" + tag]
        assert want[0] == 0
        FO._check(fr.reference(np.stack(X), F, dV, FO.ABOUT_C5[:nb], period, body=body, nbody=nb), want[1], want[2], f"{name}{tag}, one rank")
        assert FO._same(res1["body", "owned" + tag], want)
        for what, res in (("two ranks", res2), ("interior ranks", resn)):
            for rank, r in enumerate(res):
                assert FO._same(r["body", "replicated" + tag], want), (what, rank, "replicated")
                assert FO._same(r["body", "owned" + tag], want), (what, rank, "owned")
    counts = [r["body", "count"] for r in resn]
    assert sum(counts) == L and min(counts[:3]) > 0, counts


# ------------------------------------------------------------------------------------------------ G. a time step

STEP_BOX = (3.0, 1.2, 0.8)      # x3_channel's box with uniform spacing 0.1 on all three axes (the direct-forcing IBM of the mirror wants it)


@pytest.mark.parametrize("distribution", ["replicated", "owner"])
def test_nsstep_with_the_body_on_three_ranks_in_a_row(distribution):
    """Two CNLinear steps of the channel through the C host mirror (tests/test_gpu_config5.py::_mirror_run) on x3_channel's grid and rank grid,
    uniform, with the elliptic cylinder of part E held at rest by direct forcing: the inlet on rank 0, the outlet on rank 2, a middle rank whose
    boundary-condition vectors are those of the walls in y alone.  Against StepOracle with the same forcing: v, V, p to 1e-6 -- the figure of
    test_nsstep_on_the_2x2x2_rank_grid_matches_the_oracle_step, whose solver tolerances these are on both sides (outer 1e-10, inner 1e-12), and
    what two solves that each stop at those can agree to.  Against the same run on one rank: v and V to 1e-8, p to 1e-7, the tolerance of
    test_nsstep_with_the_immersed_cylinder_on_the_2x2x2_rank_grid between rank grids."""
    from tests import test_gpu_config5 as C5
    from tests.test_gpu_ibm_owner import _extra_options
    case = ir.BY_NAME["x3_channel"]
    n, ranks, nsteps, dt, rho, mu = case.n, case.ranks, 2, 5e-3, 1.0, 0.05
    Lx, Ly, Lz = STEP_BOX
    X = ir.markers("x3_channel")
    h = Lx / n[0]
    opts = ("-ns_ibm_marker_distribution", "owner") if distribution == "owner" else ()
    with _extra_options(*opts):
        parts = inproc.run_threads(3, C5._mirror_run, n, ranks, nsteps, True, STEP_BOX, X, wire_timeout=WIRE)
    v, V, p = C5._gather(parts, n, STEP_BOX)
    one = inproc.run_threads(1, lambda R: C5._mirror_run(None, n, ranks, nsteps, True, STEP_BOX, X))
    v1, V1, p1 = C5._gather(one, n, STEP_BOX)
    free = inproc.run_threads(1, lambda R: C5._mirror_run(None, n, ranks, nsteps, False, STEP_BOX))
    vf, _, _ = C5._gather(free, n, STEP_BOX)
    assert np.linalg.norm(v1 - vf) >= 1e-3 * np.linalg.norm(vf)           # the forcing does something
    g = fo.Grid.uniform(n, [(0, Lx), (0, Ly), (0, Lz)], C5.C5_BC, dt / rho)

    def velocity(b, t, Xf):
        if b == 0:
            return np.stack([4.0 * Xf[:, 1] * (Ly - Xf[:, 1]) / Ly ** 2 * (1.0 + 0.3 * np.sin(2 * np.pi * Xf[:, 2] / Lz)), np.zeros(len(Xf)), np.zeros(len(Xf))])
        return np.zeros((3, len(Xf)))

    pressure = lambda b, t, Xf: 0.3 * np.sin(3.0 * t) + 0.1 * Xf[:, 1]
    so = fo.StepOracle(g, dt, rho, mu, velocity, krylov_rtol=1e-12, outer_rtol=1e-10, pressure=pressure, ibm=dict(kind=0, X=X, dV=np.full(X[0].size, h ** 3)))
    so.S_ksp = fo.KSP_BCGS
    vo, Vo, po = np.zeros(3 * g.ncell), [np.zeros(nf) for nf in g.nface], np.zeros(g.ncell)
    for _ in range(nsteps):
        vo, Vo, po, _info = so.step_once(vo, Vo, po)
    rel = lambda a, b: float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(b), 1e-12))
    oracle = dict(v=rel(v, vo), V=[rel(V[d], Vo[d]) for d in range(3)], p=rel(p, po))
    ranks1 = dict(v=rel(v, v1), V=[rel(V[d], V1[d]) for d in range(3)], p=rel(p, p1))
    print(f"{distribution}: three ranks against StepOracle {oracle}; against one rank {ranks1}")
    assert np.abs(vo).max() > 0.5
    assert oracle["v"] <= 1e-6 and max(oracle["V"]) <= 1e-6 and oracle["p"] <= 1e-6, oracle
    assert ranks1["v"] <= 1e-8 and max(ranks1["V"]) <= 1e-8 and ranks1["p"] <= 1e-7, ranks1
    # continuity of the projected face velocity, as test_nsstep_on_the_2x2x2_rank_grid_matches_the_oracle_step holds it (against the inlet flux scale)
    assert np.abs(g.rhs(*[a.ravel() for a in V])).max() <= 1e-6 * np.abs(Vo[0]).max() / (Lx / n[0])
    assert all(r["inner"] == parts[0]["inner"] for r in parts)        # every rank counted the same inner iterations
