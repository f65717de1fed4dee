"""-m gpu: the several-rank kernels on rank grids whose BLOCKS take the launch plans the product runs at 256^3 - 512^3, against the single-domain
CPU oracle on the global grid.

The rank grids are RANK_REGIMES of tests/launch_regimes.py (tests/test_launch_regimes.py checks on the CPU that every block still reaches its plan):
8-wave tiles whose last tile is partial in x and y, a short last z chunk, blocks with an odd nx or ny.  What a rank runs differently from a single
domain meets those edges only here: k_cg_A stores q on the block's six boundary layers only (PlanA::qb) and the neighbour's ghost of r is formed
from them as r - alpha q while k_cg_Bq runs (knob "overlap"); the single-reduction CG packs its faces behind MODE 10; fl_fill_ghosts_deep feeds
k_cheb2 two ghost layers, edge cells in two hops; fl_poisson_project runs k_project_six<false> on a padded copy of p; fl_poisson_rhs ships the
first face plane to the low neighbour; k_schur_var_ring runs at its full 128 blocks per XCD.  The toy grids of tests/test_gpu_multirank.py,
tests/test_gpu_config5.py and tests/test_gpu_schur_var_multirank.py all land in the 4-wave plans.

In-process rank grids (tests/inproc.py): one handle and one host thread per rank, the in-memory wire; at most four handles.  All oracle work of
a piece is done before the ranks start: a rank that waits for the host while its peers sit in an exchange runs into the wire's timeout.

Every tolerance is that of the single-rank or toy-grid test named beside it.  Measured on an MI355X, the largest figure over all problems (each
run prints its own before it asserts): operator pieces 5.2e-16; CG x 2.0e-14 and history 8.9e-14 of the oracle's; single-reduction CG x 2.3e-14,
history 7.5e-14; BiCGStab history 1.2e-14; Chebyshev x 2.2e-15, fused against cheb_fuse = 0 2.3e-16; the converged solves take the oracle's
iteration counts (218, 2187, 260, 267); the Schur product 9.5e-15 of the oracle's, 4.2e-16 of the composition's."""
import numpy as np
import pytest

from oracle import fluca_oracle as fo
from tests import inproc
from tests.gpu_common import CAVITY_BOX, mean_free_rhs, stretched_faces
from tests.launch_regimes import CAVITY, CHANNEL, RANK_BY_NAME, XPER, launch_plans, six_trips
from tests.test_gpu_config5 import _blk, _fblk, _handle

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 8, 11)       # odd and even: the x-updates are batched


class Problem:
    """a rank regime with one set of boundary types, uniform (the cavity box) or stretched in all three axes; the oracle grid is built here, the
    matrix on first use.  Carries what the handle / block helpers of tests/test_gpu_config5.py read from a case."""

    def __init__(self, reg, bc, stretched=False, kappa=1e-3):
        self.reg, self.n, self.ranks, self.own, self.bc, self.kappa = reg, reg.n, reg.ranks, reg.own, bc, kappa
        n = self.n
        self.size = self.ranks[0] * self.ranks[1] * self.ranks[2]
        assert 1 < self.size <= 4
        self.xf = stretched_faces(n) if stretched else [np.linspace(CAVITY_BOX[d][0], CAVITY_BOX[d][1], n[d] + 1) for d in range(3)]
        self.g = g = fo.Grid(n, self.xf, bc, kappa)
        self._S = None
        self.nullspace = fo.BC_PRESSURE_OUTLET not in bc
        self.periodic = reg.periodic(bc)
        self.shp = (n[2], n[1], n[0])
        self.fshape = [(n[2], n[1], g.nf[0]), (n[2], g.nf[1], n[0]), (g.nf[2], n[1], n[0])]

    @property
    def S(self):
        if self._S is None:
            self._S = self.g.assemble_S()
        return self._S

    def rhs(self):
        """the right-hand side of the single-rank regime tests: b = S p* with a mean-free p* where S has a null space, else random"""
        if self.nullspace:
            return mean_free_rhs(self.S, self.g.ncell)[1]
        return np.random.default_rng(5).standard_normal(self.g.ncell)


PROBLEMS = {
    "std_z-cavity": ("ranks_std_z", CAVITY, False),
    "std_z-channel": ("ranks_std_z", CHANNEL, False),
    "ranks_std_z3-cavity": ("ranks_std_z3", CAVITY, False),
    "ranks_std_z3-channel": ("ranks_std_z3", CHANNEL, False),
    "std_xy-xper": ("ranks_std_xy", XPER, False),
    "std_xy-cavity": ("ranks_std_xy", CAVITY, False),
    # on a uniform grid a rank that reads the coefficient rows of the wrong column / row / plane (an offset by its lo) reads the same numbers
    "std_xy-xper-stretched": ("ranks_std_xy", XPER, True),
    "mid_y-channel": ("ranks_mid_y", CHANNEL, False),
    "mid_x-xper": ("ranks_mid_x", XPER, False),
}
PIECES = {
    "std_z-cavity": ["operator", "cg", "cg_none", "cg_converged", "cg_sr"],
    "std_z-channel": ["operator", "cg", "cg_converged", "cg_sr", "cheb"],
    # three ranks along z: the middle block keeps q on plane 0 and plane 20 for two different peers; CHANNEL: the seam joins rank 2 to rank 0
    "ranks_std_z3-cavity": ["operator", "cg", "cg_sr"],
    "ranks_std_z3-channel": ["operator", "cg", "cg_sr", "cheb"],
    "std_xy-xper": ["operator", "cg", "cg_converged", "cg_sr", "cheb"],
    "std_xy-cavity": ["operator", "cg", "cg_converged", "cg_sr"],
    "std_xy-xper-stretched": ["operator", "cg_head", "cheb7"],
    "mid_y-channel": ["operator", "cg", "cg_sr", "bcgs", "cheb"],
    "mid_x-xper": ["operator", "cg", "cg_sr"],
}
RUNS = [(name, piece) for name, pieces in PIECES.items() for piece in pieces]

# one oracle grid and matrix at a time (up to 34 M cells: 8 s to assemble, 3 GB): the runs of a problem follow each other, the next problem
# replaces it
_LIVE = {}


def _problem(name):
    if name not in _LIVE:
        _LIVE.clear()
        reg, bc, stretched = PROBLEMS[name]
        _LIVE[name] = Problem(RANK_BY_NAME[reg], bc, stretched)
    return _LIVE[name]


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")


def _knob(name, value):
    from fluca_amd import capi
    capi.check(capi.lib.fl_tuning_set(name.encode(), int(value)))


def _open(R, pb):
    """this rank's handle; every rank checks the communicator's size and that its block is the table's, in the table's plan"""
    P, d, s = _handle(R, pb)
    info = P.comm_info()
    assert info["transport"] == 2 and info["nranks"] == R.size == pb.size and info["rank"] == R.rank, info
    blk = tuple(int(d.len[a]) for a in range(3))
    assert blk == pb.reg.blocks[R.rank], (R.rank, blk, pb.reg.blocks[R.rank])
    assert P.ncell == blk[0] * blk[1] * blk[2]
    assert launch_plans(blk)["cg.nw"] == 8 and six_trips(launch_plans(blk)) > 1
    return P, d, s


# ------------------------------------------------------------------------------------------------ operator pieces

def _operator_worker(R, pb, ref):
    """per piece, the largest absolute error on this rank's block; the two-subset projection against the all-six one, bit for bit"""
    import torch
    P, d, s = _open(R, pb)
    fig = {}
    with torch.cuda.stream(s):
        err = lambda t, want: float(np.abs(t.cpu().numpy() - want).max())
        pd = _dev(_blk(pb, d, ref["p"]))
        fig["apply"] = err(P.apply(pd), _blk(pb, d, ref["b"]))
        fig["diag"] = err(P.diagonal(), _blk(pb, d, ref["diag"]))
        Vl = [_dev(_fblk(pb, d, ref["V"][a], a)) for a in range(3)]
        assert tuple(P.nface) == tuple(int(v.numel()) for v in Vl)
        fig["rhs"] = err(P.rhs(*Vl), _blk(pb, d, ref["rhs"]))
        vl = [_dev(_blk(pb, d, ref["v"][c])) for c in range(3)]
        P.project(pd, v=vl, V=Vl)
        s.synchronize()
        for a in range(3):
            fig["project V", a] = err(Vl[a], _fblk(pb, d, ref["V-Gst"][a], a))
            fig["project v", a] = err(vl[a], _blk(pb, d, ref["v-G"][a]))
        # two subsets that together make the six (k_project_all on the padded p)
        V2 = [_dev(_fblk(pb, d, ref["V"][a], a)) for a in range(3)]
        v2 = [_dev(_blk(pb, d, ref["v"][c])) for c in range(3)]
        P.project(pd, v=(v2[0], None, None), V=(None, V2[1], None))
        P.project(pd, v=(None, v2[1], v2[2]), V=(V2[0], None, V2[2]))
        s.synchronize()
        fig["subsets bit for bit"] = all(torch.equal(V2[a], Vl[a]) and torch.equal(v2[a], vl[a]) for a in range(3))
    P.close()
    return fig


def run_operator(pb):
    """apply, diagonal, rhs (the first face plane goes to the low neighbour) and the projection of all six arrays (k_project_six<false> on the padded
    copy of p, several grid-stride trips) on every rank against S.mult, S.diag, g.rhs, g.apply_gst / g.apply_G; tolerances of
    tests/test_gpu_config5.py::_operator_worker (1e-12 relative, the diagonal 1e-13)."""
    g, S = pb.g, pb.S
    rng = np.random.default_rng(20260313)
    p = rng.uniform(-1, 1, g.ncell)
    if pb.nullspace:
        p -= p.mean()
    ref = dict(p=p, b=S.mult(p), diag=S.diag())
    ref["V"] = [rng.standard_normal(nf) for nf in g.nface]
    ref["v"] = [rng.standard_normal(g.ncell) for _ in range(3)]
    ref["rhs"] = g.rhs(*ref["V"])
    ref["V-Gst"] = [V - G for V, G in zip(ref["V"], g.apply_gst(p))]
    ref["v-G"] = [v - G for v, G in zip(ref["v"], g.apply_G(p))]
    figs = inproc.run_threads(pb.size, _operator_worker, pb, ref)
    worst = {k: max(f[k] for f in figs) for k in figs[0] if k != "subsets bit for bit"}
    scale = {"apply": np.abs(ref["b"]).max(), "diag": np.abs(ref["diag"]).max(), "rhs": max(1.0, np.abs(ref["rhs"]).max())}
    for a in range(3):
        scale["project V", a] = max(1.0, np.abs(ref["V-Gst"][a]).max())
        scale["project v", a] = max(1.0, np.abs(ref["v-G"][a]).max())
    rel = {k: worst[k] / scale[k] for k in worst}
    print("operator", pb.reg.name, rel)
    for k, v in rel.items():
        assert v <= (1e-13 if k == "diag" else 1e-12), (k, v)
    assert all(f["subsets bit for bit"] for f in figs)


# ------------------------------------------------------------------------------------------------ the Krylov solves

def _solve_worker(R, pb, b, specs, prev):
    """the solves of specs = [(key, options, oracle x or None)] one after the other on this rank's handle; per key the statistics, the block of x,
    its largest error against the oracle's block and against the same rank's x of an earlier run (prev)"""
    import torch
    P, d, s = _open(R, pb)
    out = {}
    with torch.cuda.stream(s):
        bd = _dev(_blk(pb, d, b))
        for key, kw, xo in specs:
            before = R.stats()["allreduces"]
            xg, ig = P.solve(bd, **kw)
            s.synchronize()
            ig["allreduces"] = R.stats()["allreduces"] - before
            ig["x"] = xg.cpu().numpy()
            if xo is not None:
                ig["err"] = float(np.abs(ig["x"] - _blk(pb, d, xo)).max())
            if prev is not None:
                ig["dprev"] = float(np.abs(ig["x"] - prev[R.rank][key]["x"]).max())
            out[key] = ig
    P.close()
    return out


def _agree(res, key):
    """every rank reports the same iterations, reason and history; -> rank 0's"""
    r0 = res[0][key]
    for r in res[1:]:
        assert r[key]["iters"] == r0["iters"] and r[key]["reason"] == r0["reason"], (key, r[key]["iters"], r0["iters"])
        if "history" in r0:
            assert np.array_equal(r[key]["history"], r0["history"]), key
    return r0


def _gather_x(pb, res, key):
    from tests import mp_common as mpc
    x = np.full(pb.shp, np.nan)
    for rank, r in enumerate(res):
        d = pb.reg.decomp(rank)
        x[mpc.block(d)] = r[key]["x"].reshape(d.len[2], d.len[1], d.len[0])
    assert not np.isnan(x).any(), "the blocks do not tile the grid"
    return x.ravel()


def _both_overlap_modes(pb, b, specs):
    """the solves with the exchange of r hidden behind k_cg_Bq (overlap = 1, the default: the neighbour's ghost is r - alpha q of the stored q
    layers) and after it (0); -> the two lists of per-rank results, the second with "dprev" against the first"""
    on = inproc.run_threads(pb.size, _solve_worker, pb, b, specs, None)
    _knob("overlap", 0)
    try:
        off = inproc.run_threads(pb.size, _solve_worker, pb, b, specs, on)
    finally:
        _knob("overlap", 1)
    return on, off


def _check_modes_against_each_other(pb, on, off, keys):
    """tests/test_gpu_multirank.py::test_overlapped_exchange_changes_nothing on these grids: same iteration count and reason, history and x to 1e-12
    (a ghost formed as r - alpha q may differ from its owner's cell in the last bit), the first three history entries bit-equal.  Seen on these
    grids: in the runs of up to 11 iterations every history entry is bit-equal and x differs by at most 3.8e-16 of its maximum; in the converged
    solves the first 14 to 34 entries are bit-equal, then the histories part by up to 3.0e-14, x by up to 8.2e-15."""
    for key in keys:
        a, b_ = _agree(on, key), _agree(off, key)
        assert a["iters"] == b_["iters"] and a["reason"] == b_["reason"], key
        assert np.allclose(a["history"], b_["history"], rtol=1e-12, atol=0), key
        xmax = max(np.abs(r[key]["x"]).max() for r in on)
        dx = max(r[key]["dprev"] for r in off) / xmax
        same = int(np.argmin(np.append(a["history"] == b_["history"], False)))
        print("overlap 1 against 0", pb.reg.name, key, "x", dx, "history", np.abs(a["history"] / b_["history"] - 1).max(), "bit-equal entries", same)
        assert dx <= 1e-12, (key, dx)
        assert same >= min(3, len(a["history"])), (key, same)


def run_cg(pb, pc=fo.PC_JACOBI, ks=KS):
    """k_cg_A with q on the boundary layers only + k_cg_Bq + the pack of r - alpha q: x after 1, 2, 3, 8 and 11 iterations against the oracle to
    1e-10 of its maximum and the residual history to 1e-9 (tests/test_gpu_launch_regimes.py::test_cg_iterates_match_oracle; the twelve entries as
    tests/test_gpu_config5.py::_operator_worker), in both overlap modes, and the modes against each other."""
    S, b = pb.S, pb.rhs()
    specs, hist = [], None
    for k in ks:
        xo, io = S.solve(b, pc=pc, nullspace=pb.nullspace, rtol=0.0, atol=0.0, maxit=k)
        assert io["iters"] == k and io["reason"] == -3
        hist = io["history"]
        specs.append((k, dict(pc=pc, remove_nullspace=int(pb.nullspace), rtol=0.0, atol=0.0, maxit=k, history=True), xo))
    on, off = _both_overlap_modes(pb, b, specs)
    for mode, res in (("overlap 1", on), ("overlap 0", off)):
        for k, _, xo in specs:
            ig = _agree(res, k)
            assert ig["iters"] == k and ig["reason"] == -3, (mode, k, ig["iters"], ig["reason"])
            err = max(r[k]["err"] for r in res) / np.abs(xo).max()
            print("cg", pb.reg.name, mode, "pc", pc, "k", k, "x", err, "history", np.abs(ig["history"] / hist[:k + 1] - 1).max())
            assert err <= 1e-10, (mode, k, err)
            assert np.allclose(ig["history"], hist[:k + 1], rtol=1e-9, atol=0), (mode, k)
    _check_modes_against_each_other(pb, on, off, [k for k, _, _ in specs])


def run_cg_none(pb):
    """the same without a preconditioner (k_cg_A's other instantiation)"""
    run_cg(pb, pc=fo.PC_NONE)


def run_cg_head(pb):
    """the first three iterations (the stretched case)"""
    run_cg(pb, ks=(1, 2, 3))


def run_cg_converged(pb):
    """one solve to rtol 1e-6 in both overlap modes: the oracle's reason, its iteration count within one, the first residuals to 1e-9 and the true
    residual of the gathered x (tests/test_gpu_launch_regimes.py::test_cg_iterates_match_oracle)."""
    S, b = pb.S, pb.rhs()
    xo, io = S.solve(b, nullspace=pb.nullspace, rtol=1e-6, maxit=5000)
    rtrue = np.linalg.norm(b - S.mult(xo))
    specs = [("converged", dict(remove_nullspace=int(pb.nullspace), rtol=1e-6, maxit=5000, history=True), None)]
    on, off = _both_overlap_modes(pb, b, specs)
    for mode, res in (("overlap 1", on), ("overlap 0", off)):
        ig = _agree(res, "converged")
        print("cg converged", pb.reg.name, mode, "iterations", ig["iters"], "oracle", io["iters"])
        assert ig["reason"] == io["reason"] == 2 and abs(ig["iters"] - io["iters"]) <= 1, (mode, ig["iters"], io["iters"])
        assert np.allclose(ig["history"][:5], io["history"][:5], rtol=1e-9, atol=0), mode
        assert np.linalg.norm(b - S.mult(_gather_x(pb, res, "converged"))) <= 1.5 * rtrue + 1e-12 * np.linalg.norm(b), mode
    _check_modes_against_each_other(pb, on, off, ["converged"])


def run_cg_sr(pb):
    """KSPCG with -ksp_cg_single_reduction (fl_exchange_sr_begin / k_pack_faces_sr behind MODE 10): x after 3, 8 and 11 iterations and the history
    against the oracle's single-reduction recurrence, and ONE all-reduce per iteration by the wire's counter (+ iteration 0, + at most
    check_every - 1 enqueued behind the last one: tests/test_gpu_config5.py::_operator_worker)."""
    S, b = pb.S, pb.rhs()
    specs, hist = [], None
    for k in (3, 8, 11):
        xo, io = S.solve(b, nullspace=pb.nullspace, single_reduction=True, rtol=0.0, atol=0.0, maxit=k)
        assert io["iters"] == k and io["reason"] == -3
        hist = io["history"]
        specs.append((k, dict(cg_single_reduction=1, remove_nullspace=int(pb.nullspace), rtol=0.0, atol=0.0, maxit=k, history=True, check_every=8), xo))
    res = inproc.run_threads(pb.size, _solve_worker, pb, b, specs, None)
    for k, _, xo in specs:
        ig = _agree(res, k)
        assert ig["iters"] == k and ig["reason"] == -3, (k, ig["iters"], ig["reason"])
        err = max(r[k]["err"] for r in res) / np.abs(xo).max()
        print("cg_sr", pb.reg.name, "k", k, "x", err, "history", np.abs(ig["history"] / hist[:k + 1] - 1).max(), "all-reduces", ig["allreduces"])
        assert err <= 1e-10, (k, err)
        assert np.allclose(ig["history"], hist[:k + 1], rtol=1e-9, atol=0), k
        assert all(k + 1 <= r[k]["allreduces"] <= k + 8 for r in res), (k, [r[k]["allreduces"] for r in res])


def run_bcgs(pb):
    """Jacobi-BiCGStab, 5 iterations: the history against the oracle to 1e-9 (tests/test_gpu_launch_regimes.py::test_bicgstab_history_on_the_mid_plan)."""
    S = pb.S
    b = np.random.default_rng(9).standard_normal(pb.g.ncell)
    xo, io = S.solve(b, ksp=fo.KSP_BCGS, pc=fo.PC_JACOBI, nullspace=pb.nullspace, rtol=0.0, atol=0.0, maxit=5)
    specs = [("bcgs", dict(type=1, pc=fo.PC_JACOBI, remove_nullspace=int(pb.nullspace), rtol=0.0, atol=0.0, maxit=5, history=True, check_every=5), xo)]
    res = inproc.run_threads(pb.size, _solve_worker, pb, b, specs, None)
    ig = _agree(res, "bcgs")
    assert ig["iters"] == io["iters"] == 5 and ig["reason"] == io["reason"], (ig["iters"], ig["reason"], io["iters"], io["reason"])
    m = min(len(ig["history"]), len(io["history"]))
    print("bcgs", pb.reg.name, "history", np.abs(ig["history"][:m] / io["history"][:m] - 1).max(), "x", max(r["bcgs"]["err"] for r in res) / np.abs(xo).max())
    assert m >= 5 and np.allclose(ig["history"][:m], io["history"][:m], rtol=1e-9, atol=0)


def run_cheb(pb, all_steps=(7, 20)):
    """fl_fill_ghosts_deep (two layers, edge cells in two hops) feeding k_cheb2 with two ghost rings, in its clamped plan: 7 steps (three fused pairs and
    a single step) and 20 with the default cheb_fuse against the oracle's KSPCHEBYSHEV + PCJACOBI to 1e-12 of its maximum
    (tests/test_gpu_launch_regimes.py::test_fused_chebyshev_matches_oracle); one launch per pair of steps on every rank (the ranks voted for the
    fused kernel); and against cheb_fuse = 0 on the same ranks to 1e-13 (tests/test_gpu_config5.py::_smoother_worker: the same arithmetic per cell)."""
    assert all(launch_plans(blk)["cheb2.clamp"] == 1 for blk in pb.reg.blocks)
    S, b = pb.S, pb.rhs()
    lam = S.gershgorin(fo.PC_JACOBI)
    emin, emax = 0.1 * lam, 1.1 * lam
    specs = []
    for steps in all_steps:
        xo, io = S.solve(b, ksp=fo.KSP_CHEBYSHEV, pc=fo.PC_JACOBI, norm=fo.NORM_NONE, nullspace=pb.nullspace, maxit=steps, emin=emin, emax=emax, history=False)
        assert io["iters"] == steps and io["reason"] == 4
        specs.append((steps, dict(type=2, pc=fo.PC_JACOBI, norm_type=fo.NORM_NONE, remove_nullspace=int(pb.nullspace), maxit=steps, emin=emin, emax=emax,
                                  check_every=100, profile=1), xo))
    fused = inproc.run_threads(pb.size, _solve_worker, pb, b, specs, None)
    _knob("cheb_fuse", 0)
    try:
        single = inproc.run_threads(pb.size, _solve_worker, pb, b, specs, None)
    finally:
        _knob("cheb_fuse", 1)
    for steps, _, xo in specs:
        for mode, res, launches in (("fused", fused, steps // 2), ("cheb_fuse 0", single, steps)):
            ig = _agree(res, steps)
            assert ig["iters"] == steps and ig["reason"] == 4, (mode, steps, ig["iters"], ig["reason"])
            assert all(r[steps]["kernel_launches"] == launches for r in res), (mode, steps, [r[steps]["kernel_launches"] for r in res])
            err = max(r[steps]["err"] for r in res) / np.abs(xo).max()
            print("cheb", pb.reg.name, mode, "steps", steps, "x", err)
            assert err <= 1e-12, (mode, steps, err)
        d2 = sum(((f[steps]["x"] - u[steps]["x"]) ** 2).sum() for f, u in zip(fused, single))
        n2 = sum((u[steps]["x"] ** 2).sum() for u in single)
        print("cheb", pb.reg.name, "fused against cheb_fuse 0, steps", steps, np.sqrt(d2 / n2))
        assert np.sqrt(d2 / n2) <= 1e-13, (steps, np.sqrt(d2 / n2))


def run_cheb7(pb):
    """7 steps (the stretched case)"""
    run_cheb(pb, all_steps=(7,))


RUN = {"operator": run_operator, "cg": run_cg, "cg_none": run_cg_none, "cg_head": run_cg_head, "cg_converged": run_cg_converged, "cg_sr": run_cg_sr,
       "bcgs": run_bcgs, "cheb": run_cheb, "cheb7": run_cheb7}


@pytest.mark.parametrize("name,piece", RUNS, ids=[f"{n}-{p}" for n, p in RUNS])
def test_rank_blocks_in_the_8_wave_plans_match_the_oracle(name, piece):
    """A piece (run_<piece> above says what it checks and where its tolerances come from) of a problem of PROBLEMS; the pieces of a problem follow
    each other and share its oracle grid and matrix."""
    RUN[piece](_problem(name))


# ------------------------------------------------------------------------------------------------ k_schur_var_ring at 128 blocks per XCD

SCHUR = [r for r in RANK_BY_NAME if r.startswith("ranks_schur")]


def _schur_worker(R, pb, reg, kind):
    """tests/test_gpu_schur_var_multirank.py::_product_worker for one momentum state, with the checks every rank of this module makes"""
    import torch
    from tests import test_gpu_schur_var_multirank as T
    P, M, d, s = T._session(R, pb, R.rank)
    info = P.comm_info()
    assert info["nranks"] == R.size == int(np.prod(reg.ranks)), info
    ln = [int(d.len[a]) for a in range(3)]
    assert tuple(ln) == reg.blocks[R.rank] and launch_plans(ln)["schur.per_xcd"] == 128
    cell, face = T._blocks(pb, d)
    with torch.cuda.stream(s):
        M.set_ainv_types(schur=kind)
        dt, rho = pb.states[0]
        M.set_state(dt, rho, pb.mu, [T._dev(face(pb.V0[a], a)) for a in range(3)], [T._dev(face(pb.W[c * 3 + a], a)) for c in range(3) for a in range(3)])
        y = M.schur_apply(T._dev(cell(pb.p)))
        a = M.diagonal() if kind == fo.AINV_DIAG else M.rowsum()
        s.synchronize()
        out = [y.cpu().numpy()] + list(a.cpu().numpy().reshape(3, -1))
    M.close()
    P.close()
    return dict(lo=[int(d.lo[a]) for a in range(3)], ln=ln, y=out)


@pytest.mark.parametrize("name", SCHUR)
def test_schur_product_on_rank_blocks_at_128_blocks_per_xcd(name):
    """k_schur_var_ring (DIAG and ROWSUM) at its full launch, with and without a fixed x segment, the ring on each axis in turn: the gathered product
    of the ranks against the oracle's fo.abf_schur_apply (2e-10) and the seven-kernel composition on the same ranks (schur_var_fused = 0, 1e-12) as
    tests/test_gpu_launch_regimes.py::test_schur_complement_at_128_blocks_per_xcd, with its momentum state (amplitude tied to the finest spacing, so
    that the row sums stay away from zero) and its assertions on 1 / ainv; and bit for bit against the one-rank fused product of the global grid
    (tests/test_gpu_schur_var_multirank.py::_same_bits, its cap on the cells held to 1e-15 unchanged).  Measured: ROWSUM no such cell on any grid;
    DIAG 276 (y split), 7390 and 12023 (z splits) and, on the x splits, 215691 of 1349760 and 178430 of 888000 cells (16 % and 20 %; the cap is 25 %:
    see the table for why an x split moves so many)."""
    from tests import test_gpu_schur_var_multirank as T
    reg = RANK_BY_NAME[name]
    size = int(np.prod(reg.ranks))
    for bc in reg.bcs:
        pb = T._Problem(reg.n, reg.ranks, reg.own, bc)
        g = pb.g
        amp = 75 * min(float(np.diff(xf).min()) for xf in pb.xf)
        rng = np.random.default_rng(3)
        pb.V0 = [amp * rng.standard_normal(g.nface[d]) for d in range(3)]
        pb.W = [amp * rng.standard_normal(g.nface[d]) for c in range(3) for d in range(3)]
        A = pb.A(0)
        for kind in (fo.AINV_DIAG, fo.AINV_ROWSUM):
            ainv = fo.abf_ainv(A, kind)
            assert np.abs(1.0 / ainv).min() >= 0.25 and np.abs(1.0 / ainv - 1.0).max() > 1e-2, kind   # well conditioned, and not the ID type
            want = fo.abf_schur_apply(g, ainv, pb.p)
            one = T._product_worker(None, pb, kind, 1)["y"]
            parts = inproc.run_threads(size, _schur_worker, pb, reg, kind)
            fused = [T._gather(pb, parts, c) for c in range(4)]
            T._knob("schur_var_fused", 0)
            try:
                parts = inproc.run_threads(size, _schur_worker, pb, reg, kind)
            finally:
                T._knob("schur_var_fused", 1)
            comp = T._gather(pb, parts, 0)
            scale = np.abs(want).max()
            print("schur", name, "kind", kind, "oracle", np.abs(fused[0] - want).max() / scale, "composition", np.abs(fused[0] - comp).max() / np.abs(comp).max())
            assert np.abs(fused[0] - want).max() <= 2e-10 * scale, kind
            assert np.abs(fused[0] - comp).max() <= 1e-12 * np.abs(comp).max(), kind
            moved = T._same_bits(pb, fused, one[:4])
            print("schur", name, "kind", kind, "cells held to 1e-15 instead of bit for bit:", moved, "of", g.ncell)
