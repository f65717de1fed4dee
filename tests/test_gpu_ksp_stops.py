"""-m gpu: how the Krylov solves stop -- every reason the public API can reach, the iterate at the stop, and the next solve on the handle.

The cases are those of tests/ksp_stops.py (tests/test_ksp_stops.py holds the oracle to them on the CPU).  Parts A to D, F and G compare with the
oracle: reason and iterations exactly, histories to 1e-9, x of a diverging solve to 100 times the oracle's own answer to a 1e-16 perturbation of b.
Part E needs no oracle: after a solve that ended with NaN, Inf or a divergence, the next solve on the handle must be bit for bit that of a handle
created fresh.  Figures are printed before they are asserted."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fluca_amd import capi
from tests import ksp_stops as ks
from tests.gpu_common import dev, host, stretched_faces

pytestmark = pytest.mark.gpu

KNOBS = (b"cg_xdepth", b"cg_xbatch", b"cheb_fuse")


def _knob(name, value):
    capi.check(capi.lib.fl_tuning_set(name, value), "fl_tuning_set")


def _knob_get(name):
    v = C.c_int(0)
    capi.check(capi.lib.fl_tuning_get(name, C.byref(v)), "fl_tuning_get")
    return v.value


@pytest.fixture
def restore_knobs():
    keep = {k: _knob_get(k) for k in KNOBS}
    try:
        yield
    finally:
        for k, v in keep.items():
            _knob(k, v)


def _poisson(n, bc):
    from fluca_amd.poisson import Poisson
    return Poisson(n, stretched_faces(n), list(bc), ks.KAPPA)


def _momentum(n):
    """(Poisson, Momentum) on the stretched grid n with the state of ks.momentum handed over with v0 (k_mom3 where ny > 8)"""
    from fluca_amd.poisson import Momentum
    P = _poisson(n, ks.MOM_BC[n])
    M = Momentum(P)
    s = ks.momentum(n)
    M.set_state(s.dt, s.rho, s.mu, [dev(a) for a in s.V0], M.interp_faces(dev(s.v0)), v0=dev(s.v0))
    return P, M


def _weight(M, n, w):
    s = ks.momentum(n)
    M.set_coefficients(1.0, w * s.dt, -0.5 * s.mu * s.dt / s.rho)


@pytest.fixture(scope="module")
def handles():
    """one handle per (kind, grid, boundary types) for the module: get(case) -> Poisson or Momentum.  The cases of parts A to D therefore run on a
    handle that has seen the NaN, Inf and diverging solves of the cases before them, which is meant; a failure there may depend on the order of the
    tests, where a failure of part E (a handle of its own per test) does not."""
    live = {}

    def get(case):
        key = (case.handle, case.n, case.bc)
        if key not in live:
            live[key] = _momentum(case.n) if case.handle == "momentum" else (_poisson(case.n, case.bc), None)
        P, M = live[key]
        return P if M is None else M

    yield get
    for P, M in live.values():
        if M is not None:
            M.close()
        P.close()


def _run(case, H, b=None, **over):
    kw = ks.gpu_opts(case)
    kw.update(over)
    history = kw.get("norm_type") != ks.NONORM          # no norm, no history
    x = dev(ks.momentum_guess(case.n)) if case.guess else None
    xg, ig = H.solve(dev(case.b() if b is None else b), x=x, history=history, **kw)
    return xg, ig


def _family(case):
    return case.name[2:].rsplit("-", 1)[0]


FAMILIES_A = sorted({_family(c) for c in ks.cases("A")})


@pytest.mark.parametrize("family", FAMILIES_A)
def test_A_reasons_at_iteration_zero(family, handles):
    cs = [c for c in ks.cases("A") if _family(c) == family]
    assert cs
    for c in cs:
        xg, ig = _run(c, handles(c))
        print(c, ig["reason"], ig["iters"], ig["rnorm0"])
        assert (ig["reason"], ig["iters"]) == (c.reason, 0), (c, ig["reason"], ig["iters"])
        poisoned_b = len(c.rhs) > 1
        if not poisoned_b:
            assert torch.count_nonzero(xg).item() == 0, c            # the zero guess, exactly
        normed = c.opts.get("norm_type") != ks.NONORM
        if poisoned_b:
            assert not np.isfinite(ig["rnorm0"]) and not np.isfinite(ig["history"][0]), c
        elif c.oracle and normed:
            _, io = ks.oracle_solve(c)
            want = io["history"][0]
            assert ig["rnorm0"] == ig["history"][0] == ig["rnorm"], c
            assert abs(ig["rnorm0"] - want) <= ks.HIST_RTOL * want, (c, ig["rnorm0"], want)
        elif normed:            # MG-PCG: no oracle at this size; the norm of M b is finite, and zero only for b = 0
            assert np.isfinite(ig["rnorm0"]) and (ig["rnorm0"] > 0.0) == (c.rhs[0] != "zero"), c


def _x_close(c, xg, xo):
    """x of a converging solve stopped where the oracle stopped: the tolerances the parity suite holds such iterates to"""
    xg = host(xg)
    if c.guess:             # tests/test_gpu_momentum_regimes.py::test_chebyshev_from_a_nonzero_guess: the correction the solve made
        x0 = ks.momentum_guess(c.n)
        err, scale = np.linalg.norm((xg - x0) - (xo - x0)), np.linalg.norm(xo - x0)
    elif c.handle == "momentum":
        err, scale = np.linalg.norm(xg - xo), np.linalg.norm(xo)
    else:
        err, scale = np.abs(xg - xo).max(), np.abs(xo).max()
    print(c, "x error", err / scale)
    assert err <= ks.X_RTOL * scale, (c, err / scale)


@pytest.mark.parametrize("c", ks.cases("B"), ids=[c.name for c in ks.cases("B")])
def test_B_atol_against_rtol_in_mid_solve(c, handles):
    xg, ig = _run(c, handles(c))
    xo, io = ks.oracle_solve(c)
    print(c, ig["reason"], ig["iters"], ig["rnorm"], ig["rnorm0"], "oracle", io["reason"], io["iters"], io["rnorm"], io["rnorm0"])
    assert (ig["reason"], ig["iters"]) == (c.reason, c.iters), (c, ig["reason"], ig["iters"])
    assert abs(ig["rnorm0"] - io["rnorm0"]) <= ks.HIST_RTOL * io["rnorm0"], (c, ig["rnorm0"], io["rnorm0"])
    if c.reason == ks.ATOL:
        assert ig["rnorm"] < c.opts["atol"], (c, ig["rnorm"])
    else:
        assert ig["rnorm"] <= c.opts["rtol"] * ig["rnorm0"], (c, ig["rnorm"], ig["rnorm0"])
    hg, ho = ig["history"], io["history"]
    assert len(hg) == len(ho) == c.iters + 1
    print(c, "history", np.abs(hg / ho - 1.0).max())
    assert np.allclose(hg, ho, rtol=ks.HIST_RTOL, atol=0), (c, hg, ho)
    _x_close(c, xg, xo)


def _diverging(c, ig, xg):
    """reason, iterations, history and x of a diverging solve at its stop against the oracle -> host x"""
    xo, io = ks.oracle_solve(c)
    k = c.iters
    hg, ho = ig["history"], io["history"]
    xh = host(xg)
    err = np.abs(xh - xo).max() / np.abs(xo).max()
    print(c, ig["reason"], ig["iters"], "history", np.abs(hg[:k + 1] / ho[:k + 1] - 1.0).max() if len(hg) > k else hg, "x error", err,
          "allowed", ks.X_NOISE_FACTOR * c.xtol)
    assert (ig["reason"], ig["iters"]) == (c.reason, k), (c, ig["reason"], ig["iters"])
    assert len(hg) == k + 1 and np.allclose(hg, ho[:k + 1], rtol=ks.HIST_RTOL, atol=0), (c, hg, ho)
    assert err <= ks.X_NOISE_FACTOR * c.xtol, (c, err)
    return xh


RING = ks.ring_cases()


@pytest.mark.parametrize("c", RING, ids=[c.name for c in RING])
def test_CF_cg_stops_inside_a_polling_window_with_updates_owed(c, handles, restore_knobs):
    """DIVERGED_DTOL / DIVERGED_INDEFINITE_MAT at an iteration that is no multiple of the ring depth, check_every at its default: the queued launches
    behind the stop do nothing, k_cg_finish adds exactly the updates owed; at every ring depth and with one update per iteration x is the same, bit
    for bit"""
    H = handles(c)
    xs = []
    for depth, batch in ((8, 1), (2, 1), (16, 1), (8, 0)):
        _knob(b"cg_xdepth", depth)
        _knob(b"cg_xbatch", batch)
        xg, ig = _run(c, H)
        _diverging(c, ig, xg)
        xs.append((depth, batch, xg, ig["rnorm"]))
    for depth, batch, xg, rn in xs[1:]:
        assert torch.equal(xg, xs[0][2]) and rn == xs[0][3], (c, depth, batch)


OTHERS = [c for c in ks.cases("C") if c not in RING and c.opts["type"] != ks.CHEB]


@pytest.mark.parametrize("c", OTHERS, ids=[c.name for c in OTHERS])
def test_C_dtol_in_mid_solve(c, handles):
    xg, ig = _run(c, handles(c))
    _diverging(c, ig, xg)


CHEB_C = [c for c in ks.cases("C") if c.opts["type"] == ks.CHEB]


@pytest.mark.parametrize("c", CHEB_C, ids=[c.name for c in CHEB_C])
def test_C_chebyshev_dtol_whatever_cheb_fuse(c, handles, restore_knobs):
    """a monitored Chebyshev solve takes one step per launch whatever "cheb_fuse" says (the fused sweep is legal without a norm only): same stop, same x"""
    H = handles(c)
    out = []
    for mode in (0, 2):
        _knob(b"cheb_fuse", mode)
        xg, ig = _run(c, H)
        _diverging(c, ig, xg)
        out.append((xg, ig))
    assert torch.equal(out[0][0], out[1][0]) and np.array_equal(out[0][1]["history"], out[1][1]["history"])


@pytest.mark.parametrize("c", ks.cases("D"), ids=[c.name for c in ks.cases("D")])
def test_D_momentum_chebyshev_is_watched_on_its_default_interval(c, handles):
    M = handles(c)
    A = ks.momentum_A(c.n, c.weight)
    try:
        _weight(M, c.n, c.weight)
        emin, emax = M.chebyshev_interval()
        want = ks.momentum_interval(A)
        # a diagonal entry near zero is a difference of numbers of size one: its reciprocal, hence the radius, carries their rounding 1 / |a_ii| times
        print(c, "interval", (emin, emax), want)
        assert abs(emin - want[0]) <= 1e-10 * want[0] and abs(emax - want[1]) <= 1e-10 * want[1], ((emin, emax), want)
        xg, ig = _run(c, M)
        xo, io = ks.oracle_solve(c)
        print(c, ig["reason"], ig["iters"], "oracle", io["reason"], io["iters"])
        assert ig["reason"] == c.reason, (c, ig["reason"], ig["iters"])
        if c.reason == ks.DIV_DTOL:
            assert 0 < ig["iters"] < c.opts["maxit"], (c, ig["iters"])
            assert ig["rnorm"] >= 1e5 * ig["rnorm0"] > 0.0, (c, ig["rnorm"], ig["rnorm0"])
        else:
            assert ig["iters"] == c.opts["maxit"] == ks.D_BENIGN_STEPS
            assert np.linalg.norm(host(xg) - xo) <= ks.X_RTOL * np.linalg.norm(xo)
    finally:
        _weight(M, c.n, 1.0)


# ------------------------------------------------------------------------------------------------ E: the handle after a bad solve

E_GRID, E_BC = ks.FUSED, tuple(ks.CAVITY)      # every family runs here: the fused Chebyshev sweep, the multigrid levels, six walls
E_OPTS = {
    "cg": dict(type=ks.CG, pc=ks.JACOBI),
    "cg-none": dict(type=ks.CG, pc=ks.NOPC),
    "cgsr": dict(type=ks.CG, pc=ks.JACOBI, cg_single_reduction=1),
    "bcgs": dict(type=ks.BCGS, pc=ks.JACOBI),
    "cheb": dict(type=ks.CHEB, pc=ks.JACOBI),
    "cheb-nonorm": dict(type=ks.CHEB, pc=ks.JACOBI, norm_type=ks.NONORM),
    "mg": dict(type=ks.CG, pc=ks.MG),
}
E_PAIRS = [("cg", "cg"), ("cg", "bcgs"), ("bcgs", "cg"), ("cheb-nonorm", "cg"), ("mg", "mg"),
           ("cg-none", "cg-none"), ("cgsr", "cgsr"), ("cgsr", "cg"), ("bcgs", "bcgs"), ("cheb", "cheb"), ("cheb-nonorm", "cheb-nonorm"), ("cheb", "cg"),
           ("cg", "cgsr"), ("cg", "cheb"), ("mg", "cg"), ("cg", "mg"), ("bcgs", "cheb"), ("cheb-nonorm", "bcgs"),
           # twelve unwatched steps on a NaN fill every vector Chebyshev shares with the others; a NaN cycle fills those of every multigrid level
           ("cheb-nonorm", "cgsr"), ("cheb-nonorm", "cheb"), ("cheb-nonorm", "mg"), ("mg", "bcgs"), ("mg", "cgsr"), ("mg", "cheb"), ("mg", "cheb-nonorm")]
E_GOOD = dict(rtol=1e-6, maxit=30)


def _same(a, b):
    (xa, ia), (xb, ib) = a, b
    ha, hb = ia.get("history"), ib.get("history")
    return (torch.equal(xa, xb) and (ia["iters"], ia["reason"], ia["rnorm0"], ia["rnorm"]) == (ib["iters"], ib["reason"], ib["rnorm0"], ib["rnorm"])
            and (ha is None or np.array_equal(ha, hb)))


@pytest.fixture(scope="module")
def fresh_poisson():
    """(x, info) of the finite solve of a family on a handle that has solved nothing else; computed once, left unchanged"""
    ref = {}

    def get(n, bc, good, b):
        key = (n, bc, good)
        if key not in ref:
            P = _poisson(n, bc)
            ref[key] = P.solve(dev(b), history=E_OPTS[good].get("norm_type") != ks.NONORM, **dict(E_OPTS[good], **E_GOOD))
            P.close()
        return ref[key]

    return get


@pytest.mark.parametrize("bad,good", E_PAIRS, ids=[f"{a}-then-{b}" for a, b in E_PAIRS])
def test_E_next_solve_after_a_nan_is_that_of_a_fresh_handle(bad, good, fresh_poisson):
    """b1 holds one NaN, next to each wall in turn (where 0 x NaN in a ghost would show) and in the interior; then a finite b2 on the same handle"""
    b2 = ks.poisson_rhs(E_GRID, E_BC, ("consistent",))
    want = fresh_poisson(E_GRID, E_BC, good, b2)
    assert np.isfinite(want[1]["rnorm"]) and want[1]["iters"] > 3
    P = _poisson(E_GRID, E_BC)
    v = dev(np.random.default_rng(3).standard_normal(P.ncell))
    for where in ks.WHERE:
        b1 = ks.poisson_rhs(E_GRID, E_BC, ("consistent", "nan", where))
        nonorm = E_OPTS[bad].get("norm_type") == ks.NONORM
        _, i1 = P.solve(dev(b1), **dict(E_OPTS[bad], maxit=12))
        assert (i1["reason"], i1["iters"]) == ((ks.ITS, 12) if nonorm else (ks.DIV_NANORINF, 0)), (bad, where, i1)
        assert torch.isfinite(P.apply(v)).all(), (bad, where)
        got = P.solve(dev(b2), history=E_OPTS[good].get("norm_type") != ks.NONORM, **dict(E_OPTS[good], **E_GOOD))
        assert _same(got, want), (bad, good, where, got[1], want[1])
    P.close()


E_AFTER_DTOL = [("C-pcg", "cg"), ("C-pcg", "bcgs"), ("C-cg", "cg-none"), ("C-cgsr", "cgsr"), ("C-cgsr", "cg"), ("C-bcgs", "bcgs"), ("C-bcgs", "cg"),
                ("C-cheb-half", "cheb"), ("C-cheb-half", "cg"), ("F-cg", "cg-none"), ("F-pcg", "cg"),
                # the multigrid levels carry poisoned flags of their own; the fused sweep of the norm-less Chebyshev shares X1 and d with the others
                ("C-cheb-half", "mg"), ("C-cheb-half", "cheb-nonorm"), ("C-pcg", "mg"), ("C-pcg", "cheb-nonorm"), ("C-bcgs", "mg"), ("F-pcg", "mg")]


@pytest.mark.parametrize("bad,good", E_AFTER_DTOL, ids=[f"{a}-then-{b}" for a, b in E_AFTER_DTOL])
def test_E_next_solve_after_a_divergence_is_that_of_a_fresh_handle(bad, good, fresh_poisson):
    c = ks.STOP[bad]
    b2 = ks.poisson_rhs(c.n, c.bc, ("consistent",))
    want = fresh_poisson(c.n, c.bc, good, b2)
    P = _poisson(c.n, c.bc)
    _, i1 = _run(c, P)
    assert (i1["reason"], i1["iters"]) == (c.reason, c.iters), (c, i1)
    got = P.solve(dev(b2), history=E_OPTS[good].get("norm_type") != ks.NONORM, **dict(E_OPTS[good], **E_GOOD))
    assert _same(got, want), (bad, good, got[1], want[1])
    P.close()


OVERFLOW = dict(scale=1e150, dtol=1e300)      # the diverging Chebyshev of part C on 1e150 b: the square sums overflow a few steps in


@pytest.mark.parametrize("good", ["cg", "cgsr", "bcgs", "cheb", "cheb-nonorm", "mg"])
def test_E_next_solve_after_an_overflow_in_mid_solve(good, fresh_poisson):
    """DIVERGED_NANORINF in mid-solve, with Inf and NaN in the work vectors the solvers share (ks.overflow_stop is the oracle's side of it)"""
    c = ks.STOP["C-cheb-half"]
    b2 = ks.poisson_rhs(c.n, c.bc, ("consistent",))
    want = fresh_poisson(c.n, c.bc, good, b2)
    P = _poisson(c.n, c.bc)
    _, i1 = _run(c, P, b=OVERFLOW["scale"] * c.b(), dtol=OVERFLOW["dtol"])
    print("overflow", i1["reason"], i1["iters"], "oracle", ks.overflow_stop(c, **OVERFLOW))
    assert i1["reason"] == ks.DIV_NANORINF and 0 < i1["iters"] < c.opts["maxit"], i1
    assert torch.isfinite(P.apply(dev(b2))).all()
    got = P.solve(dev(b2), history=E_OPTS[good].get("norm_type") != ks.NONORM, **dict(E_OPTS[good], **E_GOOD))
    assert _same(got, want), (good, got[1], want[1])
    P.close()


M_OPTS = {"bcgs": dict(type=ks.BCGS, pc=ks.JACOBI), "gmres": dict(type=ks.GMRES, pc=ks.JACOBI), "cheb": dict(type=ks.CHEB, pc=ks.JACOBI),
          "cheb-nonorm": dict(type=ks.CHEB, pc=ks.JACOBI, norm_type=ks.NONORM)}
M_PAIRS = [("bcgs", "bcgs"), ("gmres", "bcgs"), ("cheb", "cheb"), ("gmres", "gmres"), ("bcgs", "cheb"), ("cheb-nonorm", "bcgs"), ("cheb", "gmres")]
M_GOOD = dict(rtol=1e-8, maxit=40)


@pytest.fixture(scope="module")
def fresh_momentum():
    ref = {}

    def get(n, good, b):
        if (n, good) not in ref:
            P, M = _momentum(n)
            ref[n, good] = M.solve(dev(b), history=True, **dict(M_OPTS[good], **M_GOOD))
            M.close()
            P.close()
        return ref[n, good]

    return get


@pytest.mark.parametrize("n", [ks.MOM3, ks.MOM2], ids=["mom3", "mom2"])
@pytest.mark.parametrize("bad,good", M_PAIRS, ids=[f"{a}-then-{b}" for a, b in M_PAIRS])
def test_E_momentum_handle_after_a_nan(bad, good, n, fresh_momentum):
    """fl_momentum_solve zeroes nothing between solves: a NaN in b1 must not reach the solve of b2 through a work vector or a wall ghost"""
    b2 = ks.momentum_rhs(n, ("random",))
    want = fresh_momentum(n, good, b2)
    assert want[1]["reason"] == ks.RTOL
    P, M = _momentum(n)
    v = dev(np.random.default_rng(3).standard_normal(3 * P.ncell))
    for where in ks.WHERE:
        b1 = ks.momentum_rhs(n, ("random", "nan", where))
        _, i1 = M.solve(dev(b1), **dict(M_OPTS[bad], maxit=12))
        assert (i1["reason"], i1["iters"]) == (ks.DIV_NANORINF, 0), (bad, where, i1)      # the watched Chebyshev included
        assert torch.isfinite(M.apply(v)).all(), (bad, where)
        got = M.solve(dev(b2), history=True, **dict(M_OPTS[good], **M_GOOD))
        assert _same(got, want), (bad, good, where, got[1], want[1])
    M.close()
    P.close()


@pytest.mark.parametrize("good", ["cheb", "bcgs", "gmres"])
def test_E_momentum_handle_after_a_divergence(good, fresh_momentum):
    c = ks.STOP["D-mom3-diverges"]
    b2 = ks.momentum_rhs(c.n, ("random",))
    want = fresh_momentum(c.n, good, b2)
    P, M = _momentum(c.n)
    _weight(M, c.n, c.weight)
    _, i1 = _run(c, M)
    assert i1["reason"] == ks.DIV_DTOL, i1
    _weight(M, c.n, 1.0)
    got = M.solve(dev(b2), history=True, **dict(M_OPTS[good], **M_GOOD))
    assert _same(got, want), (good, got[1], want[1])
    M.close()
    P.close()


# ------------------------------------------------------------------------------------------------ G: several ranks

G_RANKS = (2, 1, 1)


def _rank_worker(R, case, specs):
    """the solves of specs = [(key, b, options)] one after the other on this rank's handle -> {key: (block of x, info)}"""
    from tests import mp_common as mpc
    from tests.test_gpu_config5 import _handle
    P, d, s = _handle(R, case)
    out = {}
    with torch.cuda.stream(s):
        for key, b, kw in specs:
            bd = torch.as_tensor(np.ascontiguousarray(b.reshape(case.shp)[mpc.block(d)]).ravel(), device="cuda")
            xg, ig = P.solve(bd, history=True, **kw)
            s.synchronize()
            out[key] = (xg.cpu().numpy(), ig, d)
    P.close()
    return out


def test_G_two_ranks_leave_a_bad_solve_together_and_the_next_is_clean():
    """2 x 1 x 1 ranks on the host transport.  The scalar kernels of every rank see the all-reduced sums alone (fin_step), so the reason is the same
    on both and both leave polled_loop at the same poll: DIVERGED_DTOL of part C at the oracle's iteration, then a NaN that only rank 1 owns, then
    a finite right-hand side -- whose solve is that of ranks that solved nothing else."""
    from tests import inproc
    from tests import mp_common as mpc
    c = ks.STOP["C-pcg"]
    n = c.n
    case = SimpleNamespace(n=n, ranks=G_RANKS, own=None, xf=stretched_faces(n), bc=list(c.bc), kappa=ks.KAPPA, shp=(n[2], n[1], n[0]))
    b2 = ks.poisson_rhs(n, c.bc, ("consistent",))
    bnan = ks.poisson_rhs(n, c.bc, ("consistent", "nan", "x+"))
    assert ks.cell(n, "x+") % n[0] >= (n[0] + 1) // 2           # in rank 1's block
    good = dict(type=ks.CG, pc=ks.JACOBI, rtol=1e-6, maxit=30)
    specs = [("dtol", c.b(), ks.gpu_opts(c)), ("nan", bnan, dict(type=ks.CG, pc=ks.JACOBI, maxit=30)), ("clean", b2, good)]
    res = inproc.run_threads(2, _rank_worker, case, specs)
    ref = inproc.run_threads(2, _rank_worker, case, specs[2:])
    for key in ("dtol", "nan", "clean"):
        i0, i1 = res[0][key][1], res[1][key][1]
        assert (i0["reason"], i0["iters"]) == (i1["reason"], i1["iters"]), (key, i0, i1)
        assert np.array_equal(i0["history"], i1["history"], equal_nan=True), key
    xo, io = ks.oracle_solve(c)
    ig = res[0]["dtol"][1]
    x = np.full(case.shp, np.nan)
    for r in res:
        xb, _, d = r["dtol"]
        x[mpc.block(d)] = xb.reshape(d.len[2], d.len[1], d.len[0])
    err = np.abs(x.ravel() - xo).max() / np.abs(xo).max()
    print("two ranks", c, ig["reason"], ig["iters"], "history", np.abs(ig["history"] / io["history"] - 1.0).max(), "x error", err)
    assert (ig["reason"], ig["iters"]) == (c.reason, c.iters)
    assert np.allclose(ig["history"], io["history"], rtol=ks.HIST_RTOL, atol=0)
    assert err <= ks.X_NOISE_FACTOR * c.xtol, err
    assert (res[0]["nan"][1]["reason"], res[0]["nan"][1]["iters"]) == (ks.DIV_NANORINF, 0)
    for r, f in zip(res, ref):
        (xa, ia, _), (xb, ib, _) = r["clean"], f["clean"]
        assert np.array_equal(xa, xb) and (ia["iters"], ia["reason"]) == (ib["iters"], ib["reason"]) and np.array_equal(ia["history"], ib["history"])
        assert np.isfinite(xa).all() and ia["iters"] > 3
