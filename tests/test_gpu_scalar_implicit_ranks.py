"""-m gpu: the implicit scalar diffusion on rank grids (include/fluca_hip_implicit_ranks.h), the ranks as threads of one process (tests/inproc.py), against
the one-rank calls of include/fluca_hip_implicit.h on the GLOBAL grid.

THE CONTRACT IS BITWISE: a cell of a rank's block runs the operations of the one-rank kernel on the same operands, so the gathered apply, solve and IMEX
step equal the one-rank results on their int64 views, on every case of tests/scalar_implicit_ranks.py, and info is the one-rank info on every rank.  That alone
would pass if both kernels shared a mistake, so two steps on config 5's rank grid are also held to the long-double recurrence within the derived bound of
tests/test_gpu_scalar_implicit.py.  The wire is counted from geometry: exchanges, messages and bytes per call must equal the count exactly, and no call
reduces anything.  Every caller array of every case stands 8 bytes off a 16-byte boundary between guards (tests/caller_arrays.py).

Every rank grid runs in one process with at most 8 threads; the one-rank reference of a global grid is computed once and shared by the cases on it."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import inproc
from tests import scalar_cases as sc
from tests import scalar_implicit_ranks as irk
from tests import scalar_ranks as rk

pytestmark = pytest.mark.gpu

CASES = irk.cases()
JOBS = ("apply", "solve", "solve2", "imex1.0", "imex0.5")
S, RTOL, MAXIT = irk.STAGES, irk.RTOL, irk.MAXIT
SMALL = rk.Case((7, 5, 6), (2, 1, 1), "channel", uniform=False, own=[(5, 2), (5,), (6,)])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.int64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _dev(a):
    from tests.gpu_common import dev
    return dev(np.ascontiguousarray(a, dtype=np.float64).reshape(-1))


def _host(t):
    from tests.gpu_common import host
    return host(t).copy()


# ------------------------------------------------------------------------------------------------------------------ the one-rank calls on the global grid

def one_rank_jobs(I, n, uniform, kinds, vals, jobs=JOBS, entry=""):
    """-> {job: field}, {job: info}: fl_scalar_diffusion_apply / _solve / fl_scalar_step_imex on one handle over the whole grid (entry "_ranks": through the
    collective names, which on a one-rank handle are the plain calls)"""
    from fluca_amd import capi
    from fluca_amd.poisson import Poisson
    from fluca_amd.scalar import Scalar
    Pz = Poisson(n, sc.faces(n, uniform), sc.poisson_bc(kinds), 1e-3)
    Sc = Scalar(Pz, kinds, vals, gamma=I["gamma"])
    assert not Sc.several
    if entry:
        Sc._implicit = lambda name: (getattr(capi.lib, name + entry), name + entry)
    Sc.set_velocity(*[_dev(v) for v in I["V"]])
    out, info = {}, {}
    shape = (n[2], n[1], n[0])
    for job in jobs:
        if job == "apply":
            out[job] = _host(Sc.diffusion_apply(I["c_apply"], _dev(I["phi"])))
        elif job in ("solve", "solve2"):
            x = _dev(I["x0"])
            info[job] = Sc.diffusion_solve(I["c_solve"], _dev(I["b"]), x, RTOL, MAXIT if job == "solve" else 2)
            out[job] = _host(x)
        else:
            p = _dev(I["phi0"])
            info[job] = Sc.step_imex(p, I["dt"], S, float(job[4:]), RTOL, MAXIT, _dev(I["q"]))
            out[job] = _host(p)
        out[job] = out[job].reshape(shape)
    Sc.close()
    Pz.close()
    return out, info


@functools.lru_cache(maxsize=None)
def one_rank(n, bcname, uniform):
    kinds, vals = sc.BC_SETS[bcname]
    return one_rank_jobs(irk.inputs(n, bcname, uniform), n, uniform, kinds, vals)


# ------------------------------------------------------------------------------------------------------------------ the collective calls on a rank grid

def _worker(R, case, blocks, I, jobs=JOBS, poison_then_again=False):
    """-> {job: this rank's block}, {job: info}, {job: (exchanges, messages, bytes, allreduces) of the call}.  Through fluca_amd.scalar.Scalar, whose methods take the
    collective entry points on such a handle.  Every array lives in ONE arena, 8 bytes off a 16-byte boundary, guards around it."""
    import torch
    from fluca_amd import capi
    from fluca_amd.scalar import Scalar
    from tests.caller_arrays import Arena
    from tests.test_gpu_config5 import _handle
    P, d, s = _handle(R, case)
    r = R.rank
    out, info, wire = {}, {}, {}
    with torch.cuda.stream(s):
        Sc = Scalar(P, case.kinds, case.vals, gamma=I["gamma"])
        assert Sc.several
        N = P.ncell
        Vd = [torch.as_tensor(np.ascontiguousarray(blocks["V"][a][r], dtype=np.float64).ravel(), device="cuda") for a in range(3)]
        Sc.set_velocity(*Vd)
        T = Arena([("phi", N, "in"), ("out", N, "out"), ("b", N, "in"), ("x", N, "inout"), ("x2", N, "inout"), ("q", N, "in"), ("p1", N, "inout"), ("p2", N, "inout")], "B")
        assert T.phase("x") == 8
        for name, src in (("phi", "phi"), ("b", "b"), ("x", "x0"), ("x2", "x0"), ("q", "q"), ("p1", "phi0"), ("p2", "phi0")):
            T.fill(name, blocks[src][r])
        T.freeze()

        def call(job, f):
            s.synchronize()
            w0 = R.stats()
            res = f()
            s.synchronize()
            w1 = R.stats()
            wire[job] = tuple(w1[k] - w0[k] for k in ("exchanges", "messages", "bytes", "allreduces"))
            return res

        written = []
        for job in jobs:
            if job == "apply":
                call(job, lambda: Sc.diffusion_apply(I["c_apply"], T["phi"], out=T["out"]))
                where = "out"
            elif job in ("solve", "solve2"):
                where = "x" if job == "solve" else "x2"
                info[job] = call(job, lambda: Sc.diffusion_solve(I["c_solve"], T["b"], T[where], RTOL, MAXIT if job == "solve" else 2))
                if poison_then_again:                       # nothing stale is read: both slabs become NaN, the guess goes back, the same solve again
                    first = T.get(where)
                    assert capi.lib.fldbg_scalar_poison_slabs(Sc.h) == 0
                    T[where].copy_(torch.from_numpy(np.ascontiguousarray(blocks["x0"][r]).ravel()))
                    call(job, lambda: Sc.diffusion_solve(I["c_solve"], T["b"], T[where], RTOL, MAXIT if job == "solve" else 2))
                    assert same(first, T.get(where)) and np.isfinite(first).all(), (r, job, "a solve after poisoned slabs differs")
            else:
                where = "p1" if job == "imex1.0" else "p2"
                info[job] = call(job, lambda: Sc.step_imex(T[where], I["dt"], S, float(job[4:]), RTOL, MAXIT, T["q"]))
            written.append(where)
            T.check(written=written)                        # guards, inputs and the arrays not yet written: untouched
            out[job] = T.get(where)
        Sc.close()
    P.close()
    return out, info, wire


def run_case(case, I, jobs=JOBS, poison_then_again=False):
    res = inproc.run_threads(case.size, _worker, case, irk.scatter(case, I), I, jobs, poison_then_again)
    got = {job: rk.gather_cells(case, [res[r][0][job] for r in range(case.size)]) for job in jobs}
    return got, [res[r][1] for r in range(case.size)], [res[r][2] for r in range(case.size)]


def expected_wire(case, r, job, info):
    if job == "apply":
        return irk.wire_apply(case, r)
    if job in ("solve", "solve2"):
        return irk.wire_solve(case, r, info[job]["steps"])
    return irk.wire_imex(case, r, S, info[job]["steps"], float(job[4:]))


@pytest.mark.parametrize("case", CASES, ids=rk.case_id)
def test_bits_info_wire_and_guards_across_rank_grids(case):
    """apply; solve to 1e-6 at S = 20; solve with maxit = 2; step_imex with theta = 1 and 1 / 2 at a Courant number of 0.4 and a diffusive number of 20 (ten times
    the explicit limit of the three-stage step): gathered = one rank bit for bit, info the one-rank info on every rank, the wire the geometry's count"""
    if case.n == (65, 64, 80):
        from tests.test_scalar_implicit_ranks_host import cheb_plan
        from fluca_amd import capi
        pl = cheb_plan(capi, tuple(case.lo_len(1)[1]))
        assert (pl["fixed_seg"], pl["per_xcd"]) == (1, 160)        # (k_scalar_cheb's cap is 256: the case after this one is the block at the cap)
    if case.n == (65, 64, 130):
        from tests.test_scalar_implicit_ranks_host import cheb_plan
        from fluca_amd import capi
        pl, big = cheb_plan(capi, tuple(case.lo_len(1)[1])), cheb_plan(capi, (512, 512, 512))
        assert (pl["fixed_seg"], pl["per_xcd"]) == (big["fixed_seg"], big["per_xcd"]) == (1, 256) and pl["items"] > 4 * 8 * pl["per_xcd"]
    I = irk.inputs(*irk.case_key(case))
    want, winfo = one_rank(*irk.case_key(case))
    got, infos, wires = run_case(case, I)
    assert winfo["solve"]["steps"] > 2 and not winfo["solve"]["capped"] and winfo["solve2"]["steps"] == 2 and winfo["solve2"]["capped"]
    assert winfo["imex1.0"]["steps"] > 0 and winfo["imex0.5"]["steps"] > 0
    for job in JOBS:
        a, b = bits(got[job]), bits(want[job])
        assert np.isfinite(got[job]).all(), job
        assert np.array_equal(a, b), (rk.case_id(case), job, f"{int((a != b).sum())} of {a.size} cells differ from the one-rank result, the first at {int(np.flatnonzero(a != b)[0])}",
                                      float(np.abs(got[job] - want[job]).max()))
    for r in range(case.size):
        assert infos[r] == winfo, (r, infos[r], winfo)
        for job in JOBS:
            assert wires[r][job][3] == 0, (r, job, "an all-reduce")
            assert wires[r][job][:3] == expected_wire(case, r, job, winfo), (rk.case_id(case), r, job, wires[r][job], expected_wire(case, r, job, winfo))


def test_two_steps_against_the_long_double_recurrence():
    """independent of the one-rank kernel: on config 5's rank grid (channel: its periodic z split) x_2 of a solve with maxit = 2 against the long-double
    recurrence of tests/scalar_implicit_reference.py, cell by cell, within the derived two-step bound of tests/test_gpu_scalar_implicit.py"""
    from tests import scalar_implicit_reference as ir
    from tests.test_gpu_scalar_implicit import two_step_bound
    n, ranks, bcname, uniform = irk.CHANNEL_222
    case = rk.Case(n, ranks, bcname, uniform=uniform)
    I = irk.inputs(n, bcname, uniform)
    P = ir.grid_problem(n, uniform, bcname)
    got, infos, _ = run_case(case, I, jobs=("solve2",))
    assert all(i["solve2"]["steps"] == 2 and i["solve2"]["capped"] for i in infos)
    want, E = two_step_bound(P, I["c_solve"], I["b"], I["x0"])
    err = np.abs(got["solve2"].astype(np.longdouble) - want).astype(np.float64)
    tol = sc.rhs_slack(E)
    print(f"two steps on 2 x 2 x 2: largest error / bound = {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), float((err / tol).max())


def test_nothing_stale_is_read_from_the_slabs():
    """after a solve both slabs are filled with NaN and the solve runs again from the same guess: the same bits (every layer read was received or packed by
    the call itself); on 2 x 2 x 2 and on the two-cell blocks with the same peer on both sides"""
    for case in (rk.Case(*irk.CHANNEL_222[:3], uniform=False), rk.Case((4, 4, 4), (1, 1, 2), "periodic")):
        I = irk.inputs(*irk.case_key(case))
        got, _, _ = run_case(case, I, jobs=("solve", "imex1.0", "solve2"), poison_then_again=True)
        want, _ = one_rank(*irk.case_key(case))
        for job in ("solve", "imex1.0", "solve2"):
            assert same(got[job], want[job]), (rk.case_id(case), job)


def test_boundary_values_are_not_applied_at_a_rank_face():
    """channel (Dirichlet x-, Neumann x+ and y) with boundary values of 1e6 on a 2 x 1 x 1 split: the one-rank bits -- a rank face taken for a boundary would
    move the cells beside it by orders of magnitude"""
    case = rk.Case((7, 5, 6), (2, 1, 1), "channel", uniform=False, own=[(5, 2), (5,), (6,)])
    case.vals = (1e6, -1e6, 1e6, -1e6, 0.0, 0.0)
    I = irk.inputs(*irk.case_key(case))
    want, winfo = one_rank_jobs(I, case.n, case.uniform, case.kinds, case.vals)
    assert not same(want["apply"], one_rank(*irk.case_key(case))[0]["apply"])        # (the values matter)
    got, infos, _ = run_case(case, I)
    for job in JOBS:
        assert same(got[job], want[job]), job
    assert infos[0] == infos[1] == winfo


# ------------------------------------------------------------------------------------------------------------------ Gamma = 0, c = 0, history

def _plain_worker(R, case, blocks, I, script):
    """script(Sc, dev, blk, R, s) on this rank's handles -> what it returns"""
    import torch
    from fluca_amd.scalar import Scalar
    from tests.test_gpu_config5 import _handle
    P, d, s = _handle(R, case)
    with torch.cuda.stream(s):
        Sc = Scalar(P, case.kinds, case.vals, gamma=I["gamma"])
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        Sc.set_velocity(*[dev(blocks["V"][a][R.rank]) for a in range(3)])
        blk = {k: blocks[k][R.rank] for k in ("phi", "b", "x0", "q", "phi0")}

        def wired(f):
            s.synchronize()
            w0 = R.stats()
            res = f()
            s.synchronize()
            w1 = R.stats()
            return res, tuple(w1[k] - w0[k] for k in ("exchanges", "messages", "bytes", "allreduces"))
        res = script(Sc, dev, blk, R, wired)
        s.synchronize()
        Sc.close()
    P.close()
    return res


def run_plain(case, I, script):
    return inproc.run_threads(case.size, _plain_worker, case, irk.scatter(case, I), I, script)


def test_without_diffusivity_the_step_is_fl_scalar_step_and_c_zero_copies_b():
    case = rk.Case(*irk.CHANNEL_222[:3], uniform=False)
    I = irk.inputs(*irk.case_key(case))

    def script(Sc, dev, blk, R, wired):
        Sc.set_diffusivity(0.0)
        a, wa = wired(lambda: Sc.step(dev(blk["phi0"]), I["dt"], S, dev(blk["q"])))
        p = dev(blk["phi0"])
        info, wb = wired(lambda: Sc.step_imex(p, I["dt"], S, 1.0, RTOL, MAXIT, dev(blk["q"])))
        x = dev(blk["x0"])
        info0, wc = wired(lambda: Sc.diffusion_solve(0.0, dev(blk["b"]), x, RTOL, MAXIT))
        return a.cpu().numpy(), p.cpu().numpy(), x.cpu().numpy(), info, info0, wa, wb, wc
    for r, (a, p, x, info, info0, wa, wb, wc) in enumerate(run_plain(case, I, script)):
        assert same(a, p) and info["steps"] == 0, r
        assert wa == wb == irk.wire_explicit_step(case, r, S) + (0,), (r, wa, wb)
        assert same(x, rk.scatter_cells(case, I["b"])[r]) and info0["steps"] == 0 and not info0["capped"], r
        assert (info0["emin"], info0["emax"], info0["bound"]) == (1.0, 1.0, 1.0) and wc == (0, 0, 0, 0), (r, info0, wc)


def test_history_changes_no_bit():
    """step_imex after rhs, step, cfl, boundary_flux and an earlier solve = the same call on fresh handles (the one-rank bits of the main test); fl_scalar_step after
    an implicit step keeps the bits and the wire it has on fresh handles"""
    case = rk.Case(*irk.CHANNEL_222[:3], uniform=False)
    I = irk.inputs(*irk.case_key(case))
    want, _ = one_rank(*irk.case_key(case))

    def fresh_step(Sc, dev, blk, R, wired):
        a, w = wired(lambda: Sc.step(dev(blk["phi0"]), I["dt"], 5, dev(blk["q"])))
        return a.cpu().numpy(), w

    def script(Sc, dev, blk, R, wired):
        Sc.rhs(dev(blk["phi"]), dev(blk["q"]))
        Sc.step(dev(blk["phi0"]), I["dt"], 5, dev(blk["q"]))
        Sc.cfl(I["dt"])
        Sc.boundary_flux(dev(blk["phi"]))
        Sc.diffusion_solve(I["c_solve"] * 3.0, dev(blk["phi"]), dev(blk["phi0"]), 1e-8, 1000)
        out = []
        for theta in irk.THETAS:
            p = dev(blk["phi0"])
            Sc.step_imex(p, I["dt"], S, theta, RTOL, MAXIT, dev(blk["q"]))
            out.append(p.cpu().numpy())
        a, w = wired(lambda: Sc.step(dev(blk["phi0"]), I["dt"], 5, dev(blk["q"])))
        return out, a.cpu().numpy(), w
    first = run_plain(case, I, fresh_step)
    res = run_plain(case, I, script)
    for t, theta in enumerate(irk.THETAS):
        assert same(rk.gather_cells(case, [res[r][0][t] for r in range(case.size)]), want[f"imex{theta}"]), theta
    for r in range(case.size):
        assert same(res[r][1], first[r][0]) and res[r][2] == first[r][1] == irk.wire_explicit_step(case, r, 5) + (0,), r


# ------------------------------------------------------------------------------------------------------------------ a busy stream

def _delay_worker(R, case, blocks, I, theta):
    import torch
    from fluca_amd.scalar import Scalar
    from tests.test_gpu_config5 import _handle
    from tests.test_gpu_stream_order import both
    P, d, s = _handle(R, case)
    with torch.cuda.stream(s):
        Sc = Scalar(P, case.kinds, case.vals, gamma=I["gamma"])
        r = R.rank
        flat = lambda a: np.ascontiguousarray(a, dtype=np.float64).ravel()
        inputs = {"b": flat(blocks["b"][r]), "x": flat(blocks["x0"][r]), "phi": flat(blocks["phi0"][r]), "q": flat(blocks["q"][r]), **{f"V{a}": flat(blocks["V"][a][r]) for a in range(3)}}
        x0 = torch.as_tensor(inputs["x"], device="cuda")
        Sc.diffusion_solve(I["c_solve"], torch.as_tensor(inputs["b"], device="cuda"), x0, RTOL, MAXIT)          # the first implicit call allocates
        s.synchronize()

        def seq(Q):
            Sc.set_velocity(Q["V0"], Q["V1"], Q["V2"])
            Q.do(Sc.diffusion_solve, I["c_solve"], Q["b"], Q["x"], RTOL, MAXIT); Q.snap("x", "x")
            Q.release("b")
            Q.do(Sc.step_imex, Q["phi"], I["dt"], S, theta, RTOL, MAXIT, Q["q"]); Q.snap("phi", "phi")
            Q.release("q", "V0", "V1", "V2", "x", "phi")
        # (the host-staged transport of this process waits for the planes of every exchange: the delay cannot stay pending, the bits must not move)
        idle = both(f"2 x 1 x 1 rank {r} solve + step_imex theta={theta}", P, seq, inputs, {}, must_assert=False)
        Sc.close()
    P.close()
    return {k: v[0] for k, v in idle.items()}


@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_solve_and_step_imex_behind_a_delay_on_both_ranks(theta):
    """one solve and one IMEX step on 2 x 1 x 1 queued behind a delay on BOTH ranks' streams, the inputs produced behind the delay and poisoned right after the
    calls (the two plays of tests/test_gpu_stream_order.py): each rank's queued bits are its idle bits, and the gathered idle bits the one-rank ones"""
    case = SMALL
    I = irk.inputs(*irk.case_key(case))
    res = inproc.run_threads(case.size, _delay_worker, case, irk.scatter(case, I), I, theta)
    want, _ = one_rank(*irk.case_key(case))
    assert same(rk.gather_cells(case, [res[r]["x"] for r in range(case.size)]), want["solve"])
    assert same(rk.gather_cells(case, [res[r]["phi"] for r in range(case.size)]), want[f"imex{theta}"])


# ------------------------------------------------------------------------------------------------------------------ errors

def _errors_worker(R, case):
    import torch
    from fluca_amd import capi
    from fluca_amd.scalar import Scalar
    from tests.test_gpu_config5 import _handle
    lib = capi.lib
    P, d, s = _handle(R, case)
    got = []
    with torch.cuda.stream(s):
        Sc = Scalar(P, case.kinds, case.vals, gamma=0.1)
        keep = np.random.default_rng(R.rank).uniform(-1, 1, P.ncell)
        x, b = torch.as_tensor(keep, device="cuda"), torch.zeros(P.ncell, dtype=torch.float64, device="cuda")
        px, pb = C.c_void_p(x.data_ptr()), C.c_void_p(b.data_ptr())
        info = capi.fl_scalar_cheb_info(steps=-7)
        nan, inf = float("nan"), float("inf")
        w0 = R.stats()
        for c in (-1.0, nan, inf):
            got.append(("c", lib.fl_scalar_diffusion_apply_ranks(Sc.h, c, pb, px), lib.fl_scalar_diffusion_solve_ranks(Sc.h, c, 1e-6, 10, pb, px, C.byref(info))))
        got.append(("null", lib.fl_scalar_diffusion_apply_ranks(Sc.h, 1.0, None, px), lib.fl_scalar_diffusion_apply_ranks(Sc.h, 1.0, px, None),
                    lib.fl_scalar_diffusion_solve_ranks(Sc.h, 1.0, 1e-6, 10, None, px, None), lib.fl_scalar_diffusion_solve_ranks(Sc.h, 1.0, 1e-6, 10, pb, None, None),
                    lib.fl_scalar_step_imex_ranks(Sc.h, 0.1, 3, 1.0, 1e-6, 10, None, None, C.byref(info))))
        got.append(("alias", lib.fl_scalar_diffusion_apply_ranks(Sc.h, 1.0, px, px), lib.fl_scalar_diffusion_solve_ranks(Sc.h, 1.0, 1e-6, 10, px, px, C.byref(info))))
        for rtol in (0.0, 1.0, -0.5, nan, inf):
            got.append(("rtol", lib.fl_scalar_diffusion_solve_ranks(Sc.h, 1.0, rtol, 10, pb, px, C.byref(info)), lib.fl_scalar_step_imex_ranks(Sc.h, 0.1, 3, 1.0, rtol, 10, None, px, C.byref(info))))
        got.append(("maxit", lib.fl_scalar_diffusion_solve_ranks(Sc.h, 1.0, 1e-6, -1, pb, px, C.byref(info)), lib.fl_scalar_step_imex_ranks(Sc.h, 0.1, 3, 1.0, 1e-6, -2, None, px, C.byref(info))))
        for theta in (0.49, 1.01, 0.0, nan):
            got.append(("theta", lib.fl_scalar_step_imex_ranks(Sc.h, 0.1, 3, theta, 1e-6, 10, None, px, C.byref(info))))
        for dt in (nan, inf, -0.1):
            got.append(("dt", lib.fl_scalar_step_imex_ranks(Sc.h, dt, 3, 1.0, 1e-6, 10, None, px, C.byref(info))))
        got.append(("stages", lib.fl_scalar_step_imex_ranks(Sc.h, 0.1, 1, 1.0, 1e-6, 10, None, px, C.byref(info))))
        got.append(("state", lib.fl_scalar_step_imex_ranks(Sc.h, 0.1, 3, 1.0, 1e-6, 10, None, px, C.byref(info))))          # no velocity yet
        s.synchronize()
        w1 = R.stats()
        untouched = same(x.cpu().numpy(), keep) and info.steps == -7 and w1 == w0
        Sc.close()
    P.close()
    return got, untouched


def test_errors_come_from_every_rank_and_leave_the_outputs_alone():
    """the argument errors of the one-rank calls, on both ranks alike, before anything is sent"""
    want = ([("c", -63, -63)] * 3 + [("null", -85, -85, -85, -85, -85), ("alias", -62, -62)] + [("rtol", -63, -63)] * 5 + [("maxit", -63, -63)] + [("theta", -63)] * 4 +
            [("dt", -63)] * 3 + [("stages", -63), ("state", -73)])
    for r, (got, untouched) in enumerate(inproc.run_threads(SMALL.size, _errors_worker, SMALL)):
        assert got == want, (r, [g for g, w in zip(got, want) if g != w])
        assert untouched, (r, "an argument error wrote an output, filled info or sent a message")


def test_on_a_one_rank_handle_the_collective_names_are_the_plain_calls():
    n, bcname, uniform = (7, 6, 5), "channel", False
    want, winfo = one_rank(n, bcname, uniform)
    kinds, vals = sc.BC_SETS[bcname]
    got, info = one_rank_jobs(irk.inputs(n, bcname, uniform), n, uniform, kinds, vals, entry="_ranks")
    for job in JOBS:
        assert same(got[job], want[job]), job
    assert info == winfo
