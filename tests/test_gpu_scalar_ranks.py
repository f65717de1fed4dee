"""-m gpu: fl_scalar_rhs, fl_scalar_cfl, fl_scalar_stats and fl_scalar_create_ranks on rank grids, the ranks as threads of one process
(tests/inproc.py), against tests/scalar_reference.py on the GLOBAL grid.

The bound on every gathered cell is the derived bound of tests/test_gpu_scalar.py (scalar_cases.rhs_slack of the reference's operation count),
nothing fitted.  The cases are the smallest at which a slab index, a predicate or a table offset can be wrong: 2-cell blocks whose +-2 images are
the peer's cells (both slabs from one peer), a middle rank with no physical boundary, uneven ownership, 2 x 2 x 2 with a periodic axis split over
two ranks, one axis split while another wraps inside the block, the 64-lane segment edge in x with slabs across x, y and z, and blocks that take
the launch plan of 512^3.  All reference work is done before the rank threads start or after they end."""
import ctypes as C

import numpy as np
import pytest

from tests import inproc
from tests import scalar_cases as sc
from tests import scalar_ranks as rk
from tests import scalar_reference as sr

pytestmark = pytest.mark.gpu

GAMMA = 0.0125
GUARD = 64
SENTINEL = -7.25e300
FULL = tuple((g, s, k) for g, s in ((0.0, False), (GAMMA, True)) for k in sc.PHI_KINDS)     # the variants of test_gpu_scalar.check_rhs


def _jobs(limiters, variants=FULL):
    return [(lim, g, s, k) for lim in limiters for g, s, k in variants]


def _inputs(case, jobs):
    """the blocks of every field the jobs use, per rank"""
    n = case.n
    V = sc.velocity(n, case.bcname)
    return {"V": [rk.scatter_faces(case, V[a], a) for a in range(3)], "q": rk.scatter_cells(case, sc.source(n)),
            "phi": {k: rk.scatter_cells(case, sc.phi_field(n, k)) for k in {j[3] for j in jobs}}}


def _rhs_worker(R, case, jobs, blocks, check_wire):
    import torch
    from fluca_amd.scalar import Scalar
    from tests.test_gpu_config5 import _handle
    P, d, s = _handle(R, case)
    outs = []
    with torch.cuda.stream(s):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        S = Scalar(P, case.kinds, case.vals)
        Vd = [dev(blocks["V"][a][R.rank]) for a in range(3)]
        assert tuple(P.nface) == tuple(int(v.numel()) for v in Vd)
        S.set_velocity(*Vd)
        qd = dev(blocks["q"][R.rank])
        for limiter, gamma, with_source, kind in jobs:
            S.set_limiter(limiter)
            S.set_diffusivity(gamma)
            phi = dev(blocks["phi"][kind][R.rank])
            buf = torch.full((P.ncell + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
            s.synchronize()
            w0 = R.stats()
            S.rhs(phi, qd if with_source else None, out=buf[GUARD:GUARD + P.ncell])
            s.synchronize()
            w1 = R.stats()
            got = buf.cpu().numpy()
            assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + P.ncell:] == SENTINEL).all(), ("guard cells written", R.rank)
            if check_wire:
                assert (w1["messages"] - w0["messages"], w1["bytes"] - w0["bytes"]) == rk.wire_rhs(case, R.rank), (R.rank, w0, w1, rk.wire_rhs(case, R.rank))
                assert w1["exchanges"] - w0["exchanges"] <= 2 and w1["allreduces"] == w0["allreduces"]
            outs.append(got[GUARD:GUARD + P.ncell].copy())
        S.close()
    P.close()
    return outs


def run_rhs(case, jobs, check_wire=True):
    """-> the gathered R of every job"""
    blocks = _inputs(case, jobs)
    res = inproc.run_threads(case.size, _rhs_worker, case, jobs, blocks, check_wire)
    return [rk.gather_cells(case, [res[r][a] for r in range(case.size)]) for a in range(len(jobs))]


def check_against_reference(case, jobs, got):
    Pr = case.problem()
    V = sc.velocity(case.n, case.bcname)
    worst = 0.0
    keep = Pr.gamma                                          # (the problem is shared between the tests of a session)
    for (limiter, gamma, with_source, kind), g in zip(jobs, got):
        Pr.gamma = gamma
        phi = sc.phi_field(case.n, kind)
        want, E, _ = sr.rhs(Pr, phi, V, sc.source(case.n) if with_source else None, np.longdouble, bounds=True, limiter=limiter)
        err = np.abs(g.astype(np.longdouble) - want).astype(np.float64)
        tol = sc.rhs_slack(E)
        worst = max(worst, float((err / tol).max()))
        bad = np.argwhere(err > tol)
        assert bad.size == 0, (f"{rk.case_id(case)} {limiter} gamma={gamma} phi={kind}: {len(bad)} cells beyond the derived bound, first (k, j, i) = {tuple(bad[0])}: "
                               f"got {g[tuple(bad[0])]!r}, exact {float(want[tuple(bad[0])])!r}, error {err[tuple(bad[0])]:.3e} > bound {tol[tuple(bad[0])]:.3e}")
    Pr.gamma = keep
    print(f"rhs {rk.case_id(case)}: largest error / bound = {worst:.3f}")


def check_case(case, limiters, variants=FULL):
    jobs = _jobs(limiters, variants)
    check_against_reference(case, jobs, run_rhs(case, jobs))


THREE = ("superbee", "vanleer", "quick")


@pytest.mark.parametrize("ranks", [(2, 1, 1), (1, 2, 1), (1, 1, 2)], ids=lambda r: "x".join(map(str, r)))
def test_two_cell_blocks_same_peer_on_both_sides(ranks):
    check_case(rk.Case((4, 4, 4), ranks, "periodic"), THREE)


@pytest.mark.parametrize("bcname", ["dirichlet", "periodic"])
@pytest.mark.parametrize("n,ranks", [((6, 5, 4), (3, 1, 1)), ((4, 5, 6), (1, 1, 3))], ids=["x3", "z3"])
def test_middle_rank_without_a_physical_boundary(n, ranks, bcname):
    check_case(rk.Case(n, ranks, bcname, uniform=False), THREE)


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "stretched"])
@pytest.mark.parametrize("bcname", list(sc.BC_SETS))
def test_uneven_ownership_every_limiter(bcname, uniform):
    """the rank with the 2-cell block has a physical boundary at its high end and a neighbour at its low end"""
    check_case(rk.Case((7, 5, 6), (2, 1, 1), bcname, uniform=uniform, own=[(5, 2), (5,), (6,)]), sr.LIMITERS)


@pytest.mark.parametrize("bcname", list(sc.BC_SETS))
def test_two_by_two_by_two(bcname):
    """channel splits its periodic z over two ranks"""
    check_case(rk.Case((7, 6, 5), (2, 2, 2), bcname, uniform=False), THREE)


def test_one_axis_split_another_wrapped():
    check_case(rk.Case((7, 5, 6), (1, 2, 1), "channel", uniform=False), THREE)


@pytest.mark.parametrize("ranks", [(2, 1, 1), (1, 2, 1), (1, 1, 2)], ids=lambda r: "x".join(map(str, r)))
def test_segment_edge_in_x(ranks):
    """blocks of 65 with a ragged second segment and x slabs; y and z slabs read along a ragged x line"""
    check_case(rk.Case((130, 6, 7), ranks, "channel", uniform=False), THREE)


@pytest.mark.parametrize("bcname,limiter", [("channel", "superbee"), ("periodic", "vanleer"), ("dirichlet", "quick")])
def test_rhs_in_the_plan_of_512_cubed(bcname, limiter):
    """each block is scalar_cases.REGIME_GRID: the blocks per XCD at their cap, fixed segments, waves with a second trip"""
    from fluca_amd import capi
    case = rk.Case((65, 64, 80), (1, 1, 2), bcname, uniform=False)
    assert tuple(case.lo_len(1)[1]) == sc.REGIME_GRID
    out = (C.c_int * 5)()
    f = capi.lib.fldbg_scalar_plan
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    assert f(512, 512, 512, sr.LIMITERS.index(limiter), out, 5) == 5
    big = list(out)
    assert f(*sc.REGIME_GRID, sr.LIMITERS.index(limiter), out, 5) == 5
    assert (out[0], out[3]) == (big[0], big[3]) == (128, 1) and out[4] > 4 * 8 * out[0]
    check_case(case, (limiter,), tuple((GAMMA, True, k) for k in ("random", "step")))


# ------------------------------------------------------------------------------------------------ bits

BITS_N, BITS_BC = (7, 6, 5), "channel"
BITS_JOBS = [("superbee", GAMMA, True, "random"), ("vanleer", 0.0, False, "step"), ("quick", GAMMA, True, "alternating"), ("venkatakrishnan", GAMMA, False, "plateau")]


def _one_rank_rhs(jobs):
    from tests.gpu_common import dev, host
    n = BITS_N
    Pz, S = sc.make_handles(n, False, BITS_BC)
    S.set_velocity(*[dev(v.reshape(-1)) for v in sc.velocity(n, BITS_BC)])
    out = []
    for limiter, gamma, with_source, kind in jobs:
        S.set_limiter(limiter)
        S.set_diffusivity(gamma)
        out.append(host(S.rhs(dev(sc.phi_field(n, kind).reshape(-1)), dev(sc.source(n).reshape(-1)) if with_source else None)).reshape(n[2], n[1], n[0]).copy())
    S.close()
    Pz.close()
    return out


def test_rank_grid_independence_bit_for_bit():
    """the same kernel instance on the same values per cell: the gathered R is bitwise the same on five rank grids -- and bitwise the one-rank
    fl_scalar_rhs, whose kernel shares the arithmetic's source"""
    got = {ranks: run_rhs(rk.Case(BITS_N, ranks, BITS_BC, uniform=False), BITS_JOBS) for ranks in [(2, 1, 1), (1, 2, 1), (1, 1, 2), (2, 2, 1), (2, 2, 2)]}
    first = got[(2, 1, 1)]
    for ranks, g in got.items():
        for a, b, job in zip(first, g, BITS_JOBS):
            assert np.array_equal(a, b), (ranks, job, int((a != b).sum()))
    one = _one_rank_rhs(BITS_JOBS)
    for a, b, job in zip(first, one, BITS_JOBS):
        assert np.array_equal(a, b), ("one rank", job, int((a != b).sum()), float(np.abs(a - b).max()))


# ------------------------------------------------------------------------------------------------ stats, cfl

def _stats_worker(R, case, blocks, dt):
    import torch
    from fluca_amd.scalar import Scalar
    from tests.test_gpu_config5 import _handle
    P, d, s = _handle(R, case)
    with torch.cuda.stream(s):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        S = Scalar(P, case.kinds, case.vals, gamma=GAMMA)
        S.set_velocity(*[dev(blocks["V"][a][R.rank]) for a in range(3)])
        out = {"cfl": S.cfl(dt), "cfl2": S.cfl(dt)}
        for kind in blocks["phi"]:
            phi = dev(blocks["phi"][kind][R.rank])
            out[kind] = S.stats(phi)
            assert S.stats(phi) == out[kind]                 # the same bits on every call
        S.close()
    P.close()
    return out


@pytest.mark.parametrize("n,ranks,bcname,uniform", [((7, 6, 5), (2, 2, 2), "channel", False), ((66, 9, 5), (2, 1, 1), "periodic", True), ((40, 33, 37), (2, 2, 1), "periodic", False)],
                         ids=["7x6x5-2x2x2-channel", "66x9x5-2x1x1-periodic", "40x33x37-2x2x1-periodic"])
def test_cfl_and_stats(n, ranks, bcname, uniform):
    """min and max exactly and identical on every rank; the sum within the depth-derived bound of test_gpu_scalar.test_cfl_and_stats -- the depth
    of the deepest rank's own sum, plus one rounding per rank for the all-reduce; the Courant numbers within that test's 6- and 9-operation bounds
    of the reference on the global grid"""
    case = rk.Case(n, ranks, bcname, uniform=uniform)
    Pr = case.problem()
    V = sc.velocity(n, bcname)
    dt = 0.0123
    jobs = [(None, 0, 0, "random"), (None, 0, 0, "step")]
    keep = Pr.gamma
    Pr.gamma = GAMMA
    want_cfl = sr.cfl(Pr, V, dt, np.longdouble)
    want = {k: sr.stats(Pr, sc.phi_field(n, k), np.longdouble) for k in ("random", "step")}
    Pr.gamma = keep
    res = inproc.run_threads(case.size, _stats_worker, case, _inputs(case, jobs), dt)
    depth = 0
    for r in range(case.size):
        ncell = int(np.prod(case.lo_len(r)[1]))
        nb = min(1024, -(-ncell // 256))
        depth = max(depth, -(-ncell // (256 * nb)) + 6 + 2 + nb + 3)
    depth += case.size
    for r in range(case.size):
        assert res[r] == res[0], r                                # identical on every rank, bit for bit
    assert res[0]["cfl"] == res[0]["cfl2"]
    for g, w, ops in zip(res[0]["cfl"], want_cfl, (6, 9)):
        assert abs(g - w) <= ops * sr.U * abs(w) * (1 + 2.0 ** -10), (g, w)
    for kind in ("random", "step"):
        mn, mx, sm = res[0][kind]
        wmn, wmx, wsm = want[kind]
        assert (mn, mx) == (wmn, wmx)
        mag = float((np.abs(sc.phi_field(n, kind)) * sr.volumes(Pr)).sum())
        assert abs(sm - wsm) <= depth * sr.U * mag * (1 + 2.0 ** -10), (sm, float(wsm), depth * sr.U * mag)


# ------------------------------------------------------------------------------------------------ errors

def _six(*v):
    return (C.c_int * 6)(*v)


def _errors_worker(R, case):
    import torch
    from fluca_amd import capi
    from tests.test_gpu_config5 import _handle
    lib = capi.lib
    P, d, s = _handle(R, case)
    h = C.c_void_p()
    out = {}
    with torch.cuda.stream(s):
        good = list(case.kinds)
        flipped = [0 if good[0] == 2 else 2] * 2 + good[2:]                 # x's periodic flags against the grid's
        out["flags"] = lib.fl_scalar_create_ranks(P.h, _six(*flipped), C.byref(h)), bool(h.value)
        out["kind"] = lib.fl_scalar_create_ranks(P.h, _six(*(good[:5] + [3])), C.byref(h)), bool(h.value)
        out["one_rank_entry"] = lib.fl_scalar_create(P.h, _six(*good), C.byref(h)), bool(h.value)
        rc = lib.fl_scalar_create_ranks(P.h, _six(*good), C.byref(h))
        out["create"] = rc, bool(h.value)
        if h.value:
            assert lib.fl_scalar_destroy(h) == 0
    P.close()
    return out


def test_errors():
    from fluca_amd import capi
    from fluca_amd.poisson import Poisson, default_decomp
    from oracle import fluca_oracle as fo
    from tests.gpu_common import dev, host
    lib = capi.lib
    # on a one-rank handle the entry point is fl_scalar_create, bit for bit
    n = (7, 5, 6)
    Pz, S = sc.make_handles(n, False, "channel", gamma=GAMMA)
    h = C.c_void_p()
    kinds, vals = sc.BC_SETS["channel"]
    assert lib.fl_scalar_create_ranks(Pz.h, _six(*kinds), C.byref(h)) == 0 and h.value
    assert lib.fl_scalar_create_ranks(Pz.h, _six(0, 0, 0, 0, 0, 0), C.byref(C.c_void_p())) == -62
    Vd = [dev(v.reshape(-1)) for v in sc.velocity(n, "channel")]
    S.set_velocity(*Vd)
    phi = dev(sc.phi_field(n, "random").reshape(-1))
    a = host(S.rhs(phi)).copy()
    for b, v in enumerate(vals):
        assert lib.fl_scalar_set_boundary_value(h, b, v) == 0
    assert lib.fl_scalar_set_diffusivity(h, GAMMA) == 0
    assert lib.fl_scalar_set_velocity(h, *[C.c_void_p(v.data_ptr()) for v in Vd]) == 0
    out = Pz.empty()
    Pz._pre()
    assert lib.fl_scalar_rhs(h, C.c_void_p(phi.data_ptr()), None, C.c_void_p(out.data_ptr())) == 0
    Pz._post()
    assert np.array_equal(host(out), a)
    assert lib.fl_scalar_destroy(h) == 0
    S.close()
    Pz.close()
    # a decomposed handle with no transport attached
    P2 = Poisson((8, 6, 4), sc.faces((8, 6, 4), True), [fo.BC_VELOCITY] * 6, 1e-3, decomp=default_decomp((8, 6, 4), (2, 1, 1), 0))
    assert lib.fl_scalar_create_ranks(P2.h, _six(0, 0, 0, 0, 0, 0), C.byref(h)) == -73 and not h.value
    assert lib.fl_scalar_create_ranks(P2.h, _six(2, 2, 0, 0, 0, 0), C.byref(h)) == -62 and not h.value
    assert lib.fl_scalar_create(P2.h, _six(0, 0, 0, 0, 0, 0), C.byref(h)) == -56 and not h.value
    P2.close()
    # with the transport: the flag checks, fl_scalar_create's refusal, success
    ok = rk.Case((7, 5, 6), (2, 1, 1), "dirichlet", own=[(5, 2), (5,), (6,)])
    for res in inproc.run_threads(2, _errors_worker, ok):
        assert res == {"flags": (-62, False), "kind": (-63, False), "one_rank_entry": (-56, False), "create": (0, True)}, res
    # a 1-cell block along the split axis: the voted error on EVERY rank, and no handle.  (On a periodic axis: a 1-cell block before a wall is
    # refused by fl_poisson_create already, whose one-sided wall rows leave such a block.)
    thin = rk.Case((7, 5, 6), (2, 1, 1), "periodic", own=[(6, 1), (5,), (6,)])
    for res in inproc.run_threads(2, _errors_worker, thin):
        assert res == {"flags": (-62, False), "kind": (-63, False), "one_rank_entry": (-56, False), "create": (-63, False)}, res
