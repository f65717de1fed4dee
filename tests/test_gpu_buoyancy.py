"""-m gpu: fl_momentum_add_buoyancy (k_buoyancy, fluca_amd/csrc/fl_buoyancy.hip) through the C-ABI against tests/buoyancy_reference.py.

Every cell is compared with the term in long double; the tolerance (2 nscalar + 2) U (|momrhs before| + |dt| sum_s |a_s,d| |phi_s - ref_s|) is the
operation count -- nscalar differences, nscalar products or fused steps, the product with dt and the final sum -- not a fit.  The kernel documents
its operation order (include/fluca_hip.h), so the bits are pinned as well: by the restatement of that order with tests/step_rhs.fused, and in the
few cells where the long double behind it rounds twice by the same chain in rational arithmetic.  Sizes: the smallest at which it can go wrong -- 27 cells (less than a wave, odd), 60, 33 x 7 x 5 (odd: the
components start 8 bytes off a 16-byte boundary), and the smallest grid of 80 x 64 planes beyond one round of the kernel's own grid-stride plan."""
import ctypes as C

import numpy as np
import pytest

from tests import buoyancy_reference as br
from tests import scalar_cases as sc
from tests import scalar_ranks as rk
from tests import scalar_reference as sr

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -7.25e300
DT = 0.0375
U = sr.U


def beyond_one_round():
    """80 x 64 x nz with nz the first at which the pairs of cells exceed blocks x threads of the kernel's plan"""
    from fluca_amd import capi
    f = capi.lib.fldbg_buoyancy_plan
    f.argtypes = [C.c_int, C.c_int64, C.POINTER(C.c_int), C.c_int]
    f.restype = C.c_int
    out = (C.c_int * 3)()
    assert f(0, 512 ** 3, out, 3) == 3
    blocks, threads, per_lane = out
    assert blocks >= 64 and threads == 512 and per_lane >= 2 and per_lane % 2 == 0      # one 8-wave block per CU, pairs of cells
    nz = blocks * threads * per_lane // (80 * 64) + 1
    assert f(0, 80 * 64 * nz, out, 3) == 3 and out[0] == blocks         # the plan is at its cap: the loop takes a second trip
    return (80, 64, nz)


def coefficients(name, rng):
    """-> accel (nscalar x 3), refs.  Gravity on one, two and three axes; a scalar whose coefficients are all zero among others; single zeros"""
    if name == "one-scalar-one-axis":
        return [[0.0, 2.5, 0.0]], [0.3]
    if name == "three-scalars-two-axes":
        return [[0.7, 0.0, -1.3], [0.0, 0.0, 0.0], [-0.45, 0.0, 2.0]], [0.25, -1.0, 0.5]
    if name == "eight-scalars-three-axes":
        a = rng.uniform(-2.0, 2.0, (8, 3))
        a[4] = 0.0                      # a passive one in the middle
        a[1, 0] = a[6, 2] = 0.0         # single zeros among non-zero coefficients
        return a.tolist(), rng.uniform(-1.0, 1.0, 8).tolist()
    raise ValueError(name)


COEFS = ["one-scalar-one-axis", "three-scalars-two-axes", "eight-scalars-three-axes"]
SMALL = [(3, 3, 3), (5, 4, 3), (33, 7, 5)]


def fields(n, ns, seed):
    rng = np.random.default_rng(seed)
    N = n[0] * n[1] * n[2]
    phis = [rng.uniform(-1.0, 1.0, N) for _ in range(ns)]
    m = rng.uniform(-1.0, 1.0, 3 * N)
    m[rng.uniform(size=3 * N) < 0.1] = -0.0         # a -0.0 keeps its sign where nothing is added, and where +0.0 is added it does not
    m[rng.uniform(size=3 * N) < 0.05] = 0.0
    return phis, m


@pytest.fixture(scope="module")
def handles():
    from fluca_amd.poisson import Momentum, Poisson
    from oracle import fluca_oracle as fo
    made = {}

    def get(n):
        if n not in made:
            Pz = Poisson(n, sc.faces(n, False), [fo.BC_VELOCITY] * 6, 1e-3)
            made[n] = (Pz, Momentum(Pz))
        return made[n]
    yield get
    for Pz, M in made.values():
        M.close()
        Pz.close()


def run_kernel(M, N, phis, m, accel, refs, dt, shift_m=0, shift_phi=0):
    """momrhs inside a sentinel-filled buffer, shift_*: doubles by which the arrays are moved off their 16-byte alignment.  -> the new momrhs; checks
    the sentinels and that the scalars are unchanged"""
    import torch
    buf = torch.full((GUARD + shift_m + 3 * N + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    lo = GUARD + shift_m
    buf[lo:lo + 3 * N] = torch.as_tensor(m, device="cuda")
    pbufs, views = [], []
    for p in phis:
        pb = torch.full((shift_phi + N,), SENTINEL, dtype=torch.float64, device="cuda")
        pb[shift_phi:] = torch.as_tensor(p, device="cuda")
        pbufs.append(pb)
        views.append(pb[shift_phi:])
    assert buf[lo:].data_ptr() % 16 == 8 * (shift_m % 2) and all(v.data_ptr() % 16 == 8 * (shift_phi % 2) for v in views)
    M.add_buoyancy(buf[lo:lo + 3 * N], views, accel, refs, dt)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:lo] == SENTINEL).all() and (got[lo + 3 * N:] == SENTINEL).all(), "written outside momrhs"
    for pb, p in zip(pbufs, phis):
        assert np.array_equal(pb.cpu().numpy()[shift_phi:].view(np.int64), np.asarray(p).view(np.int64)), "a scalar was written"
    return got[lo:lo + 3 * N].copy()


def check(got, m, phis, accel, refs, dt, what):
    ns, N = len(phis), phis[0].size
    T, Mag = br.term(phis, accel, refs, dt)
    want = np.asarray(m, dtype=np.longdouble).reshape(3, N) + T
    got3, m3 = got.reshape(3, N), np.asarray(m).reshape(3, N)
    tol = (2 * ns + 2) * U * (np.abs(m3) + Mag.astype(np.float64))
    err = np.abs(got3.astype(np.longdouble) - want).astype(np.float64)
    worst = float((err / np.where(tol > 0, tol, 1.0)).max())
    print(f"{what}: largest error / bound = {worst:.3f}")
    fused = br.add_fused(m, phis, accel, refs, dt)
    for d in range(3):
        if all(accel[s][d] == 0.0 for s in range(ns)):
            # neither read nor written: every bit stays, the sign of a -0.0 included
            assert np.array_equal(got3[d].view(np.int64), m3[d].view(np.int64)), (what, d)
            continue
        assert (err[d] <= tol[d]).all(), (what, d, int((err[d] > tol[d]).sum()), worst)
        assert np.mean(got3[d] != m3[d]) > 0.9, (what, d)                      # (and the component did change)
        # the bits: the long-double restatement of the fused chain, and where that differs (its rare double roundings) the chain in rational arithmetic
        differ = np.flatnonzero(got3[d].view(np.int64) != fused[d].view(np.int64))
        assert differ.size <= max(2, N // 100), (what, d, differ.size)
        if differ.size:
            exact = br.add_fused_exact(m3[d], phis, [accel[s][d] for s in range(ns)], refs, dt, differ)
            assert np.array_equal(got3[d][differ].view(np.int64), exact.view(np.int64)), (what, d, differ[:8].tolist())
    return worst


@pytest.mark.parametrize("coef", COEFS)
@pytest.mark.parametrize("n", SMALL, ids=lambda n: "x".join(map(str, n)))
def test_term_cell_by_cell(handles, n, coef):
    Pz, M = handles(n)
    rng = np.random.default_rng(11)
    accel, refs = coefficients(coef, rng)
    phis, m = fields(n, len(accel), 3)
    N = Pz.ncell
    assert N == n[0] * n[1] * n[2]
    # aligned arrays; momrhs 8 bytes off (every component then changes its alignment); the scalars 8 bytes off
    for shift_m, shift_phi in ((0, 0), (1, 0), (0, 1), (1, 1)):
        got = run_kernel(M, N, phis, m, accel, refs, DT, shift_m, shift_phi)
        check(got, m, phis, accel, refs, DT, f"{n} {coef} shifts {shift_m} {shift_phi}")


@pytest.mark.parametrize("coef", COEFS)
def test_beyond_one_round_of_the_grid_stride_loop(handles, coef):
    n = beyond_one_round()
    Pz, M = handles(n)
    rng = np.random.default_rng(12)
    accel, refs = coefficients(coef, rng)
    phis, m = fields(n, len(accel), 4)
    got = run_kernel(M, Pz.ncell, phis, m, accel, refs, DT)
    check(got, m, phis, accel, refs, DT, f"{n} {coef}")


def test_all_zero_coefficients_launch_nothing_and_negative_dt(handles):
    n = (5, 4, 3)
    Pz, M = handles(n)
    phis, m = fields(n, 2, 5)
    got = run_kernel(M, Pz.ncell, phis, m, [[0.0, 0.0, 0.0], [0.0, -0.0, 0.0]], [0.1, 0.2], DT)
    assert np.array_equal(got.view(np.int64), m.view(np.int64))
    accel, refs = [[0.0, 0.0, 9.81], [0.0, 0.0, -3.0]], [0.1, 0.2]
    got = run_kernel(M, Pz.ncell, phis, m, accel, refs, -DT)
    check(got, m, phis, accel, refs, -DT, "negative dt")


def _rank_worker(R, case, blocks, accel, refs):
    import torch
    from fluca_amd.poisson import Momentum
    from tests.test_gpu_config5 import _handle
    Pz, d, s = _handle(R, case)
    with torch.cuda.stream(s):
        M = Momentum(Pz)
        N = Pz.ncell
        phis = [np.ascontiguousarray(b[R.rank]).ravel() for b in blocks["phi"]]
        m = np.concatenate([np.ascontiguousarray(blocks["m"][q][R.rank]).ravel() for q in range(3)])
        assert m.size == 3 * N
        buf = torch.full((GUARD + 3 * N + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        buf[GUARD:GUARD + 3 * N] = torch.as_tensor(m, device="cuda")
        w0 = R.stats()
        M.add_buoyancy(buf[GUARD:GUARD + 3 * N], [torch.as_tensor(p, device="cuda") for p in phis], accel, refs, DT)
        s.synchronize()
        w1 = R.stats()
        assert (w1["messages"], w1["allreduces"]) == (w0["messages"], w0["allreduces"])       # pointwise: nothing crosses a rank face
        got = buf.cpu().numpy()
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + 3 * N:] == SENTINEL).all()
        M.close()
    Pz.close()
    return got[GUARD:GUARD + 3 * N].reshape(3, N).copy()


def test_rank_grid_gives_the_one_rank_bits(handles):
    """2 x 2 x 2 in one process; blocks of 4 x 3 x 3 and 3 x 3 x 2 cells: odd block sizes, components 8 bytes off"""
    from tests import inproc
    n = (7, 6, 5)
    case = rk.Case(n, (2, 2, 2), "dirichlet", uniform=False)
    rng = np.random.default_rng(13)
    accel, refs = coefficients("three-scalars-two-axes", rng)
    phis, m = fields(n, 3, 6)
    Pz, M = handles(n)
    one = run_kernel(M, Pz.ncell, phis, m, accel, refs, DT).reshape(3, -1)
    check(one.ravel(), m, phis, accel, refs, DT, "one rank 7x6x5")
    N = Pz.ncell
    blocks = {"phi": [rk.scatter_cells(case, p) for p in phis], "m": [rk.scatter_cells(case, m[q * N:(q + 1) * N]) for q in range(3)]}
    res = inproc.run_threads(case.size, _rank_worker, case, blocks, accel, refs)
    for q in range(3):
        gathered = rk.gather_cells(case, [res[r][q] for r in range(case.size)]).ravel()
        assert np.array_equal(gathered.view(np.int64), one[q].view(np.int64)), q
