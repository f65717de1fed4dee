"""-m gpu: passive scalars in the host mirror's NSStep on several ranks: the periodic Taylor-Green run of tests/test_gpu_scalar_ns.py at 16^3, four
steps, on the rank grids 2 x 2 x 1 and 2 x 2 x 2 -- one thread, one mesh and one NS per rank, joined by the in-memory transport (the set-up of
tests/test_gpu_ibm_motion.py).  Each scalar equals tests/scalar_reference.py driven by the gathered face velocities read back after each step, to
the derived bound of one step; the flow on a rank grid keeps its bits when scalars are added; NSGetScalarCFL is the same number on every rank."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import inproc
from tests import scalar_reference as sr
from tests.test_gpu_scalar_ns import N, NSTEPS, phi_start, problem

pytestmark = pytest.mark.gpu
P = C.c_void_p
SCALARS = ((0.01, None, 1, 1), (0.0, "superbee", 2, 2))      # gamma, limiter (None: -ns_scalar_limiter), substeps, seed of the start field
OPTS = ("-ns_scalar_limiter", "vanleer", "-ns_scalar_stages", 3)
DT = 0.1


def _worker(R, ranks, with_scalars):
    """tests/test_gpu_scalar_ns.py's run() on one rank of `ranks`: -> this rank's corners, per step its blocks of v, V, p and phi, the Courant numbers"""
    from fluca_amd import capi, hostapi as H
    L = 2 * np.pi
    rho, mu = 1.0, 0.1
    mesh, ns = P(), P()
    assert H.lib.MeshCartCreate3d(1, 1, 1, N, N, N, ranks[0], ranks[1], ranks[2], None, None, None, C.byref(mesh)) == 0
    assert H.lib.MeshSetRank(mesh, R.rank, R.size) == 0
    assert H.lib.MeshSetUp(mesh) == 0 and H.lib.MeshCartSetUniformCoordinates(mesh, 0., L, 0., L, 0., L) == 0
    assert H.lib.NSCreate(C.byref(ns)) == 0 and H.lib.NSSetType(ns, b"cnlinear") == 0 and H.lib.NSSetMesh(ns, mesh) == 0
    assert H.lib.NSSetDensity(ns, rho) == 0 and H.lib.NSSetViscosity(ns, mu) == 0
    for b in range(6):
        assert H.lib.NSSetBoundaryCondition(ns, b, H.NSBoundaryCondition(type=H.NS_BC_PERIODIC)) == 0
    argc, av = H.argv("-ns_time_step_size", DT, "-ns_ksp_type", "richardson", "-ns_ksp_rtol", 1e-8, "-ns_abf_schur_ksp_rtol", 1e-10,
                      "-ns_abf_momentum_ksp_rtol", 1e-10, *OPTS)
    assert H.lib.NSSetFromOptions(ns, argc, av) == 0 and H.lib.NSSetUp(ns) == 0
    hp = P()
    assert H.lib.NSGetPoisson(ns, C.byref(hp)) == 0
    R.attach(hp)
    cc = [C.c_int64() for _ in range(6)]
    assert H.lib.MeshCartGetCorners(mesh, *[C.byref(q) for q in cc]) == 0
    lo, ln = [q.value for q in cc[:3]], [q.value for q in cc[3:]]
    blk = tuple(slice(lo[a], lo[a] + ln[a]) for a in (2, 1, 0))          # periodic everywhere: a rank's faces are those in front of its cells
    shape = (ln[2], ln[1], ln[0])
    ncell = ln[0] * ln[1] * ln[2]
    v, p, V = P(), P(), (C.c_void_p * 3)()
    assert H.lib.NSGetSolutionArrays(ns, C.byref(v), V, C.byref(p)) == 0
    h = L / N
    xc, xf = (np.arange(N) + 0.5) * h, np.arange(N) * h
    Z = np.ones((N, 1, 1))
    ex = lambda xs, ys: (Z * (np.sin(xs)[None, None, :] * np.cos(ys)[None, :, None]), Z * (-np.cos(xs)[None, None, :] * np.sin(ys)[None, :, None]))

    def put(ptr, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        capi.check(capi.lib.fl_memcpy_h2d(0, ptr, a.ctypes.data_as(C.c_void_p), a.size * 8))

    def get(ptr, shp):
        out = np.empty(shp)
        capi.check(capi.lib.fl_memcpy_d2h(0, out.ctypes.data_as(C.c_void_p), ptr, out.size * 8))
        return out
    u0, w0 = ex(xc, xc)
    put(v, np.stack([u0[blk], w0[blk], 0.2 * np.ones(shape)]))
    put(C.c_void_p(V[0]), ex(xf, xc)[0][blk])
    put(C.c_void_p(V[1]), ex(xc, xf)[1][blk])
    put(C.c_void_p(V[2]), 0.2 * np.ones(shape))
    X, Y = np.meshgrid(xc, xc, indexing="xy")
    put(p, (Z * (rho / 4 * (np.cos(2 * X) + np.cos(2 * Y)))[None, :, :])[blk])
    ids, arrays, rcs = [], [], []
    if with_scalars:
        for gamma, limiter, substeps, seed in SCALARS:
            sid, ptr = C.c_int(-1), P()
            rcs.append(H.lib.NSAddScalar(ns, b"dye%d" % len(ids), gamma, None if limiter is None else limiter.encode(), C.byref(sid)))
            assert rcs[-1] == 0 and sid.value == len(ids)
            assert H.lib.NSSetScalarSubsteps(ns, sid.value, substeps) == 0
            assert H.lib.NSGetScalarArray(ns, sid.value, C.byref(ptr)) == 0 and ptr.value
            assert np.all(get(ptr, shape) == 0.0)                        # the rank's block, zeroed
            put(ptr, phi_start(seed)[blk])
            ids.append(sid.value)
            arrays.append(ptr)
    steps, cfls = [], []
    for _ in range(NSTEPS):
        assert H.lib.NSStep(ns) == 0
        steps.append((get(v, (3, ncell)), [get(C.c_void_p(V[d]), shape) for d in range(3)], get(p, shape), [get(a, shape) for a in arrays]))
        out = (C.c_double * 2)()
        for sid in ids:
            assert H.lib.NSGetScalarCFL(ns, sid, out) == 0
            cfls.append((out[0], out[1]))
    H.lib.NSDestroy(C.byref(ns))
    H.lib.MeshDestroy(C.byref(mesh))
    return dict(blk=blk, steps=steps, cfls=cfls, rcs=rcs)


def _gather(parts, pick):
    out = np.full((N, N, N), np.nan)
    for part in parts:
        out[part["blk"]] = pick(part)
    assert not np.isnan(out).any()
    return out


@functools.lru_cache(maxsize=None)
def _runs(ranks):
    from fluca_amd import build
    build.build()
    size = ranks[0] * ranks[1] * ranks[2]
    return inproc.run_threads(size, _worker, ranks, False), inproc.run_threads(size, _worker, ranks, True)


RANK_GRIDS = [(2, 2, 1), (2, 2, 2)]
ids = lambda r: "x".join(map(str, r))


@pytest.mark.parametrize("ranks", RANK_GRIDS, ids=ids)
def test_add_scalar_on_several_ranks_and_the_flow_keeps_its_bits(ranks):
    plain, scal = _runs(ranks)
    for a, b in zip(plain, scal):
        assert b["rcs"] == [0, 0]                                      # NSAddScalar on a several-rank mesh
        for (v0, V0, p0, _), (v1, V1, p1, _) in zip(a["steps"], b["steps"]):
            assert np.array_equal(v0, v1) and np.array_equal(p0, p1) and all(np.array_equal(x, y) for x, y in zip(V0, V1))
    assert np.abs(plain[0]["steps"][-1][0] - plain[0]["steps"][0][0]).max() > 1e-3          # (and it moves)


@pytest.mark.parametrize("ranks", RANK_GRIDS, ids=ids)
def test_scalars_follow_the_reference_with_the_gathered_velocity(ranks):
    _, scal = _runs(ranks)
    for part in scal:
        assert part["cfls"] == scal[0]["cfls"]                         # NSGetScalarCFL: the same numbers on every rank
    cfls = scal[0]["cfls"]
    P0, P1 = problem(0.01, "vanleer"), problem(0.0, "superbee")
    before = [phi_start(1), phi_start(2)]
    for it in range(NSTEPS):
        V = [_gather(scal, lambda part, d=d: part["steps"][it][1][d]) for d in range(3)]
        phis = [_gather(scal, lambda part, a=a: part["steps"][it][3][a]) for a in range(2)]
        # scalar 0: one step of s = 3 with the options' limiter
        want, B = sr.step(P0, before[0], V, DT, 3, None, np.longdouble, bounds=True)
        err = np.abs(phis[0].astype(np.longdouble) - want).astype(np.float64)
        assert (err <= np.asarray(B, dtype=np.float64) * (1 + 2.0 ** -10)).all(), (it, float(err.max()), float(B.max()))
        assert cfls[2 * it] == pytest.approx(sr.cfl(P0, V, DT), rel=1e-12)
        # scalar 1: two half steps
        half, B1 = sr.step(P1, before[1], V, DT / 2, 3, None, np.longdouble, bounds=True)
        want, B2 = sr.step(P1, half, V, DT / 2, 3, None, np.longdouble, bounds=True, eps_in=float(B1.max()))
        err = np.abs(phis[1].astype(np.longdouble) - want).astype(np.float64)
        assert (err <= np.asarray(B2, dtype=np.float64) * (1 + 2.0 ** -10)).all(), (it, float(err.max()), float(B2.max()))
        assert cfls[2 * it + 1][0] == pytest.approx(sr.cfl(P1, V, DT / 2)[0], rel=1e-12) and cfls[2 * it + 1][1] == 0.0
        before = phis
    assert np.abs(before[0] - phi_start(1)).max() > 0.05
