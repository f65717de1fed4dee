"""-m gpu: scalars that drive the flow, through the host mirror's NSStep (include/fluca_host.h: NSSetGravity, NSSetScalarBuoyancy,
NSGetScalarBoundaryFlux).

1. inert when off: gravity with every beta = 0, and beta != 0 with g = 0, leave the Taylor-Green run of tests/test_gpu_scalar_ns.py bit for bit
2. the term reaches the right-hand side: r.v of NSGetSolverVectors with and without buoyancy differ by the long-double term, r.V and r.p keep their bits
3. three whole steps of a closed, differentially heated 12^3 cavity against tests/buoyancy_reference.BuoyantStep, with the solver options and the
   tolerances of tests/test_host_mirror.py::test_nsstep_matches_the_oracle_step
4. NSGetScalarBoundaryFlux after those steps against the reference on the fields read back
5. the 2 x 2 x 1 rank grid in one process: the right-hand side of item 2 bit for bit, the steps of item 3 within the tolerance of
   tests/test_gpu_config5.py::test_nsstep_with_the_immersed_cylinder_on_the_2x2x2_rank_grid (several ranks against one rank, its solver options)
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import buoyancy_reference as br
from tests import inproc
from tests import scalar_reference as sr
from tests import step_rhs as sh

pytestmark = pytest.mark.gpu
P = C.c_void_p
U = sr.U


@pytest.fixture(scope="module")
def H():
    from fluca_amd import build
    build.build()
    from fluca_amd import hostapi
    return hostapi


# ------------------------------------------------------------------------------------------------ 1. inert when off

def tg_run(H, gravity=None, buoyancy=None, view=None):
    """three steps of the periodic Taylor-Green set-up of tests/test_gpu_scalar_ns.py with one scalar.  -> per step (v, V, p, phi)"""
    from tests.test_gpu_scalar_ns import N, phi_start
    L = 2 * np.pi
    rho, mu, dt = 1.0, 0.1, 0.1
    mesh, ns = P(), P()
    assert H.lib.MeshCartCreate3d(1, 1, 1, N, N, N, -1, -1, -1, None, None, None, C.byref(mesh)) == 0
    assert H.lib.MeshSetUp(mesh) == 0 and H.lib.MeshCartSetUniformCoordinates(mesh, 0., L, 0., L, 0., L) == 0
    assert H.lib.NSCreate(C.byref(ns)) == 0 and H.lib.NSSetType(ns, b"cnlinear") == 0 and H.lib.NSSetMesh(ns, mesh) == 0
    assert H.lib.NSSetDensity(ns, rho) == 0 and H.lib.NSSetViscosity(ns, mu) == 0
    for b in range(6):
        assert H.lib.NSSetBoundaryCondition(ns, b, H.NSBoundaryCondition(type=H.NS_BC_PERIODIC)) == 0
    argc, av = H.argv("-ns_time_step_size", dt, "-ns_ksp_type", "richardson", "-ns_ksp_rtol", 1e-8, "-ns_abf_schur_ksp_rtol", 1e-10,
                      "-ns_abf_momentum_ksp_rtol", 1e-10)
    assert H.lib.NSSetFromOptions(ns, argc, av) == 0 and H.lib.NSSetUp(ns) == 0
    v, p, V = P(), P(), (C.c_void_p * 3)()
    assert H.lib.NSGetSolutionArrays(ns, C.byref(v), V, C.byref(p)) == 0
    h = L / N
    xc, xf = (np.arange(N) + 0.5) * h, np.arange(N) * h
    Z = np.ones((N, 1, 1))
    ex = lambda xs, ys: (Z * (np.sin(xs)[None, None, :] * np.cos(ys)[None, :, None]), Z * (-np.cos(xs)[None, None, :] * np.sin(ys)[None, :, None]))
    put = lambda ptr, a: H.capi.check(H.capi.lib.fl_memcpy_h2d(0, ptr, np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.c_void_p), a.size * 8))

    def get(ptr, shape):
        out = np.empty(shape)
        H.capi.check(H.capi.lib.fl_memcpy_d2h(0, out.ctypes.data_as(C.c_void_p), ptr, out.size * 8))
        return out
    u0, w0 = ex(xc, xc)
    put(v, np.stack([u0, w0, 0.2 * np.ones_like(u0)]))
    put(C.c_void_p(V[0]), ex(xf, xc)[0])
    put(C.c_void_p(V[1]), ex(xc, xf)[1])
    put(C.c_void_p(V[2]), 0.2 * np.ones((N, N, N)))
    X, Y = np.meshgrid(xc, xc, indexing="xy")
    put(p, Z * (rho / 4 * (np.cos(2 * X) + np.cos(2 * Y)))[None, :, :])
    sid, ptr = C.c_int(-1), P()
    assert H.lib.NSAddScalar(ns, b"temperature", 0.01, None, C.byref(sid)) == 0 and sid.value == 0
    assert H.lib.NSGetScalarArray(ns, 0, C.byref(ptr)) == 0
    put(ptr, phi_start(1))
    # the errors that need a set-up NS: a bad id, a value that is not finite
    out = (C.c_double * 12)()
    for bad in (-1, 1, 8):
        assert H.lib.NSSetScalarBuoyancy(ns, bad, 1.0, 0.0) == H.ERR_ARG_OUTOFRANGE and H.lib.NSGetScalarBoundaryFlux(ns, bad, out) == H.ERR_ARG_OUTOFRANGE
    for bad in (float("nan"), float("inf")):
        assert H.lib.NSSetScalarBuoyancy(ns, 0, bad, 0.0) == H.ERR_ARG_OUTOFRANGE and H.lib.NSSetScalarBuoyancy(ns, 0, 1.0, bad) == H.ERR_ARG_OUTOFRANGE
    if gravity is not None:
        assert H.lib.NSSetGravity(ns, (C.c_double * 3)(*gravity)) == 0
    if buoyancy is not None:
        assert H.lib.NSSetScalarBuoyancy(ns, 0, *buoyancy) == 0
    text = None
    if view is not None:
        vw = P()
        assert H.lib.FlucaViewerASCIIOpen(str(view).encode(), C.byref(vw)) == 0 and H.lib.NSView(ns, vw) == 0
        assert H.lib.FlucaViewerDestroy(C.byref(vw)) == 0
        text = open(view).read()
    steps = []
    for _ in range(3):
        assert H.lib.NSStep(ns) == 0
        steps.append((get(v, (3, N, N, N)), [get(C.c_void_p(V[d]), (N, N, N)) for d in range(3)], get(p, (N, N, N)), get(ptr, (N, N, N))))
    # a fully periodic box has no wall: exactly twelve zeros
    assert H.lib.NSGetScalarBoundaryFlux(ns, 0, out) == 0 and list(out) == [0.0] * 12
    H.lib.NSDestroy(C.byref(ns))
    H.lib.MeshDestroy(C.byref(mesh))
    return steps, text


def test_inert_when_off(H, tmp_path):
    plain, t0 = tg_run(H, view=tmp_path / "plain.txt")
    only_g, t1 = tg_run(H, gravity=(0.0, -9.81, 0.5), buoyancy=(0.0, 0.3), view=tmp_path / "g.txt")
    only_beta, t2 = tg_run(H, gravity=(0.0, 0.0, 0.0), buoyancy=(2.0, 0.3), view=tmp_path / "beta.txt")
    both, t3 = tg_run(H, gravity=(0.0, -9.81, 0.5), buoyancy=(2.0, 0.3), view=tmp_path / "both.txt")
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    for other in (only_g, only_beta):
        for (v0, V0, p0, f0), (v1, V1, p1, f1) in zip(plain, other):
            assert np.array_equal(bits(v0), bits(v1)) and np.array_equal(bits(p0), bits(p1)) and np.array_equal(bits(f0), bits(f1))
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(V0, V1))
    assert np.abs(both[-1][0] - plain[-1][0]).max() > 1e-3            # (and with both the flow does move)
    # NSView: gravity and the (beta, phi_ref) pairs only while the term is active
    assert t0 == t1 == t2 and "Gravity" not in t0
    assert t3.startswith(t0.rstrip("\n")) and "Gravity: (0, -9.81, 0.5)" in t3 and "Buoyant scalar temperature: beta 2, reference 0.3" in t3


# ------------------------------------------------------------------------------------------------ scalars on a step_rhs.Mirror

def add_scalars(M, specs, gravity):
    """specs: dicts name, gamma, start (global field), bc {boundary: (kind, value)}, beta, ref.  -> the device arrays"""
    H = M.H
    g = M.case.grid()
    cs, _ = sh.shapes(g)
    ptrs = []
    for k, s in enumerate(specs):
        sid, ptr = C.c_int(-1), P()
        assert H.lib.NSAddScalar(M.ns, s["name"].encode(), s["gamma"], None, C.byref(sid)) == 0 and sid.value == k
        for b, (kind, val) in s.get("bc", {}).items():
            assert H.lib.NSSetScalarBoundaryCondition(M.ns, k, b, kind, val) == 0
        assert H.lib.NSGetScalarArray(M.ns, k, C.byref(ptr)) == 0
        M._put(ptr, sh.block_of(s["start"], cs, M.lo, M.ln))
        if s.get("beta") is not None:
            assert H.lib.NSSetScalarBuoyancy(M.ns, k, s["beta"], s["ref"]) == 0
        ptrs.append(ptr)
    if gravity is not None:
        assert H.lib.NSSetGravity(M.ns, (C.c_double * 3)(*gravity)) == 0
        back = (C.c_double * 3)()
        assert H.lib.NSGetGravity(M.ns, back) == 0 and tuple(back) == tuple(float(x) for x in gravity)
    return ptrs


def gather_cells(parts, key, g):
    cs, _ = sh.shapes(g)
    out = np.full(cs, np.nan)
    for r in parts:
        lo, ln = r["lo"], r["ln"]
        out[lo[2]:lo[2] + ln[2], lo[1]:lo[1] + ln[1], lo[0]:lo[0] + ln[0]] = r[key].reshape(ln[2], ln[1], ln[0])
    assert not np.isnan(out).any()
    return out


# ------------------------------------------------------------------------------------------------ 2. the term reaches the right-hand side

RHS_N = (12, 10, 8)
RHS_GRAVITY = (0.0, -9.81, 3.0)
RHS_BETA, RHS_REF = (0.8, -1.7), (0.2, -0.1)


def rhs_fields():
    rng = np.random.default_rng(41)
    return [rng.uniform(-1.0, 1.0, (RHS_N[2], RHS_N[1], RHS_N[0])) for _ in range(2)]


def _rhs_run(R, ranks, buoyant):
    case = sh.make_case(RHS_N, sh.SIX_WALLS, True)
    g = case.grid()
    st = sh.random_state(g, 77)
    M = sh.Mirror(case, (), R, ranks)
    try:
        phis = rhs_fields()
        specs = [dict(name="s%d" % k, gamma=0.0, start=phis[k], beta=RHS_BETA[k] if buoyant else None, ref=RHS_REF[k]) for k in range(2)]
        add_scalars(M, specs, RHS_GRAVITY if buoyant else None)
        M.put_state(g, st)
        M.set_time(3, 3 * sh.DT)
        M.step()
        return M.rhs()
    finally:
        M.close()


@functools.lru_cache(maxsize=None)
def rhs_one_rank(buoyant):
    return _rhs_run(None, (1, 1, 1), buoyant)


def test_term_reaches_the_right_hand_side(H):
    off, on = rhs_one_rank(False), rhs_one_rank(True)
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    assert np.array_equal(bits(off["p"]), bits(on["p"])) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(off["V"], on["V"]))
    phis = rhs_fields()
    accel = [[-RHS_BETA[s] * gd for gd in RHS_GRAVITY] for s in range(2)]
    T, Mag = br.term(phis, accel, RHS_REF, sh.DT)
    N = phis[0].size
    base, got = off["v"].reshape(3, N), on["v"].reshape(3, N)
    want = base.astype(np.longdouble) + T
    tol = (2 * 2 + 4) * U * (np.abs(base) + Mag.astype(np.float64))
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    print(f"r.v with buoyancy - (r.v without + term): largest error / bound = {float((err / tol).max()):.3f}")
    assert np.array_equal(bits(base[0]), bits(got[0]))                 # g_x = 0: the x component is not touched
    assert (err <= tol).all(), (int((err > tol).sum()), float((err / tol).max()))
    assert np.abs(got[1:] - base[1:]).min() > 0 and np.abs(got[1] - base[1]).max() > 1e-3


def test_right_hand_side_on_2x2x1_ranks_bit_for_bit(H):
    case = sh.make_case(RHS_N, sh.SIX_WALLS, True)
    g = case.grid()
    parts = inproc.run_threads(4, _rhs_run, (2, 2, 1), True)
    v, Vg, p = sh.gather(parts, g)
    one = rhs_one_rank(True)
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    assert np.array_equal(bits(v), bits(one["v"])), int((v != one["v"]).sum())
    assert np.array_equal(bits(p), bits(one["p"])) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(Vg, one["V"]))


# ------------------------------------------------------------------------------------------------ 3. - 5. whole steps of the heated cavity

CAV_N = (12, 12, 12)
CAV_GRAVITY = (0.0, -9.81, 0.0)
CAV_BETA, CAV_REF, CAV_GAMMA = 2.0, 0.5, 0.01
NSTEPS = 3
# the options of tests/test_host_mirror.py::test_nsstep_matches_the_oracle_step (GMRES is the default it runs with; step_rhs.Mirror appends its cheap
# options behind these, and the first occurrence of an option counts)
ORACLE_OPTS = ("-ns_ksp_type", "gmres", "-ns_ksp_rtol", 1e-9, "-ns_abf_schur_ksp_rtol", 1e-10, "-ns_abf_momentum_ksp_rtol", 1e-10, "-ns_abf_schur_ksp_max_it", 20000,
               "-ns_abf_momentum_ksp_max_it", 10000)
# those of tests/test_gpu_config5.py::_mirror_run, whose several-rank run is compared with one rank to 1e-8 (v, V) and 1e-7 (p)
RANK_OPTS = ("-ns_ksp_type", "gmres", "-ns_ksp_rtol", 1e-10, "-ns_abf_schur_ksp_rtol", 1e-12, "-ns_abf_momentum_ksp_rtol", 1e-12, "-ns_abf_schur_ksp_max_it", 20000,
             "-ns_abf_momentum_ksp_max_it", 10000)


def still_walls(b, t, X):
    return np.zeros((3, len(np.asarray(X).reshape(-1, 3))))


def cavity_case():
    return sh.make_case(CAV_N, sh.SIX_WALLS, stretched=False, velocity=still_walls)


def cavity_start():
    """temperature: the conduction profile between the hot wall x = 0 (1) and the cold wall x = 1 (0), perturbed; dye: random in [0, 1]"""
    case = cavity_case()
    rng = np.random.default_rng(43)
    shp = (CAV_N[2], CAV_N[1], CAV_N[0])
    T = (1.0 - case.xc[0])[None, None, :] + 0.1 * rng.uniform(-1.0, 1.0, shp)
    return T, rng.uniform(0.0, 1.0, shp)


def cavity_problems():
    case = cavity_case()
    kinds = (sr.DIRICHLET, sr.DIRICHLET) + (sr.NEUMANN,) * 4
    PT = sr.Problem(case.xf, kinds, (1.0, 0.0, 0.0, 0.0, 0.0, 0.0), gamma=CAV_GAMMA, limiter="superbee", xc=case.xc)
    PD = sr.Problem(case.xf, (sr.NEUMANN,) * 6, (0.0,) * 6, gamma=0.0, limiter="superbee", xc=case.xc)
    return PT, PD


def _cavity_run(R, ranks, opts, gravity):
    """-> this rank's state, temperature, dye after each step and the temperature's wall fluxes after the last"""
    case = cavity_case()
    g = case.grid()
    M = sh.Mirror(case, opts, R, ranks)
    try:
        T0, D0 = cavity_start()
        specs = [dict(name="temperature", gamma=CAV_GAMMA, start=T0, bc={0: (0, 1.0), 1: (0, 0.0)}, beta=CAV_BETA, ref=CAV_REF),
                 dict(name="dye", gamma=0.0, start=D0)]
        ptrs = add_scalars(M, specs, gravity)
        zero = dict(v=np.zeros(3 * g.ncell), V=[np.zeros(nf) for nf in g.nface], p=np.zeros(g.ncell), phalf=np.zeros(g.ncell))
        M.put_state(g, zero)
        M.set_time(0, 0.0)
        steps = []
        for _ in range(NSTEPS):
            M.step()
            st = M.get_state()
            st["T"], st["dye"] = M._get(ptrs[0], M.sz[0]), M._get(ptrs[1], M.sz[0])
            steps.append(st)
        out = (C.c_double * 12)()
        assert M.H.lib.NSGetScalarBoundaryFlux(M.ns, 0, out) == 0
        return dict(steps=steps, flux=np.array(list(out)).reshape(6, 2))
    finally:
        M.close()


@functools.lru_cache(maxsize=None)
def cavity_one_rank(opts, gravity):
    return _cavity_run(None, (1, 1, 1), opts, gravity)


def global_fields(parts_step, g):
    """v, V[3], p, T, dye on the global grid from the ranks' blocks of one step"""
    v, Vg, p = sh.gather(parts_step, g)
    return v, Vg, p, gather_cells(parts_step, "T", g), gather_cells(parts_step, "dye", g)


def test_heated_cavity_steps_match_the_buoyant_oracle(H):
    case = cavity_case()
    g = case.grid()
    run = cavity_one_rank(ORACLE_OPTS, CAV_GRAVITY)
    PT, PD = cavity_problems()
    fs = PT.shapes()[1]
    T_or, D_or = cavity_start()
    T_prev, D_prev = T_or, D_or
    so = br.BuoyantStep(g, sh.DT, sh.RHO, sh.MU, still_walls, krylov_rtol=1e-10, outer_rtol=1e-9, gravity=CAV_GRAVITY,
                        scalars=[(T_or, CAV_BETA, CAV_REF), (D_or, 0.0, 0.0)])
    vo, Vo, po = np.zeros(3 * g.ncell), [np.zeros(nf) for nf in g.nface], np.zeros(g.ncell)
    for it in range(NSTEPS):
        vo, Vo, po, info = so.step_once(vo, Vo, po)
        v, Vg, p, T, dye = global_fields([run["steps"][it]], g)
        Vr = [Vg[d].reshape(fs[d]) for d in range(3)]
        # the scalars follow the reference driven by the face velocities read back, to the derived bound of one step (tests/test_gpu_scalar_ns.py);
        # for the dye that reference IS the run in which it is the only scalar: nothing of the temperature or of the buoyancy enters it but V
        for name, Pr, got, prev in (("temperature", PT, T, T_prev), ("dye", PD, dye, D_prev)):
            want, B = sr.step(Pr, prev, Vr, sh.DT, 5, None, np.longdouble, bounds=True)
            err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
            print(f"step {it} {name}: largest error / bound = {float((err / np.asarray(B, dtype=np.float64)).max()):.3f}")
            assert (err <= np.asarray(B, dtype=np.float64) * (1 + 2.0 ** -10)).all(), (it, name, float(err.max()), float(B.max()))
        # the oracle's own scalars, advanced with the same velocities: the next step's buoyancy uses them
        T_or, D_or = sr.step(PT, T_or, Vr, sh.DT, 5), sr.step(PD, D_or, Vr, sh.DT, 5)
        so.scalars = [(T_or, CAV_BETA, CAV_REF), (D_or, 0.0, 0.0)]
        T_prev, D_prev = T, dye
    # the tolerances of test_nsstep_matches_the_oracle_step
    print(f"|v - oracle| / |oracle| = {np.linalg.norm(v - vo) / np.linalg.norm(vo):.3e}, p: "
          f"{np.linalg.norm((p - p.mean()) - (po - po.mean())) / np.linalg.norm(po - po.mean()):.3e}")
    assert np.abs(vo).max() > 0.01
    assert np.linalg.norm(v - vo) <= 1e-6 * np.linalg.norm(vo)
    for d in range(3):
        assert np.linalg.norm(Vg[d] - Vo[d]) <= 1e-6 * max(np.linalg.norm(Vo[d]), 1e-12)
    assert np.linalg.norm((p - p.mean()) - (po - po.mean())) <= 1e-5 * np.linalg.norm(po - po.mean())
    # the test can see the term: the run without gravity is further away than a thousand times that tolerance
    still = cavity_one_rank(ORACLE_OPTS, None)
    v_still = global_fields([still["steps"][-1]], g)[0]
    assert np.linalg.norm(v - v_still) > 1e3 * 1e-6 * np.linalg.norm(vo)
    assert np.abs(dye - cavity_start()[1]).max() > 1e-4                   # (the dye is carried)


def test_boundary_flux_after_the_steps(H):
    case = cavity_case()
    g = case.grid()
    run = cavity_one_rank(ORACLE_OPTS, CAV_GRAVITY)
    PT, _ = cavity_problems()
    fs = PT.shapes()[1]
    v, Vg, p, T, dye = global_fields([run["steps"][-1]], g)
    Vr = [Vg[d].reshape(fs[d]) for d in range(3)]
    want, bound = br.wall_fluxes(PT, T, Vr, np.longdouble)
    got = run["flux"]
    err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    tol = br.slack(bound)
    print(f"wall fluxes: largest error / bound = {float((err / tol).max()):.3f}; hot wall {got[0].tolist()}, cold wall {got[1].tolist()}")
    assert (err <= tol).all(), (got.tolist(), np.asarray(want, dtype=np.float64).tolist())
    # heat enters through the hot wall and leaves through the cold one: both fluxes point along +x
    assert got[0, 1] > 0 and got[1, 1] > 0
    assert (got[2:, 1] == 0.0).all()                                       # insulated elsewhere


def test_heated_cavity_on_2x2x1_ranks(H):
    case = cavity_case()
    g = case.grid()
    parts = inproc.run_threads(4, _cavity_run, (2, 2, 1), RANK_OPTS, CAV_GRAVITY)
    one = cavity_one_rank(RANK_OPTS, CAV_GRAVITY)
    v, Vg, p, T, dye = global_fields([r["steps"][-1] for r in parts], g)
    v1, V1, p1, T1, dye1 = global_fields([one["steps"][-1]], g)
    print(f"2x2x1 against one rank: v {np.linalg.norm(v - v1) / np.linalg.norm(v1):.3e}, p {np.linalg.norm(p - p1) / np.linalg.norm(p1):.3e}, "
          f"T {np.abs(T - T1).max():.3e}")
    assert np.linalg.norm(v1) > 0.01
    assert np.linalg.norm(v - v1) <= 1e-8 * np.linalg.norm(v1)
    for d in range(3):
        assert np.linalg.norm(Vg[d] - V1[d]) <= 1e-8 * max(np.linalg.norm(V1[d]), 1e-12), d
    assert np.linalg.norm(p - p1) <= 1e-7 * np.linalg.norm(p1)
    assert np.abs(T - T1).max() <= 1e-8 and np.abs(dye - dye1).max() <= 1e-8
    # the wall flux is collective: the same bits on every rank, and the one-rank number up to the velocities' difference and the order of the sums
    for r in parts:
        assert np.array_equal(r["flux"].view(np.int64), parts[0]["flux"].view(np.int64))
    assert np.allclose(parts[0]["flux"], one["flux"], rtol=1e-7, atol=1e-12)
