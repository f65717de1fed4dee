"""-m gpu: implicit scalar diffusion through the host mirror's NSStep (include/fluca_host.h: NSSetScalarImplicit, NSGetScalarImplicitInfo, the options
-ns_scalar_implicit_theta / -ns_scalar_implicit_rtol) on the closed, differentially heated 12^3 cavity of tests/test_gpu_buoyancy_ns.py, three steps.

  off        theta = 0 (the default, and set explicitly): the bits of the run that never makes the call
  Gamma = 0  theta = 1 on the dye, whose diffusivity is 0: also those bits
  on         theta = 1 on a temperature whose diffusive number is about 8.6 per step (the explicit step's limit with five stages is 4): after every step the
             temperature against ir.imex_step driven by the face velocities read back, within the tolerance of tests/test_gpu_scalar_implicit.py's IMEX
             check, and NSGetScalarImplicitInfo = ir's count
  options    the option strings give the bits of the call; values out of range are refused
  two ranks  theta != 0 on a 2 x 1 x 1 mesh: PETSC_ERR_SUP (56); theta = 0 is accepted there"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import inproc
from tests import scalar_implicit_reference as ir
from tests import scalar_reference as sr
from tests import step_rhs as sh
from tests.test_gpu_buoyancy_ns import CAV_BETA, CAV_GAMMA, CAV_GRAVITY, CAV_REF, NSTEPS, ORACLE_OPTS, add_scalars, cavity_case, cavity_problems, cavity_start, global_fields

pytestmark = pytest.mark.gpu
P = C.c_void_p
HOT_GAMMA = 5.0            # dt Gamma sum_d 2 / h^2 = 2e-3 * 5 * 864 = 8.64
RTOL = 1e-6
FLOOR_MARGIN = 8.0


@pytest.fixture(scope="module")
def H():
    from fluca_amd import build
    build.build()
    from fluca_amd import hostapi
    return hostapi


def _run(R, ranks, opts, gamma, calls):
    """calls: (scalar id, theta, rtol) for NSSetScalarImplicit.  -> per step the state, temperature, dye and (steps, bound) of both scalars"""
    case = cavity_case()
    g = case.grid()
    M = sh.Mirror(case, opts, R, ranks)
    try:
        T0, D0 = cavity_start()
        specs = [dict(name="temperature", gamma=gamma, start=T0, bc={0: (0, 1.0), 1: (0, 0.0)}, beta=CAV_BETA, ref=CAV_REF), dict(name="dye", gamma=0.0, start=D0)]
        ptrs = add_scalars(M, specs, CAV_GRAVITY)
        k, B = C.c_int(-1), C.c_double(-1.0)
        assert M.H.lib.NSGetScalarImplicitInfo(M.ns, 0, C.byref(k), C.byref(B)) == 0 and (k.value, B.value) == (0, 1.0)
        for sid, theta, rtol in calls:
            assert M.H.lib.NSSetScalarImplicit(M.ns, sid, theta, rtol) == 0
        zero = dict(v=np.zeros(3 * g.ncell), V=[np.zeros(nf) for nf in g.nface], p=np.zeros(g.ncell), phalf=np.zeros(g.ncell))
        M.put_state(g, zero)
        M.set_time(0, 0.0)
        steps = []
        for _ in range(NSTEPS):
            M.step()
            st = M.get_state()
            st["T"], st["dye"] = M._get(ptrs[0], M.sz[0]), M._get(ptrs[1], M.sz[0])
            st["info"] = []
            for sid in range(2):
                assert M.H.lib.NSGetScalarImplicitInfo(M.ns, sid, C.byref(k), C.byref(B)) == 0
                st["info"].append((k.value, B.value))
            cfl = (C.c_double * 2)()
            assert M.H.lib.NSGetScalarCFL(M.ns, 0, cfl) == 0
            st["cfl"] = tuple(cfl)
            steps.append(st)
        return steps
    finally:
        M.close()


@functools.lru_cache(maxsize=None)
def run(opts=ORACLE_OPTS, gamma=CAV_GAMMA, calls=()):
    return _run(None, (1, 1, 1), opts, gamma, calls)


def same_bits(a, b):
    bits = lambda x: np.ascontiguousarray(x).view(np.int64)
    for sa, sb in zip(a, b):
        for key in ("v", "p", "T", "dye"):
            if not np.array_equal(bits(sa[key]), bits(sb[key])):
                return False
        if not all(np.array_equal(bits(x), bits(y)) for x, y in zip(sa["V"], sb["V"])):
            return False
    return len(a) == len(b) == NSTEPS


def test_off_by_default_and_with_theta_zero(H):
    plain = run()
    assert same_bits(plain, run(calls=((0, 0.0, RTOL), (1, 0.0, 1e-3))))
    assert all(st["info"] == [(0, 1.0), (0, 1.0)] for st in plain)
    assert np.abs(plain[-1]["T"] - plain[0]["T"]).max() > 1e-6 and np.abs(plain[-1]["v"]).max() > 1e-3          # (and the run moves)


def test_on_without_diffusivity_is_the_explicit_step(H):
    on = run(calls=((1, 1.0, RTOL),))
    assert same_bits(run(), on)
    assert all(st["info"][1] == (0, 1.0) for st in on)


def test_on_follows_the_imex_reference(H):
    case = cavity_case()
    g = case.grid()
    steps = run(gamma=HOT_GAMMA, calls=((0, 1.0, RTOL),))
    PT = ir.with_gamma(cavity_problems()[0], HOT_GAMMA)
    fs = PT.shapes()[1]
    prev = cavity_start()[0]
    ld = np.longdouble
    c = sh.DT * HOT_GAMMA
    emin, emax = ir.interval(PT, c)
    k, Bk = ir.steps(emin, emax, RTOL, 100000)
    w = ir.weights(PT, c)
    for it, st in enumerate(steps):
        v, Vg, p, T, dye = global_fields([st], g)
        Vr = [Vg[d].reshape(fs[d]) for d in range(3)]
        want, star, b, Bx = ir.imex_step(PT, prev, Vr, sh.DT, 5, 1.0, None, bounds=True)
        assert st["info"][0][0] == k and abs(st["info"][0][1] - Bk) <= 64 * k * sr.U * Bk, (st["info"], k, Bk)
        assert st["cfl"][1] == pytest.approx(sr.cfl(PT, Vr, sh.DT)[1], rel=1e-12) and st["cfl"][1] > 8.0          # NSGetScalarCFL keeps reporting both numbers
        star64 = np.asarray(star, dtype=np.float64)
        yard = ir.wnorm(w, ir.chebyshev(PT, c, star64, star64, k, np.float64) - ir.chebyshev(PT, c, star64, star64, k, ld))
        explicit = float(np.max(Bx)) * (1 + 2.0 ** -10) * float(np.sqrt(w.sum()))
        e0, e = ir.wnorm(w, star - want), ir.wnorm(w, T.astype(ld) - want)
        tol = (1 + Bk) * explicit + Bk * e0 + FLOOR_MARGIN * yard
        print(f"step {it}: k = {k}, |e| = {e:.3e}, explicit {explicit:.3e}, B_k |e0| = {Bk * e0:.3e}, floor {FLOOR_MARGIN * yard:.3e}")
        assert e <= tol, (it, e, tol)
        assert np.isfinite(T).all() and T.min() >= -0.2 and T.max() <= 1.2
        prev = T
    # the implicit step is not the explicit one: the first step of the explicit reference with the same velocities is somewhere else
    Vg = global_fields([steps[0]], g)[1]
    other = sr.step(PT, cavity_start()[0], [Vg[d].reshape(fs[d]) for d in range(3)], sh.DT, 5)
    assert np.abs(global_fields([steps[0]], g)[3] - other).max() > 1e-3


def test_the_option_strings_parse(H):
    by_call = run(gamma=HOT_GAMMA, calls=((0, 1.0, 1e-5),))
    by_option = run(opts=ORACLE_OPTS + ("-ns_scalar_implicit_theta", 1.0, "-ns_scalar_implicit_rtol", 1e-5), gamma=HOT_GAMMA)
    assert same_bits(by_call, by_option)
    assert by_option[-1]["info"][0][0] > 0 and by_option[-1]["info"][0] == by_call[-1]["info"][0]
    assert by_option[-1]["info"][0][0] < run(gamma=HOT_GAMMA, calls=((0, 1.0, RTOL),))[-1]["info"][0][0]          # (the rtol reached the solve)
    for bad in (("-ns_scalar_implicit_theta", 0.3), ("-ns_scalar_implicit_theta", 1.5), ("-ns_scalar_implicit_rtol", 0.0), ("-ns_scalar_implicit_rtol", 1.0)):
        ns = P()
        assert H.lib.NSCreate(C.byref(ns)) == 0 and H.lib.NSSetType(ns, b"cnlinear") == 0
        argc, av = H.argv(*bad)
        assert H.lib.NSSetFromOptions(ns, argc, av) == H.ERR_ARG_OUTOFRANGE, bad
        H.lib.NSDestroy(C.byref(ns))


def test_argument_errors(H):
    M = sh.Mirror(cavity_case(), ORACLE_OPTS, None, (1, 1, 1))
    try:
        add_scalars(M, [dict(name="t", gamma=0.1, start=cavity_start()[0])], None)
        f = M.H.lib.NSSetScalarImplicit
        for theta, rtol in ((0.3, 1e-6), (1.1, 1e-6), (-0.5, 1e-6), (float("nan"), 1e-6), (1.0, 0.0), (1.0, 1.0), (1.0, float("nan"))):
            assert f(M.ns, 0, theta, rtol) == H.ERR_ARG_OUTOFRANGE, (theta, rtol)
        assert f(M.ns, 1, 1.0, 1e-6) == H.ERR_ARG_OUTOFRANGE and f(None, 0, 1.0, 1e-6) == H.ERR_ARG_NULL
        k, B = C.c_int(), C.c_double()
        g = M.H.lib.NSGetScalarImplicitInfo
        assert g(M.ns, 0, None, C.byref(B)) == H.ERR_ARG_NULL and g(M.ns, 0, C.byref(k), None) == H.ERR_ARG_NULL and g(M.ns, 3, C.byref(k), C.byref(B)) == H.ERR_ARG_OUTOFRANGE
        assert f(M.ns, 0, 0.5, 1e-3) == 0 and f(M.ns, 0, 0.0, 1e-3) == 0
    finally:
        M.close()


def _two_ranks(R, ranks):
    M = sh.Mirror(cavity_case(), ORACLE_OPTS + ("-ns_scalar_implicit_theta", 1.0), R, ranks)
    try:
        add_scalars(M, [dict(name="t", gamma=0.1, start=cavity_start()[0])], None)
        f = M.H.lib.NSSetScalarImplicit
        rcs = (f(M.ns, 0, 1.0, 1e-6), f(M.ns, 0, 0.5, 1e-6), f(M.ns, 0, 0.0, 1e-6))
        M.step()            # the option does not reach a scalar of a several-rank mesh: the explicit, collective step runs
        k, B = C.c_int(-1), C.c_double(-1.0)
        assert M.H.lib.NSGetScalarImplicitInfo(M.ns, 0, C.byref(k), C.byref(B)) == 0
        return rcs, (k.value, B.value)
    finally:
        M.close()


def test_two_ranks_are_not_supported(H):
    for rcs, info in inproc.run_threads(2, _two_ranks, (2, 1, 1)):
        assert rcs == (H.ERR_SUP, H.ERR_SUP, 0) and info == (0, 1.0)
