"""fl_scalar_rhs, fl_scalar_cfl, fl_scalar_stats and the handle's errors on the GPU against tests/scalar_reference.py.

The bound on every cell of R is DERIVED, not fitted: scalar_reference.rhs evaluates the scheme in long double (the exact value, for this purpose)
and follows one unit roundoff per rounded operation through the formula -- the cell's sum of absolute flux and gradient terms, the limiter's
Lipschitz constant times the error of the gradient ratio, the limiter's own operation count (scalar_cases.rhs_slack).  Shapes: the smallest at
which the kernel can go wrong -- 4^3 (the periodic images of +-2 overlap), 7 x 5 x 6, 66 x 9 x 5 and 130 x 6 x 7 (an x line crosses the 64-lane
segment with a ragged tail), and scalar_cases.REGIME_GRID, which takes the launch plan of 512^3."""
import ctypes as C

import numpy as np
import pytest

from tests import scalar_cases as sc
from tests import scalar_reference as sr

pytestmark = pytest.mark.gpu

SMALL = (7, 5, 6)
ELSEWHERE = [(4, 4, 4), (66, 9, 5), (130, 6, 7)]
GAMMA = 0.0125


@pytest.fixture(scope="module")
def handles():
    made = {}

    def get(n, uniform, bcname):
        key = (n, uniform, bcname)
        if key not in made:
            made[key] = sc.make_handles(n, uniform, bcname)
        return made[key]
    yield get
    for Pz, S in made.values():
        S.close()
        Pz.close()


def _dev(a):
    from tests.gpu_common import dev
    return dev(np.ascontiguousarray(a).reshape(-1))


def check_rhs(get, n, uniform, bcname, limiter, kinds=sc.PHI_KINDS, variants=((0.0, False), (GAMMA, True))):
    from tests.gpu_common import host
    Pz, S = get(n, uniform, bcname)
    Pr = sc.problem(n, uniform, bcname)
    V = sc.velocity(n, bcname)
    S.set_velocity(*[_dev(v) for v in V])
    S.set_limiter(limiter)
    worst = 0.0
    for gamma, with_source in variants:
        S.set_diffusivity(gamma)
        Pr.gamma = gamma
        q = sc.source(n) if with_source else None
        for kind in kinds:
            phi = sc.phi_field(n, kind)
            got = host(S.rhs(_dev(phi), None if q is None else _dev(q))).reshape(phi.shape)
            want, E, _ = sr.rhs(Pr, phi, V, q, np.longdouble, bounds=True, limiter=limiter)
            err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
            tol = sc.rhs_slack(E)
            worst = max(worst, float((err / tol).max()))
            bad = np.argwhere(err > tol)
            assert bad.size == 0, (f"{n} {'uniform' if uniform else 'stretched'} {bcname} {limiter} gamma={gamma} phi={kind}: {len(bad)} cells beyond the derived bound, "
                                   f"first (k, j, i) = {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, exact {float(want[tuple(bad[0])])!r}, "
                                   f"error {err[tuple(bad[0])]:.3e} > bound {tol[tuple(bad[0])]:.3e}")
    print(f"rhs {n} {'uniform' if uniform else 'stretched'} {bcname} {limiter}: largest error / bound = {worst:.3f}")


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "stretched"])
@pytest.mark.parametrize("bcname", list(sc.BC_SETS))
@pytest.mark.parametrize("limiter", sr.LIMITERS)
def test_rhs_every_limiter(handles, limiter, bcname, uniform):
    check_rhs(handles, SMALL, uniform, bcname, limiter)


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "stretched"])
@pytest.mark.parametrize("bcname", list(sc.BC_SETS))
@pytest.mark.parametrize("n", ELSEWHERE, ids=lambda n: "x".join(map(str, n)))
def test_rhs_shapes(handles, n, bcname, uniform):
    for limiter in ("superbee", "vanleer", "quick"):
        check_rhs(handles, n, uniform, bcname, limiter)


@pytest.mark.parametrize("bcname,limiter", [("channel", "superbee"), ("periodic", "vanleer"), ("dirichlet", "quick")])
def test_rhs_in_the_plan_of_512_cubed(handles, bcname, limiter):
    """the whole grid is evaluated: the reference takes about two seconds on it"""
    from fluca_amd import capi
    out = (C.c_int * 5)()
    f = capi.lib.fldbg_scalar_plan
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    assert f(512, 512, 512, sr.LIMITERS.index(limiter), out, 5) == 5
    big = list(out)
    assert f(*sc.REGIME_GRID, sr.LIMITERS.index(limiter), out, 5) == 5
    assert (out[0], out[3]) == (big[0], big[3]) == (128, 1) and out[4] > 4 * 8 * out[0]     # capped, fixed segments, waves with a second trip
    check_rhs(handles, sc.REGIME_GRID, False, bcname, limiter, kinds=("random", "step"), variants=((GAMMA, True),))


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "stretched"])
@pytest.mark.parametrize("bcname", ["periodic", "channel"])
@pytest.mark.parametrize("n", [SMALL, (66, 9, 5), (40, 33, 37)], ids=lambda n: "x".join(map(str, n)))
def test_cfl_and_stats(handles, n, bcname, uniform):
    """min and max exactly; the sum and the two Courant numbers at rounding level.  The sum's order (fl_scalar.hip): a thread adds its cells, 6
    shuffle levels, 2 levels across the waves, the blocks one after another on the host -- so many roundings on the sum of the magnitudes, and
    three for a term phi hx hy hz.  A Courant number is a maximum of sums of three quotients: 3 roundings in a term, 2 in the sum, 1 for dt
    (and one more product and square for the diffusive one)."""
    Pz, S = handles(n, uniform, bcname)
    Pr = sc.problem(n, uniform, bcname)
    V = sc.velocity(n, bcname)
    S.set_velocity(*[_dev(v) for v in V])
    S.set_diffusivity(GAMMA)
    Pr.gamma = GAMMA
    dt = 0.0123
    got = S.cfl(dt)
    want = sr.cfl(Pr, V, dt, np.longdouble)
    for g, w, ops in zip(got, want, (6, 9)):
        assert abs(g - w) <= ops * sr.U * abs(w) * (1 + 2.0 ** -10), (g, w)
    ncell = n[0] * n[1] * n[2]
    nb = min(1024, -(-ncell // 256))
    depth = -(-ncell // (256 * nb)) + 6 + 2 + nb + 3
    for kind in ("random", "step"):
        phi = sc.phi_field(n, kind)
        mn, mx, sm = S.stats(_dev(phi))
        wmn, wmx, wsm = sr.stats(Pr, phi, np.longdouble)
        assert (mn, mx) == (wmn, wmx)
        mag = float((np.abs(phi) * sr.volumes(Pr)).sum())
        assert abs(sm - wsm) <= depth * sr.U * mag * (1 + 2.0 ** -10), (sm, float(wsm), depth * sr.U * mag)


def test_errors():
    from fluca_amd import capi
    from fluca_amd.poisson import Poisson, default_decomp
    from oracle import fluca_oracle as fo
    lib = capi.lib
    n = (8, 6, 4)
    six = lambda *v: (C.c_int * 6)(*v)
    Pz = Poisson(n, sc.faces(n, True), [fo.BC_VELOCITY] * 4 + [fo.BC_PERIODIC] * 2, 1e-3)
    h = C.c_void_p()
    # periodic flags that disagree with the grid, either way; a kind out of range
    assert lib.fl_scalar_create(Pz.h, six(0, 0, 0, 0, 0, 1), C.byref(h)) == -62 and not h.value
    assert lib.fl_scalar_create(Pz.h, six(2, 2, 0, 0, 2, 2), C.byref(h)) == -62 and not h.value
    assert lib.fl_scalar_create(Pz.h, six(0, 1, 0, 0, 2, 0), C.byref(h)) == -62 and not h.value
    assert lib.fl_scalar_create(Pz.h, six(0, 3, 0, 0, 2, 2), C.byref(h)) == -63 and not h.value
    assert lib.fl_scalar_create(Pz.h, six(0, 1, 1, 0, 2, 2), C.byref(h)) == 0 and h.value
    # nothing runs before a velocity is set
    a, b = Pz.empty(), Pz.empty()
    a.zero_()
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    out = (C.c_double * 3)()
    assert lib.fl_scalar_rhs(h, pa, None, pb) == -73
    assert lib.fl_scalar_step(h, 0.1, 5, None, pa) == -73
    assert lib.fl_scalar_cfl(h, 0.1, out) == -73
    assert lib.fl_scalar_stats(h, pa, out) == 0 and tuple(out) == (0.0, 0.0, 0.0)
    V = [Pz.empty(m).zero_() for m in Pz.nface]
    assert lib.fl_scalar_set_velocity(h, *[C.c_void_p(v.data_ptr()) for v in V]) == 0
    assert lib.fl_scalar_rhs(h, pa, None, pa) == -62               # out must not be phi
    assert lib.fl_scalar_step(h, 0.1, 1, None, pa) == -63
    assert lib.fl_scalar_rhs(h, pa, None, pb) == 0 and lib.fl_scalar_step(h, 0.1, 2, None, pa) == 0
    Pz.synchronize()
    assert lib.fl_scalar_destroy(h) == 0
    Pz.close()
    # a handle on one rank's block of two: not built
    P2 = Poisson(n, sc.faces(n, True), [fo.BC_VELOCITY] * 6, 1e-3, decomp=default_decomp(n, (2, 1, 1), 0))
    assert lib.fl_scalar_create(P2.h, six(0, 0, 0, 0, 0, 0), C.byref(h)) == -56 and not h.value
    P2.close()
