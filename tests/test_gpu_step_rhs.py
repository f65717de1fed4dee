"""-m gpu: the right-hand side of a CNLinear time step at rounding level.

NSFormFunction_CNLinear and the v0interp boundary insertion of NSStep_CNLinear (fluca_amd/host/fluca_host.c) with the small kernels under them
(fl_momentum_rhs, fl_boundary_set_faces / add_faces / add_cells, fl_poisson_gst_bc, fl_vec_lincomb, fl_vec_dot, fl_momentum_face_interp_scaled,
fl_pressure_update) against StepOracle.form_function and numpy: per entry |got - want| <= 2e-13 x the sum of the absolute values of the terms added
into the entry (the operator tolerance of tests/test_gpu_momentum.py, measured against the term scale so that cancellation is not held against
the kernel).  The whole-step parities elsewhere see these pieces through two solves and a 1e-6 norm; tests/test_step_rhs.py pins the oracle's
own coefficients to mathematics.  Cases and the mirror driver: tests/step_rhs.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import fluca_oracle as fo
from tests import inproc
from tests import step_rhs as sr
from tests.gpu_common import dev, host
from tests.test_gpu_momentum import CASES as MOM_CASES, _close, _pair

pytestmark = pytest.mark.gpu

TOL = 2e-13            # _close of tests/test_gpu_momentum.py
V, O, PER, SYM = sr.V, sr.O, sr.PER, sr.SYM

# grid, stretched: planes wider than one 64-thread block row for axes 1 and 2 and ragged in both plane directions; the same for axis 0 with the
# minimum of 3 cells a wall row needs; ny <= 8, where fl_momentum_interp_faces_ends falls back to whole fields; the last once more on a uniform grid
GRIDS = [((70, 9, 6), True), ((5, 67, 3), True), ((9, 6, 7), True), ((9, 6, 7), False)]
# boundary set, options, outlet pressure
VARIANTS = {
    "six_walls": ("six_walls", (), sr.outlet_pressure),
    "six_walls_no_keep": ("six_walls", ("-ns_keep_boundary_values", "false"), sr.outlet_pressure),
    "outlet_hi_x": ("outlet_hi_x", (), sr.outlet_pressure),
    "outlets_lo_x_hi_z": ("outlets_lo_x_hi_z", (), sr.outlet_pressure),
    "outlet_hi_x_steady": ("outlet_hi_x", (), sr.outlet_pressure_steady),       # differs == 0: no w, no fl_momentum_face_interp_scaled
}


def _time_of(step):
    return sr.T0 if step == 0 else step * sr.DT


def _compare(r, momrhs, interprhs, scale, tol, what):
    sr.within(r["v"], momrhs, scale["v"], tol, what + " momrhs")
    for d in range(3):
        sr.within(r["V"][d], interprhs[d], scale["V"][d], tol, what + f" interprhs[{d}]")
    assert not r["p"].any(), what + ": contrhs is exactly zero"


@pytest.mark.parametrize("step", [0, 3])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n,stretched", GRIDS)
def test_assembled_right_hand_side_matches_form_function(n, stretched, variant, step):
    """One NSStep from a random state set up as "step 0 at T0" (p0, outlet pressure at t) or "step 3 at 3 dt" (phalf, outlet pressure at t - dt / 2):
    r.v, r.V[d], r.p of NSGetSolverVectors against form_function on the same inputs, and v0interp through the operator it feeds (fl_momentum_apply
    on NSGetMomentum's handle against the assembled A of V0 and W).  Six non-zero walls take 18 planes of the 7-plane scratch ring: two laps."""
    setname, opts, pressure = VARIANTS[variant]
    case = sr.make_case(n, sr.SETS[setname], stretched, pressure)
    g = case.grid()
    st = sr.random_state(g, 100 + step)
    t = _time_of(step)
    M = sr.Mirror(case, opts)
    try:
        M.put_state(g, st)
        M.set_time(step, t)
        M.step()
        assert M.time() == (step + 1, t + sr.DT)
        r = M.rhs()
        so, momrhs, interprhs, W, scale = sr.oracle_at(case, step, t, st)
        _compare(r, momrhs, interprhs, scale, TOL, f"{n} {variant} step {step}")
        x = np.random.default_rng(7).standard_normal(3 * g.ncell)
        A = g.assemble_momentum(1.0, sr.DT, -0.5 * sr.MU * sr.DT / sr.RHO, st["V"], W)
        _close(M.momentum_apply(x), A.mult(x))
    finally:
        M.close()


@pytest.mark.parametrize("variant", ["six_walls", "outlet_hi_x"])
def test_second_of_two_consecutive_steps_uses_the_kept_planes(variant):
    """Two NSSteps in a row: the second takes the planes the first evaluated at t + dt as its planes at t (the two-slot cache of cnl_eval_velocity)
    and evaluates only t + 2 dt.  Its right-hand side against form_function fed the GPU's own state after step one."""
    setname, opts, pressure = VARIANTS[variant]
    n = (70, 9, 6)
    case = sr.make_case(n, sr.SETS[setname], True, pressure)
    g = case.grid()
    st = sr.random_state(g, 31)
    M = sr.Mirror(case, opts)
    try:
        M.put_state(g, st)
        M.set_time(0, sr.T0)
        M.step()
        t1 = M.time()[1]
        assert M.time()[0] == 1 and t1 == sr.T0 + sr.DT
        st1 = M.get_state()
        assert set(t for _, t in M.calls) == {sr.T0, t1}
        del M.calls[:]
        M.step()
        assert set(t for _, t in M.calls) == {t1 + sr.DT}, "the planes at t were evaluated again"
        r = M.rhs()
        so, momrhs, interprhs, W, scale = sr.oracle_at(case, 1, t1, st1)
        _compare(r, momrhs, interprhs, scale, TOL, f"{variant} second step")
        x = np.random.default_rng(8).standard_normal(3 * g.ncell)
        _close(M.momentum_apply(x), g.assemble_momentum(1.0, sr.DT, -0.5 * sr.MU * sr.DT / sr.RHO, st1["V"], W).mult(x))
    finally:
        M.close()


# ------------------------------------------------------------------------------------------------------------------ several ranks

# an outer Richardson iteration of two applications of the preconditioner: its correction goes through cnl->d_v, the scratch array that
# NSFormFunction_CNLinear uses for w.  The state and the time are then set again and a second NSStep forms the right-hand side with a scratch
# array that is NOT zero any more (whether the cut-off iteration counted as converged or not does not matter).
DIRTY = ("-ns_ksp_type", "richardson", "-ns_ksp_max_it", 2, "-ns_ksp_rtol", 1e-14, "-ns_error_if_step_failed", 0)


def _rank_run(R, case, g, st, ranks, step, t, dirty):
    M = sr.Mirror(case, DIRTY if dirty else (), R, ranks)
    try:
        M.put_state(g, st)
        M.set_time(step, t)
        M.step()
        if dirty:
            assert M.outer_its() >= 2, "no correction went through the scratch array"
            M.put_state(g, st)
            M.set_time(step, t)
            M.step()
        return M.rhs()
    finally:
        M.close()


@pytest.mark.parametrize("setname", ["six_walls", "channel_half_steady_outlet"])
@pytest.mark.parametrize("n,ranks", [((140, 10, 6), (2, 2, 2)), ((12, 134, 6), (1, 2, 2))])
def test_right_hand_side_on_several_ranks(n, ranks, setname):
    """Per-rank planes still wider than 64, every wall touched by only some ranks; with [V, O, V, V, PER, PER] the outlet pressure
    0.1 y + 0.3 sin(3 t) [y > Ly / 2] is steady on the ranks that hold the lower half of the outlet and unsteady on the others: the branch in which
    a rank that found no difference must zero its share of w and join the collective T w (the Rhie-Chow flag of NSFormFunction_CNLinear).
    Gathered r against the undecomposed form_function to 1e-12 x term scale (the figure of tests/test_gpu_config5.py for operators across ranks);
    every rank's r against a one-rank run of the mirror to 4e-15 x term scale: the sums and their order are the same (measured: the same bits).
    The ranks form the right-hand side twice (DIRTY above), the second time with what an outer iteration left in the scratch array of w."""
    bc = sr.SIX_WALLS if setname == "six_walls" else [V, O, V, V, PER, PER]
    case = sr.make_case(n, bc, True, sr.outlet_pressure_half_steady)
    g = case.grid()
    st = sr.random_state(g, 57)
    step, t = 3, _time_of(3)
    size = ranks[0] * ranks[1] * ranks[2]
    parts = inproc.run_threads(size, _rank_run, case, g, st, ranks, step, t, True)
    one = inproc.run_threads(1, lambda R: _rank_run(None, case, g, st, ranks, step, t, False))[0]
    so, momrhs, interprhs, W, scale = sr.oracle_at(case, step, t, st)
    if setname != "six_walls":      # the case is what it claims: both kinds of outlet rank exist
        dp = so._outlet(1, t - 0.5 * sr.DT) - so._outlet(1, t + 0.5 * sr.DT)
        ylo = dp[:, :n[1] // 2]
        assert not ylo.any() and np.abs(dp[:, n[1] // 2:]).min() > 0
    v, Vg, p = sr.gather(parts, g)
    _compare(dict(v=v, V=Vg, p=p), momrhs, interprhs, scale, 1e-12, f"{n} {ranks} {setname} gathered")
    cs, fs = sr.shapes(g)
    N = g.ncell
    for k, r in enumerate(parts):
        lo, ln = r["lo"], r["ln"]
        blk = lambda a: sr.block_of(a, cs, lo, ln)
        want_v = np.concatenate([blk(one["v"][q * N:(q + 1) * N]) for q in range(3)])
        sc_v = np.concatenate([blk(scale["v"][q * N:(q + 1) * N]) for q in range(3)])
        sr.within(r["v"], want_v, sc_v, 4e-15, f"rank {k} momrhs against one rank")
        for d in range(3):
            f = list(ln)
            f[d] = r["V"][d].size // (ln[(d + 1) % 3] * ln[(d + 2) % 3])
            sr.within(r["V"][d], sr.block_of(one["V"][d], fs[d], lo, f), sr.block_of(scale["V"][d], fs[d], lo, f), 4e-15,
                      f"rank {k} interprhs[{d}] against one rank")


# ------------------------------------------------------------------------------------------------------------------ the small kernels

def _handle(n, bc, decomp=None):
    from fluca_amd.poisson import Poisson
    from tests.gpu_common import stretched_faces
    return Poisson(n, stretched_faces(n, sr.BOX), bc, 1e-3, decomp=decomp)


def _raw(P, fn, *args):
    """a C-ABI call on the handle's stream, ordered against torch's"""
    from fluca_amd import capi
    P._pre()
    rc = getattr(capi.lib, fn)(*args)
    P._post()
    torch.cuda.synchronize()
    return rc


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _layer_index(shape, ax, side):
    sl = [slice(None)] * 3
    sl[2 - ax] = -1 if side else 0
    return tuple(sl)


def _sentinel(m):
    """distinct, non-trivial values: an entry written by mistake, or moved, shows"""
    return 1000.0 + np.arange(m, dtype=np.float64) * 0.37


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("b", range(6))
@pytest.mark.parametrize("n", [(70, 9, 6), (5, 67, 3)])
def test_boundary_kernels_write_their_layer_and_nothing_else(n, b):
    """fl_boundary_set_faces / add_faces / add_cells and fl_poisson_gst_bc on every boundary of grids whose planes are wider than the 64 x 4 thread
    block in one direction and ragged in both: the layer holds coeff * plane bit for bit (set) or to one unit in the last place (add: the
    multiply-add may be fused), every other entry of the target keeps its sentinel bit for bit."""
    P = _handle(n, [O] * 6)
    ax, side = b // 2, b % 2
    shp_c = (n[2], n[1], n[0])
    shp_f = tuple(s + (1 if 2 - ax == i else 0) for i, s in enumerate(shp_c))
    pshape = tuple(s for i, s in enumerate(shp_c) if i != 2 - ax)
    rng = np.random.default_rng(40 + b)
    plane = rng.standard_normal(pshape)
    coeff = -1.37
    pd = dev(plane.ravel())
    lay = None
    for fn, shp in (("fl_boundary_set_faces", shp_f), ("fl_boundary_add_faces", shp_f), ("fl_boundary_add_cells", shp_c)):
        before = _sentinel(int(np.prod(shp))).reshape(shp)
        td = dev(before.ravel())
        assert _raw(P, fn, P.h, b, coeff, _ptr(pd), _ptr(td)) == 0
        after = host(td).reshape(shp)
        lay = _layer_index(shp, ax, side)
        if fn == "fl_boundary_set_faces":
            assert np.array_equal(_bits(after[lay]), _bits(coeff * plane)), fn
        else:
            sr.one_ulp_of_any(after[lay], [before[lay] + coeff * plane, sr.fused(coeff, plane, before[lay])], fn)
        rest = after.copy()
        rest[lay] = before[lay]
        assert np.array_equal(_bits(rest), _bits(before)), fn + " wrote outside its layer"
    # fl_poisson_gst_bc: the handle's own coefficient -- read off a plane of ones, compared with the oracle's, then bit for bit on the random plane
    g = fo.Grid(n, P._xf, [O] * 6, 1e-3)
    before = _sentinel(int(np.prod(shp_f))).reshape(shp_f)
    td, ones = dev(before.ravel()), dev(np.ones(plane.size))
    assert _raw(P, "fl_poisson_gst_bc", P.h, b, _ptr(ones), _ptr(td)) == 0
    c = host(td).reshape(shp_f)[lay]
    assert np.all(c == c.flat[0]) and abs(c.flat[0] - g.gst_bc_coeff(ax, side)) <= 4 * np.spacing(abs(c.flat[0]))
    td = dev(before.ravel())
    assert _raw(P, "fl_poisson_gst_bc", P.h, b, _ptr(pd), _ptr(td)) == 0
    after = host(td).reshape(shp_f)
    assert np.array_equal(_bits(after[lay]), _bits(c.flat[0] * plane))
    rest = after.copy()
    rest[lay] = before[lay]
    assert np.array_equal(_bits(rest), _bits(before)), "fl_poisson_gst_bc wrote outside its layer"
    P.close()


def test_boundary_kernels_do_nothing_where_there_is_no_boundary_and_check_their_arguments():
    from fluca_amd import capi
    from tests import mp_common as mpc
    n = (9, 6, 7)
    fns = ("fl_boundary_set_faces", "fl_boundary_add_faces", "fl_boundary_add_cells")
    big = int(np.prod([m + 1 for m in n]))
    before = _sentinel(big)
    plane = dev(np.random.default_rng(3).standard_normal(big))

    def untouched(P, fn, b, *coeff):
        td = dev(before)
        assert _raw(P, fn, P.h, b, *coeff, _ptr(plane), _ptr(td)) == 0, (fn, b)
        assert np.array_equal(_bits(host(td)), _bits(before)), (fn, b)

    # a periodic axis has no boundary; gst_bc acts on outlets only
    P = _handle(n, [PER, PER, V, O, V, V])
    for b in (0, 1):
        for fn in fns:
            untouched(P, fn, b, 2.5)
    for b in (0, 1, 2, 4, 5):
        untouched(P, "fl_poisson_gst_bc", b)
    # argument errors: FL_ERR_ARG_NULL = -85, FL_ERR_ARG_OUTOFRANGE = -63
    td = dev(before)
    for fn in fns:
        assert _raw(P, fn, None, 2, 1.0, _ptr(plane), _ptr(td)) == -85 and _raw(P, fn, P.h, 2, 1.0, None, _ptr(td)) == -85
        assert _raw(P, fn, P.h, 2, 1.0, _ptr(plane), None) == -85
        assert _raw(P, fn, P.h, 6, 1.0, _ptr(plane), _ptr(td)) == -63 and _raw(P, fn, P.h, -1, 1.0, _ptr(plane), _ptr(td)) == -63
    assert _raw(P, "fl_poisson_gst_bc", None, 3, _ptr(plane), _ptr(td)) == -85 and _raw(P, "fl_poisson_gst_bc", P.h, 3, None, _ptr(td)) == -85
    assert _raw(P, "fl_poisson_gst_bc", P.h, 3, _ptr(plane), None) == -85
    assert _raw(P, "fl_poisson_gst_bc", P.h, 6, _ptr(plane), _ptr(td)) == -63 and _raw(P, "fl_poisson_gst_bc", P.h, -1, _ptr(plane), _ptr(td)) == -63
    assert np.array_equal(_bits(host(td)), _bits(before))
    P.close()
    # two ranks along x: rank 0 does not touch boundary 1, rank 1 does not touch boundary 0 (the kernels are local: no wire is needed)
    for rank, b in ((0, 1), (1, 0)):
        P = _handle((12, 6, 7), [O, O, V, V, V, V], decomp=mpc.decomp_of(capi, (12, 6, 7), (2, 1, 1), rank))
        for fn in fns:
            untouched(P, fn, b, 2.5)
        untouched(P, "fl_poisson_gst_bc", b)
        P.close()


LENGTHS = [1, 255, 257, 8192 * 256 + 77]      # one thread, a ragged block, two blocks, the grid-stride loop of 8192 blocks run twice


@pytest.fixture(scope="module")
def small_handle():
    P = _handle((9, 6, 7), [V] * 6)
    yield P
    P.close()


@pytest.mark.parametrize("n", LENGTHS)
def test_vec_lincomb(small_handle, n):
    P = small_handle
    rng = np.random.default_rng(n)
    x, z = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
    xd, zd = dev(x), dev(z)
    lin = lambda a, xx, b, zz, yy: _raw(P, "fl_vec_lincomb", P.h, n, a, _ptr(xx), b, _ptr(zz), _ptr(yy))
    # coefficients whose products are exact leave ONE rounding, fused or not: bit for bit (signs mixed: the residual's r = f - J x is such a call)
    for a, b in ((-1.0, 1.0), (1.0, 1.0), (2.0, -1.0), (1.0, 0.0)):
        yd = dev(np.full(n, np.nan))
        assert lin(a, xd, b, zd, yd) == 0
        assert np.array_equal(_bits(host(yd)), _bits(a * x + b * z)), (a, b)
    # general coefficients on positive data (no cancellation between the two products): one unit in the last place, whichever product was fused
    a, b = 1.7, 0.6
    yd = dev(np.full(n, np.nan))
    assert lin(a, xd, b, zd, yd) == 0
    sr.one_ulp_of_any(host(yd), [a * x + b * z, sr.fused(a, x, b * z), sr.fused(b, z, a * x)], "a x + b z")
    # y aliasing x
    yd = dev(x)
    assert lin(a, yd, b, zd, yd) == 0
    sr.one_ulp_of_any(host(yd), [a * x + b * z, sr.fused(a, x, b * z), sr.fused(b, z, a * x)], "y aliasing x")
    # z = NULL
    yd = dev(np.full(n, np.nan))
    assert lin(a, xd, 5.0, None, yd) == 0
    assert np.array_equal(_bits(host(yd)), _bits(a * x))
    # a = 0 with NaN in x: x is not part of the sum
    xn = x.copy()
    xn[::3] = np.nan
    yd = dev(np.full(n, np.nan))
    assert lin(0.0, dev(xn), b, zd, yd) == 0
    assert np.array_equal(_bits(host(yd)), _bits(b * z))
    # a = b = 0: exact (positive) zeros, whatever x and z hold
    yd = dev(np.full(n, np.nan))
    assert lin(0.0, dev(xn), 0.0, dev(xn), yd) == 0
    assert np.array_equal(_bits(host(yd)), np.zeros(n, dtype=np.int64))
    assert lin(1.0, None, 1.0, zd, yd) == -85 and lin(1.0, xd, 1.0, zd, None) == -85 and _raw(P, "fl_vec_lincomb", None, n, 1.0, _ptr(xd), 1.0, _ptr(zd), _ptr(yd)) == -85


@pytest.mark.parametrize("n", LENGTHS)
def test_vec_dot(small_handle, n):
    """against math.fsum of the exact products (each product split into two doubles by two_prod).  Bound n 2^-53 sum |x_i y_i|: any order of a
    recursive or blocked summation of n rounded products stays inside it; a dropped tail, thread or block does not."""
    P = small_handle
    rng = np.random.default_rng(n + 1)
    x, y = rng.standard_normal(n), rng.standard_normal(n)

    def check(x, y, what):
        p, e = sr.two_prod(x, y)
        exact = math.fsum(np.concatenate([p, e]))
        out = C.c_double(np.nan)
        assert _raw(P, "fl_vec_dot", P.h, n, _ptr(dev(x)), _ptr(dev(y)), C.byref(out)) == 0
        bound = n * 2.0 ** -53 * float(np.abs(p).sum())
        print(f"fl_vec_dot n = {n} {what}: |got - exact| = {abs(out.value - exact):.3e}, bound {bound:.3e}")
        assert abs(out.value - exact) <= bound, (what, out.value, exact)

    check(x, y, "random")
    last = np.zeros(n)
    last[-1] = 1.25
    check(last, np.full(n, 3.0), "only the last entry")
    check(np.full(n, 0.1), np.full(n, 0.1), "every entry counts the same")
    out = C.c_double()
    xd = dev(x)
    assert _raw(P, "fl_vec_dot", P.h, n, None, _ptr(xd), C.byref(out)) == -85 and _raw(P, "fl_vec_dot", P.h, n, _ptr(xd), _ptr(xd), None) == -85


@pytest.mark.parametrize("n,bc,nonuni", [MOM_CASES[2], MOM_CASES[3], MOM_CASES[5]])
@pytest.mark.parametrize("alpha", [-1.0, 0.37])
def test_face_interp_scaled(n, bc, nonuni, alpha):
    """V_d = rhs_d + alpha (T v)_d with rhs aliasing V (as NSFormFunction calls it, alpha = -1) and with rhs = NULL"""
    P, M, g = _pair(n, bc, nonuni)
    rng = np.random.default_rng(23)
    v = rng.standard_normal(3 * g.ncell)
    rhs = [rng.standard_normal(nf) for nf in g.nface]
    Tv = g.apply_T(v)
    vd = dev(v)
    Vd = [dev(a) for a in rhs]
    ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in Vd])
    assert _raw(P, "fl_momentum_face_interp_scaled", M.h, alpha, _ptr(vd), ptrs, ptrs) == 0
    for d in range(3):
        _close(host(Vd[d]), rhs[d] + alpha * Tv[d])
    Vd = [dev(np.full(nf, np.nan)) for nf in g.nface]
    ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in Vd])
    assert _raw(P, "fl_momentum_face_interp_scaled", M.h, alpha, _ptr(vd), None, ptrs) == 0
    for d in range(3):
        _close(host(Vd[d]), alpha * Tv[d])
    assert _raw(P, "fl_momentum_face_interp_scaled", M.h, alpha, None, None, ptrs) == -85
    M.close()
    P.close()


@pytest.mark.parametrize("n,bc,nonuni", [MOM_CASES[2], MOM_CASES[3], MOM_CASES[5], MOM_CASES[6]])
def test_momentum_rhs(n, bc, nonuni):
    """fl_momentum_rhs = v0 + cv L v0 - kappa G p + vbc from the oracle's operators, per entry to 2e-13 x (|v0| + cv |L| |v0| + |kappa G| |p| + |vbc|);
    p = NULL, vbc = NULL, both, neither; rho <= 0 is refused"""
    P, M, g = _pair(n, bc, nonuni)
    dt, rho, mu = 0.013, 13.0, 0.4             # dt / rho = the handle's kappa (1e-3)
    so = fo.StepOracle(g, dt, rho, mu)
    cv = 0.5 * mu * dt / rho
    rng = np.random.default_rng(29)
    v0, p, vbc = rng.standard_normal(3 * g.ncell), rng.standard_normal(g.ncell), rng.standard_normal(3 * g.ncell)
    base = v0 + cv * so.L.mult(v0)
    Gp = np.concatenate(g.apply_G(p))
    v0d, pd, vbcd = dev(v0), dev(p), dev(vbc)
    for pp, bb in ((None, None), (p, None), (None, vbc), (p, vbc)):
        want = base - (Gp if pp is not None else 0.0) + (bb if bb is not None else 0.0)
        out = dev(np.full(3 * g.ncell, np.nan))
        assert _raw(P, "fl_momentum_rhs", M.h, dt, rho, mu, _ptr(v0d), _ptr(pd if pp is not None else None), _ptr(vbcd if bb is not None else None), _ptr(out)) == 0
        sr.within(host(out), want, sr.momrhs_scale(so, v0, pp, bb), TOL, f"fl_momentum_rhs {n} p {pp is not None} vbc {bb is not None}")
    out = dev(np.zeros(3 * g.ncell))
    for bad in (0.0, -1.0):
        assert _raw(P, "fl_momentum_rhs", M.h, dt, bad, mu, _ptr(v0d), _ptr(pd), None, _ptr(out)) == -63
    assert _raw(P, "fl_momentum_rhs", M.h, dt, rho, mu, None, _ptr(pd), None, _ptr(out)) == -85
    M.close()
    P.close()


@pytest.mark.parametrize("first", [1, 0])
def test_pressure_update(first):
    """first: p = p0 + 2 dp, phalf = p0 + dp; afterwards p = phalf + 1.5 dp, phalf += dp -- single roundings (2 dp is exact), except 1.5 dp + phalf,
    which may be fused: one unit in the last place of either.  The length is the handle's cell count (the call takes no n), and no axis may be longer
    than 100000 cells, so the prime 8192 * 256 + 77 cannot be had: 131 x 127 x 127 = 2112899 cells, odd, more than twice the 4096 blocks of 256
    threads the kernel is launched with, so that its grid-stride loop runs a third, ragged time.  p0 aliasing nothing, then p0 aliasing p."""
    n = (131, 127, 127)
    P = _handle(n, [V] * 6)
    N = P.ncell
    assert N == 131 * 127 * 127 >= 8192 * 256 + 77
    rng = np.random.default_rng(5 + first)
    dp, p0, ph = rng.standard_normal(N), rng.standard_normal(N), rng.standard_normal(N)
    for alias in (False, True):
        dpd, phd = dev(dp), dev(ph)
        pd = dev(p0) if alias else dev(np.full(N, np.nan))
        p0d = pd if alias else dev(p0)
        assert _raw(P, "fl_pressure_update", P.h, first, _ptr(dpd), _ptr(p0d if first or alias else None), _ptr(phd), _ptr(pd)) == 0
        if first:
            assert np.array_equal(_bits(host(pd)), _bits(2.0 * dp + p0)) and np.array_equal(_bits(host(phd)), _bits(dp + p0)), alias
            if not alias:
                assert np.array_equal(_bits(host(p0d)), _bits(p0))
        else:
            sr.one_ulp_of_any(host(pd), [1.5 * dp + ph, sr.fused(1.5, dp, ph)], "p = phalf + 1.5 dp")
            assert np.array_equal(_bits(host(phd)), _bits(ph + dp)), alias
        assert np.array_equal(_bits(host(dpd)), _bits(dp))
    assert _raw(P, "fl_pressure_update", P.h, 1, _ptr(dpd), None, _ptr(phd), _ptr(pd)) == -85
    P.close()
