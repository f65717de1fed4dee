"""Cases and drivers shared by tests/test_step_rhs.py (CPU) and tests/test_gpu_step_rhs.py (-m gpu): the right-hand side of a CNLinear time step
(NSFormFunction_CNLinear and the v0interp boundary insertion of NSStep_CNLinear, fluca_amd/host/fluca_host.c) against StepOracle.form_function.

Boundary data are polynomials in (t, x): the vectorised evaluation of the oracle and the point-by-point evaluation of the mirror's callbacks then go
through the same IEEE operations in the same order and give the same bits (no transcendental function of x; sin(3 t) is taken of the scalar t by
math.sin on both sides)."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np

V, O, PER, SYM = 1, 2, 3, 4
BOX = [(0.0, 1.0), (0.0, 1.0), (0.0, 0.5)]
RHO, MU, DT = 1.3, 0.02, 2e-3
T0 = 0.011            # the time of a "step 0" case: not zero, so that a wrong time is a wrong value

SIX_WALLS = [V] * 6
SETS = {
    "six_walls": SIX_WALLS,
    "outlet_hi_x": [V, O, SYM, V, PER, PER],
    "outlets_lo_x_hi_z": [O, V, V, SYM, V, O],
}

_rng = np.random.default_rng(20261018)
_COEF = _rng.uniform(0.3, 1.0, (6, 3, 8)) * _rng.choice([-1.0, 1.0], (6, 3, 8))


def wall_velocity(b, t, X):
    """(3, npoints): every component of every wall non-zero, different from wall to wall, varying in all coordinates (hence in both plane
    coordinates of every wall) and in time -- the wall-normal component included (only the right-hand side is compared: no compatibility needed)"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    out = []
    for q in range(3):
        k = _COEF[b, q]
        out.append(k[0] + k[1] * x + k[2] * y + k[3] * z + k[4] * (x * y + y * z + z * x) + 50.0 * t * (k[5] + k[6] * (x + y + z) + k[7] * x * y * z))
    return np.stack(out)


def tangential_wall_velocity(b, t, X):
    """wall_velocity without its wall-normal component: walls that a closed box can satisfy (the recorded cavity steps converge)"""
    out = wall_velocity(b, t, X)
    out[b // 2] = 0.0
    return out


def outlet_pressure(b, t, X):
    """varies in space (both plane coordinates of every boundary) and in time"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return 0.1 * y + 0.2 * z * x + 0.05 * x + (0.1 * (b + 1)) * z * y + math.sin(3.0 * t) * (0.3 + 0.1 * (x + y) + 0.4 * z)


def outlet_pressure_steady(b, t, X):
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return 0.1 * y + 0.2 * z * x + 0.05 * x + (0.1 * (b + 1)) * z * y


def outlet_pressure_half_steady(b, t, X):
    """p(t, x) = 0.1 y + 0.3 sin(3 t) [y > Ly / 2]: steady on the lower half of an x outlet, unsteady on the upper half"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    y = X[:, 1]
    return 0.1 * y + 0.3 * math.sin(3.0 * t) * (y > 0.5 * (BOX[1][0] + BOX[1][1]))


def faces(n, stretched=True):
    if stretched:
        from tests.gpu_common import stretched_faces
        return stretched_faces(n, BOX)
    return [BOX[d][0] + np.arange(n[d] + 1, dtype=np.float64) * ((BOX[d][1] - BOX[d][0]) / n[d]) for d in range(3)]


def make_case(n, bc, stretched=True, pressure=outlet_pressure, velocity=wall_velocity):
    """grid + boundary data; the oracle Grid is made on demand (case.grid())"""
    from oracle import fluca_oracle as fo
    c = SimpleNamespace(n=tuple(n), bc=list(bc), stretched=stretched, xf=faces(n, stretched), velocity=velocity, pressure=pressure)
    if not stretched:     # MeshCartSetUniformCoordinates' centres, bit for bit (lo + (i + 1/2) h, not the mean of the faces)
        c.xc = [BOX[d][0] + (np.arange(n[d], dtype=np.float64) + 0.5) * ((BOX[d][1] - BOX[d][0]) / n[d]) for d in range(3)]
    else:
        c.xc = None
    c.grid = lambda: fo.Grid(c.n, c.xf, c.bc, DT / RHO, c.xc)
    c.oracle = lambda: fo.StepOracle(c.grid(), DT, RHO, MU, velocity=c.velocity, pressure=c.pressure)
    return c


def random_state(g, seed):
    """v, V[3], p, phalf: random, of order one"""
    rng = np.random.default_rng(seed)
    return dict(v=rng.standard_normal(3 * g.ncell), V=[rng.standard_normal(nf) for nf in g.nface], p=rng.standard_normal(g.ncell),
                phalf=rng.standard_normal(g.ncell))


def shapes(g):
    n = g.n
    return (n[2], n[1], n[0]), [(n[2], n[1], g.nf[0]), (n[2], g.nf[1], n[0]), (g.nf[2], n[1], n[0])]


def within(got, want, scale, tol, what):
    """per entry |got - want| <= tol * scale; prints the largest ratio before it asserts"""
    err = np.abs(np.asarray(got) - np.asarray(want))
    bad = err > tol * scale
    worst = float(np.max(err / np.where(scale > 0, scale, 1.0))) if err.size else 0.0
    print(f"{what}: max |got - want| / scale = {worst:.3e} (tol {tol:g}), max |got - want| = {float(err.max()) if err.size else 0.0:.3e}")
    assert not bad.any(), (what, int(bad.sum()), worst, np.flatnonzero(bad)[:8].tolist())


# ------------------------------------------------------------------------------------------------------------------ blocks of a rank

def block_of(a, shape, lo, ln):
    """this rank's block of a global array shaped (k, j, i); ln[d] may be the FACE count of the block along d"""
    a = np.asarray(a).reshape(shape)
    return np.ascontiguousarray(a[lo[2]:lo[2] + ln[2], lo[1]:lo[1] + ln[1], lo[0]:lo[0] + ln[0]]).ravel()


def gather(parts, g):
    """blocks of the ranks (dicts with lo, ln, v, V[3], p) -> global v (3 ncell), V[3], p on the grid of the oracle Grid g (any boundary types)"""
    cs, fs = shapes(g)
    v = np.full((3,) + cs, np.nan)
    p = np.full(cs, np.nan)
    Vg = [np.full(fs[d], np.nan) for d in range(3)]
    for r in parts:
        lo, ln = r["lo"], r["ln"]
        sl = (slice(lo[2], lo[2] + ln[2]), slice(lo[1], lo[1] + ln[1]), slice(lo[0], lo[0] + ln[0]))
        v[(slice(None),) + sl] = r["v"].reshape(3, ln[2], ln[1], ln[0])
        p[sl] = r["p"].reshape(ln[2], ln[1], ln[0])
        for d in range(3):
            f = list(ln)
            f[d] = r["V"][d].size // (ln[(d + 1) % 3] * ln[(d + 2) % 3])
            fsl = [slice(lo[a], lo[a] + f[a]) for a in (2, 1, 0)]
            Vg[d][tuple(fsl)] = r["V"][d].reshape(f[2], f[1], f[0])
    assert not (np.isnan(v).any() or np.isnan(p).any() or any(np.isnan(a).any() for a in Vg)), "the blocks do not tile the grid"
    return v.ravel(), [a.ravel() for a in Vg], p.ravel()


# ------------------------------------------------------------------------------------------------------------------ the C host mirror

CHEAP = ("-ns_ksp_type", "preonly", "-ns_abf_schur_ksp_rtol", 1e-2, "-ns_abf_momentum_ksp_rtol", 1e-2, "-ns_abf_schur_ksp_max_it", 4,
         "-ns_abf_momentum_ksp_max_it", 4)      # the cheapest outer solve: its answer is not under test


class Mirror:
    """One rank's NS of the C host mirror on a case; R: tests.inproc.Rank (None: the undecomposed run)."""

    def __init__(self, case, opts=(), R=None, ranks=(1, 1, 1)):
        from fluca_amd import capi, hostapi as H
        self.H, self.capi, self.case = H, capi, case
        P = C.c_void_p
        n, bc = case.n, case.bc
        rank, size = (0, 1) if R is None else (R.rank, R.size)
        rk = ranks if size > 1 else (1, 1, 1)
        bt = [1 if bc[2 * d] == PER else 0 for d in range(3)]
        self.mesh = P()
        assert H.lib.MeshCartCreate3d(bt[0], bt[1], bt[2], n[0], n[1], n[2], rk[0], rk[1], rk[2], None, None, None, C.byref(self.mesh)) == 0
        assert H.lib.MeshSetRank(self.mesh, rank, size) == 0
        assert H.lib.MeshSetUp(self.mesh) == 0
        if case.stretched:
            self._xf = [np.ascontiguousarray(a, dtype=np.float64) for a in case.xf]
            assert H.lib.MeshCartSetCoordinates(self.mesh, *[a.ctypes.data_as(C.c_void_p) for a in self._xf]) == 0
        else:
            assert H.lib.MeshCartSetUniformCoordinates(self.mesh, BOX[0][0], BOX[0][1], BOX[1][0], BOX[1][1], BOX[2][0], BOX[2][1]) == 0
        self.ns = P()
        assert H.lib.NSCreate(C.byref(self.ns)) == 0 and H.lib.NSSetType(self.ns, b"cnlinear") == 0 and H.lib.NSSetMesh(self.ns, self.mesh) == 0
        assert H.lib.NSSetDensity(self.ns, RHO) == 0 and H.lib.NSSetViscosity(self.ns, MU) == 0
        self.calls = []          # (boundary, t) of every velocity callback
        self._keep = []
        for b in range(6):
            if bc[b] == V:
                cb = H.BCFunc(self._velocity_cb(b))
                self._keep.append(cb)
                cond = H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=cb)
            elif bc[b] == O:
                cb = H.BCFunc(self._pressure_cb(b))
                self._keep.append(cb)
                cond = H.NSBoundaryCondition(type=H.NS_BC_PRESSURE_OUTLET, pressure=cb)
            else:
                cond = H.NSBoundaryCondition(type=H.NS_BC_PERIODIC if bc[b] == PER else H.NS_BC_SYMMETRY)
            assert H.lib.NSSetBoundaryCondition(self.ns, b, cond) == 0
        argc, av = H.argv("-ns_time_step_size", DT, *opts, *CHEAP)          # the first occurrence of an option counts: the caller's
        assert H.lib.NSSetFromOptions(self.ns, argc, av) == 0 and H.lib.NSSetUp(self.ns) == 0
        if R is not None:
            hp = P()
            assert H.lib.NSGetPoisson(self.ns, C.byref(hp)) == 0
            R.attach(hp)
        sz = (C.c_int64 * 4)()
        assert H.lib.NSGetLocalSizes(self.ns, sz) == 0
        self.sz = tuple(sz)
        cc = [C.c_int64() for _ in range(6)]
        assert H.lib.MeshCartGetCorners(self.mesh, *[C.byref(q) for q in cc]) == 0
        self.lo, self.ln = [q.value for q in cc[:3]], [q.value for q in cc[3:]]
        self.fln = []            # the block's extents with the FACE count along d
        for d in range(3):
            f = list(self.ln)
            f[d] = self.sz[1 + d] // (self.ln[(d + 1) % 3] * self.ln[(d + 2) % 3])
            self.fln.append(f)

    def _velocity_cb(self, b):
        def cb(dim, t, x, val, ctx):
            self.calls.append((b, t))
            r = self.case.velocity(b, t, np.array([[x[0], x[1], x[2]]]))
            val[0], val[1], val[2] = r[0, 0], r[1, 0], r[2, 0]
            return 0
        return cb

    def _pressure_cb(self, b):
        def cb(dim, t, x, val, ctx):
            val[0] = self.case.pressure(b, t, np.array([[x[0], x[1], x[2]]]))[0]
            return 0
        return cb

    def _put(self, ptr, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.capi.check(self.capi.lib.fl_memcpy_h2d(0, ptr, a.ctypes.data_as(C.c_void_p), a.size * 8))

    def _get(self, ptr, m):
        out = np.empty(m)
        self.capi.check(self.capi.lib.fl_memcpy_d2h(0, out.ctypes.data_as(C.c_void_p), ptr, m * 8))
        return out

    def _arrays(self):
        P = C.c_void_p
        v, p, Vp, ph = P(), P(), (C.c_void_p * 3)(), P()
        assert self.H.lib.NSGetSolutionArrays(self.ns, C.byref(v), Vp, C.byref(p)) == 0
        assert self.H.lib.NSGetPressureHalfStep(self.ns, C.byref(ph)) == 0
        return v, [C.c_void_p(Vp[d]) for d in range(3)], p, ph

    def put_state(self, g, st):
        """this rank's blocks of the GLOBAL state st (random_state) into the solution arrays and the half-step pressure"""
        cs, fs = shapes(g)
        v, Vp, p, ph = self._arrays()
        N = g.ncell
        self._put(v, np.concatenate([block_of(st["v"][q * N:(q + 1) * N], cs, self.lo, self.ln) for q in range(3)]))
        for d in range(3):
            self._put(Vp[d], block_of(st["V"][d], fs[d], self.lo, self.fln[d]))
        self._put(p, block_of(st["p"], cs, self.lo, self.ln))
        self._put(ph, block_of(st["phalf"], cs, self.lo, self.ln))

    def get_state(self):
        v, Vp, p, ph = self._arrays()
        return dict(lo=self.lo, ln=self.ln, v=self._get(v, 3 * self.sz[0]), V=[self._get(Vp[d], self.sz[1 + d]) for d in range(3)],
                    p=self._get(p, self.sz[0]), phalf=self._get(ph, self.sz[0]))

    def set_time(self, step, t):
        assert self.H.lib.NSSetTimeStep(self.ns, step) == 0 and self.H.lib.NSSetTime(self.ns, t) == 0

    def time(self):
        step, t = C.c_int64(), C.c_double()
        assert self.H.lib.NSGetTimeStep(self.ns, C.byref(step)) == 0 and self.H.lib.NSGetTime(self.ns, C.byref(t)) == 0
        return step.value, t.value

    def step(self):
        assert self.H.lib.NSStep(self.ns) == 0

    def outer_its(self):
        """applications of the preconditioner in the last step's outer solve"""
        its, rn, reason = C.c_int(), C.c_double(), C.c_int()
        assert self.H.lib.NSGetLinearSolveInfo(self.ns, C.byref(its), C.byref(rn), C.byref(reason)) == 0
        return its.value

    def rhs(self):
        """the right-hand side the last NSStep formed: this rank's blocks of r.v, r.V[3], r.p (NSGetSolverVectors)"""
        r = self.H.NSVec()
        assert self.H.lib.NSGetSolverVectors(self.ns, None, C.byref(r)) == 0
        return dict(lo=self.lo, ln=self.ln, v=self._get(C.c_void_p(r.v), 3 * self.sz[0]), V=[self._get(C.c_void_p(r.V[d]), self.sz[1 + d]) for d in range(3)],
                    p=self._get(C.c_void_p(r.p), self.sz[0]))

    def momentum_apply(self, x):
        """fl_momentum_apply on NSGetMomentum's handle: the operator the last step formed from V0, v0interp and v0"""
        m = C.c_void_p()
        assert self.H.lib.NSGetMomentum(self.ns, C.byref(m)) == 0 and m.value
        n = 3 * self.sz[0]
        xd, yd = C.c_void_p(), C.c_void_p()
        self.capi.check(self.capi.lib.fl_malloc(0, n * 8, C.byref(xd)))
        self.capi.check(self.capi.lib.fl_malloc(0, n * 8, C.byref(yd)))
        try:
            self._put(xd, x)
            self.capi.check(self.capi.lib.fl_momentum_apply(m, xd, yd))
            hp = C.c_void_p()
            assert self.H.lib.NSGetPoisson(self.ns, C.byref(hp)) == 0
            self.capi.check(self.capi.lib.fl_poisson_synchronize(hp))
            return self._get(yd, n)
        finally:
            self.capi.lib.fl_free(0, xd)
            self.capi.lib.fl_free(0, yd)

    def close(self):
        self.H.lib.NSDestroy(C.byref(self.ns))
        self.H.lib.MeshDestroy(C.byref(self.mesh))


def oracle_at(case, step, t, st):
    """StepOracle set up as "step number `step` at time t with this phalf" and its form_function on the state st"""
    so = case.oracle()
    so.step, so.t, so.phalf = step, t, st["phalf"]
    momrhs, interprhs, W, scale = so.form_function(st["v"], st["V"], st["p"])
    return so, momrhs, interprhs, W, scale


# ------------------------------------------------------------------------------------------------------------------ recorded steps

def golden_step_cases():
    """The two cases whose StepOracle.step_once outputs are recorded in tests/golden/step_once_steps.npz (tests/golden/gen_step_once_fixtures.py):
    a cavity (five walls and a symmetry plane, uniform) and a channel with an unsteady outlet (stretched), two steps each from a random state."""
    return {"cavity": make_case((6, 5, 4), [V, V, V, V, SYM, V], stretched=False, velocity=tangential_wall_velocity), "outlet": make_case((6, 5, 4), [V, O, V, V, PER, PER], stretched=True)}


def run_golden_steps(name):
    """-> dict of arrays: v, V0..2, p, phalf after each of two steps, its: the outer iteration counts, rnorm"""
    from oracle import fluca_oracle as fo
    case = golden_step_cases()[name]
    so = case.oracle()
    so.krtol, so.ortol = 1e-10, 1e-8
    if O in case.bc:
        so.S_ksp = fo.KSP_BCGS
    st = random_state(so.g, 5)
    v, Vf, p = st["v"], st["V"], st["p"]
    out = {}
    nt = fo.num_threads()
    fo.set_num_threads(1)        # the Krylov solves' sums are deterministic for a GIVEN thread count
    try:
        for k in range(2):
            v, Vf, p, info = so.step_once(v, Vf, p)
            out.update({f"{name}_s{k}_v": v, f"{name}_s{k}_p": p, f"{name}_s{k}_phalf": so.phalf, f"{name}_s{k}_its": np.array([info["outer_its"]]),
                        f"{name}_s{k}_rnorm": np.array([info["rnorm"]])})
            out.update({f"{name}_s{k}_V{d}": Vf[d] for d in range(3)})
    finally:
        fo.set_num_threads(nt)
    return out


def momrhs_scale(so, v0, p, vbc):
    """|v0| + cv |L| |v0| + |kappa G| |p| + |vbc| per entry: the term scale of fl_momentum_rhs (p, vbc may be None)"""
    g = so.g
    cv = 0.5 * so.mu * so.dt / so.rho
    rp, col, val = so.L.arrays()
    s = np.abs(v0) + cv * np.add.reduceat(np.abs(val) * np.abs(v0)[col], rp[:-1])
    if p is not None:
        s = s + np.concatenate([so._along(np.abs(so._line_matrix("G", d)), np.abs(p).reshape(so.cshape), d).ravel() for d in range(3)])
    if vbc is not None:
        s = s + np.abs(vbc)
    return s


# ------------------------------------------------------------------------------------------------------------------ roundings

def two_prod(a, b):
    """a * b = p + e exactly (Veltkamp / Dekker, no fused multiply-add needed)"""
    p = a * b
    c = 134217729.0
    t = c * a
    ah = t - (t - a)
    al = a - ah
    t = c * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fused(a, x, y):
    """fl(a x + y) as a fused multiply-add gives it: the product exactly (two_prod), summed with y in the 64-bit significand of the x87 long
    double and rounded to double -- one rounding, up to the rare double rounding (64 -> 53 bits) that one_ulp_of_any's unit covers"""
    p, e = two_prod(np.float64(a) * np.ones_like(x), x)
    return np.asarray((p.astype(np.longdouble) + e.astype(np.longdouble)) + np.asarray(y, dtype=np.longdouble), dtype=np.float64)


def one_ulp_of_any(got, candidates, what):
    """every entry of got within one unit in the last place of at least one candidate: a*x + y rounded twice or fused, as the compiler chose"""
    ok = np.zeros(got.shape, dtype=bool)
    for c in candidates:
        ok |= np.abs(got - c) <= np.spacing(np.abs(c))
    assert ok.all(), (what, int((~ok).sum()), np.flatnonzero(~ok)[:8].tolist())
