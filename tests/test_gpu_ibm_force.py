"""-m gpu: fl_ibm_force (include/fluca_hip.h) -- force and torque on each body as a sum whose bits do not depend on the order of the markers, on
how they are shared out between ranks or on what has migrated -- and its host mirror NSGetImmersedBoundaryForce / NSSetImmersedBoundaryBodies /
NSMonitorImmersedBoundaryForce (include/fluca_host.h).

The reference is tests/ibm_force_reference.py: the terms in numpy with the header's roundings, their exact rational sum, the bound
L 2^(E-61) + 1/2 ulp, and the split sum restated in numpy, whose bits the kernels must give.  Independent of that formula: the moments of the
force field that fl_ibm_spread makes of the same markers."""
import ctypes as C
import functools
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import ibm_force_reference as fr
from tests import inproc

pytestmark = pytest.mark.gpu

V, PER = 1, 3
N32 = (32, 32, 32)
BOX = [(0.0, 1.0)] * 3
PERIOD_Z = (None, None, 1.0)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _dev(a, dtype=np.float64):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype).ravel(), device="cuda")


def _force(lib, m, F, dV, body, nbody, about, want_torque=True, fill=7.0):
    """-> (rc, force (nbody, 3), torque (nbody, 3)); the outputs start as `fill`"""
    n = max(nbody, 1)
    ab = (C.c_double * (3 * n))(*np.asarray(about, dtype=np.float64).ravel()[:3 * n])
    f, t = (C.c_double * (3 * n))(*([fill] * (3 * n))), (C.c_double * (3 * n))(*([fill] * (3 * n)))
    rc = lib.fl_ibm_force(m, _ptr(F), _ptr(dV), _ptr(body), nbody, ab, f, t if want_torque else None)
    return rc, np.array(f).reshape(n, 3), np.array(t).reshape(n, 3)


class _Box:
    """one rank: a 32^3 box, periodic in z (or in all three), on a stream of its own"""

    def __init__(self, bc):
        import torch
        from fluca_amd.poisson import Poisson
        self.P = Poisson.uniform(N32, BOX, bc, 1e-3)
        self.s = torch.cuda.Stream()
        self.P.set_stream(self.s)

    def create(self, X, kind=0):
        """a replicated set of the markers X (3, L); L = 0: an owned set without markers"""
        from fluca_amd import capi
        m = C.c_void_p()
        Xd = [_dev(a) for a in X]
        if X.shape[1]:
            capi.check(capi.lib.fl_ibm_create(self.P.h, kind, X.shape[1], *[_ptr(t) for t in Xd], C.byref(m)), "fl_ibm_create")
        else:
            capi.check(capi.lib.fl_ibm_create_owned(self.P.h, kind, 0, None, None, None, None, C.byref(m)), "fl_ibm_create_owned")
        return m


@pytest.fixture(scope="module")
def zbox():
    import torch
    b = _Box([V, V, V, V, PER, PER])
    with torch.cuda.stream(b.s):
        yield b
    b.P.close()


def _random_markers(L, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.1, 0.9, (3, L))
    X[2] = rng.uniform(-0.3, 1.3, L)                   # across the periodic seam at both ends, unwrapped
    F = rng.standard_normal((3, L)) * np.exp2(rng.integers(-8, 8, (3, L)))
    dV = rng.uniform(0.5, 1.5, L) / 32.0 ** 3
    return X, F, dV


def _check(ref, f, t, what):
    wf, wt = fr.within(ref, "force", f), fr.within(ref, "torque", t)
    print(f"{what}: |force - exact| / bound {wf:.3f}, |torque - exact| / bound {wt:.3f}")
    assert wf <= 1.0 and wt <= 1.0, (what, wf, wt)
    assert np.array_equal(f, ref["force"]), (what, f, ref["force"])
    assert np.array_equal(t, ref["torque"]), (what, t, ref["torque"])


# ------------------------------------------------------------------------------------------------ 1. one rank, the kernel's seams

@pytest.mark.parametrize("L", [0, 1, 63, 64, 65, 255, 256, 257, 16385])
def test_one_rank_gives_the_bits_of_the_numpy_split_sum_in_any_marker_order(zbox, L):
    """Peskin-4 on the 32^3 box, periodic in z.  16385 = one marker more than a full pass of the 64 x 256 lanes the grid is capped at."""
    from fluca_amd import capi
    lib = capi.lib
    X, F, dV = _random_markers(L, 100 + L)
    about = np.array([0.5, 0.4375, 0.25])
    ref = fr.reference(X, F, dV, about[None], PERIOD_Z)
    m = zbox.create(X)
    Fd, dVd = _dev(F), _dev(dV)
    rc, f, t = _force(lib, m, Fd, dVd, None, 1, about)
    assert rc == 0, rc
    _check(ref, f, t, f"L = {L}")
    rc, f2, t2 = _force(lib, m, Fd, dVd, None, 1, about, want_torque=False)
    assert rc == 0 and np.array_equal(f2, f) and np.all(t2 == 7.0)                       # torque = NULL: not written
    lib.fl_ibm_destroy(m)
    if L > 1:
        p = np.random.default_rng(L).permutation(L)
        mp = zbox.create(X[:, p])
        Fp, dVp = _dev(F[:, p]), _dev(dV[p])
        rc, fp, tp = _force(lib, mp, Fp, dVp, None, 1, about)
        lib.fl_ibm_destroy(mp)
        assert rc == 0 and np.array_equal(fp, f) and np.array_equal(tp, t), (fp - f, tp - t)
        plain = (F[:, p] * dV[p]).sum(axis=1)
        print(f"L = {L}: a plain sum of the permuted terms differs from the split sum by {np.abs(plain - f[0]).max():.2e}")
    else:
        assert L == 1 or (np.all(f == 0.0) and np.all(t == 0.0))


# ------------------------------------------------------------------------------------------------ 2. bodies

@pytest.mark.parametrize("nbody", [1, 2, 5, 64])
def test_bodies_with_interleaved_ids_each_within_its_bound(zbox, nbody):
    """300 markers, ids interleaved; with more than one body the last one owns no marker and returns zeros.  An id out of range is the error and
    leaves the outputs as they were."""
    from fluca_amd import capi
    lib = capi.lib
    L = 300
    X, F, dV = _random_markers(L, 7 + nbody)
    ids = np.arange(L) % max(nbody - 1, 1)
    about = np.random.default_rng(nbody).uniform(0.2, 0.8, (nbody, 3))
    ref = fr.reference(X, F, dV, about, PERIOD_Z, body=ids, nbody=nbody)
    m = zbox.create(X)
    Fd, dVd, bd = _dev(F), _dev(dV), _dev(ids, np.int32)
    rc, f, t = _force(lib, m, Fd, dVd, bd, nbody, about)
    assert rc == 0, rc
    _check(ref, f, t, f"nbody = {nbody}")
    if nbody > 1:
        assert np.all(f[-1] == 0.0) and np.all(t[-1] == 0.0) and np.abs(f[:-1]).min() > 0.0
    for bad in (nbody, -1):
        ids2 = ids.copy()
        ids2[L // 2] = bad
        b2 = _dev(ids2, np.int32)
        rc, f2, t2 = _force(lib, m, Fd, dVd, b2, nbody, about)
        assert rc == -63 and np.all(f2 == 7.0) and np.all(t2 == 7.0), (bad, rc)            # FL_ERR_ARG_OUTOFRANGE
    for nb in (0, 65):
        assert _force(lib, m, Fd, dVd, bd, nb, np.zeros(3 * 65))[0] == -63
    assert lib.fl_ibm_force(m, _ptr(Fd), _ptr(dVd), None, 1, None, (C.c_double * 3)(), None) == -85         # about missing
    assert lib.fl_ibm_force(m, None, _ptr(dVd), None, 1, (C.c_double * 3)(), (C.c_double * 3)(), None) == -85
    lib.fl_ibm_destroy(m)


# ------------------------------------------------------------------------------------------------ 3. the periodic seam

def test_a_ring_across_the_periodic_seam_has_the_torque_of_the_ring_at_mid_box(zbox):
    """A ring in the x-z plane around (1/2, 1/2, 0) on a dyadic grid (coordinates are multiples of 2^-10, the period is 1): wrapped into the box,
    left unwrapped, or one period up, every r is the same double as that of the ring moved to mid-box, so every term and the sums are the same bits."""
    from fluca_amd import capi
    lib = capi.lib
    L = 97
    th = 2 * np.pi * (np.arange(L) + 0.5) / L
    q = lambda a: np.round(a * 1024.0) / 1024.0
    ring = np.stack([q(0.5 + 0.25 * np.cos(th)), np.full(L, 0.5), q(0.25 * np.sin(th))])
    assert (ring[2] < 0).sum() > 10 and (ring[2] > 0).sum() > 10
    rng = np.random.default_rng(4)
    F, dV = rng.standard_normal((3, L)), rng.uniform(0.5, 1.5, L)
    Fd, dVd = _dev(F), _dev(dV)

    def run(z, about_z):
        X = ring.copy()
        X[2] = z
        m = zbox.create(X)
        rc, f, t = _force(lib, m, Fd, dVd, None, 1, [0.5, 0.5, about_z])
        lib.fl_ibm_destroy(m)
        assert rc == 0
        return f, t

    f_mid, t_mid = run(ring[2] + 0.5, 0.5)
    ref = fr.reference(np.stack([ring[0], ring[1], ring[2] + 0.5]), F, dV, np.array([[0.5, 0.5, 0.5]]), PERIOD_Z)
    _check(ref, f_mid, t_mid, "ring at mid-box")
    for name, z, az in (("unwrapped", ring[2], 0.0), ("wrapped", ring[2] % 1.0, 0.0), ("one period up", ring[2] + 1.0, 0.0), ("about one period up", ring[2], 1.0)):
        f, t = run(z, az)
        assert np.array_equal(t, t_mid) and np.array_equal(f, f_mid), (name, t - t_mid)
    assert np.abs(t_mid).min() > 0.0


# ------------------------------------------------------------------------------------------------ 4. independent of the formula: the delta function's moments

@pytest.mark.parametrize("kind", [0, 1])
def test_force_and_torque_are_the_moments_of_the_spread_field(kind):
    """Uniform 32^3 periodic grid: F spread into a zero field f.  sum_x f h^3 = force (the delta functions sum to one) and
    sum_x (x - a) x f h^3 = torque (Peskin-4 and Roma-3 both have a vanishing first moment).  Field sums by math.fsum; tolerance 1e-12 sum_l |t_l|:
    spreading adds 64 weights of a few ulp each, about 3e-14 per marker."""
    import torch
    from fluca_amd import capi
    lib = capi.lib
    b = _Box([PER] * 6)
    with torch.cuda.stream(b.s):
        L = 200
        rng = np.random.default_rng(31 + kind)
        X = rng.uniform(0.25, 0.75, (3, L))                                                # supports stay clear of the seams: x - a needs no image
        F, dV = rng.standard_normal((3, L)), rng.uniform(0.5, 1.5, L) / 32.0 ** 3
        about = np.array([0.5, 0.46875, 0.53125])
        m = b.create(X, kind)
        Fd, dVd = _dev(F), _dev(dV)
        fld = torch.zeros(3 * 32 ** 3, dtype=torch.float64, device="cuda")
        capi.check(lib.fl_ibm_spread(m, 3, _ptr(Fd), _ptr(dVd), _ptr(fld)), "fl_ibm_spread")
        rc, f, t = _force(lib, m, Fd, dVd, None, 1, about)
        b.s.synchronize()
        lib.fl_ibm_destroy(m)
        fh = fld.cpu().numpy().reshape(3, 32, 32, 32) / 32.0 ** 3                          # f h^3, [component, k, j, i]
    b.P.close()
    assert rc == 0
    xc = (np.arange(32) + 0.5) / 32.0
    r = [(xc - about[0])[None, None, :], (xc - about[1])[None, :, None], (xc - about[2])[:, None, None]]
    ref = fr.reference(X, F, dV, about[None], (1.0, 1.0, 1.0))
    for c in range(3):
        c1, c2 = (c + 1) % 3, (c + 2) % 3
        mom0 = math.fsum(fh[c].ravel())
        mom1 = math.fsum((r[c1] * fh[c2]).ravel()) - math.fsum((r[c2] * fh[c1]).ravel())
        tolf, tolt = 1e-12 * ref["abs_force"][0, c], 1e-12 * ref["abs_torque"][0, c]
        print(f"kind {kind} component {c}: force {f[0, c]:+.17g} field {mom0:+.17g} (tol {tolf:.1e}); torque {t[0, c]:+.17g} field {mom1:+.17g} (tol {tolt:.1e})")
        assert abs(mom0 - f[0, c]) <= tolf and abs(mom1 - t[0, c]) <= tolt


# ------------------------------------------------------------------------------------------------ 5. the 2 x 2 x 2 in-process rank grid

ABOUT_C5 = np.array([[1.0, 0.75, 0.5], [0.9375, 0.71875, 0.25]])


def _grid_worker(R, case, sets, path, attrs):
    """sets: {name: (X, F, dV, ids)}; every set as a replicated and as an owned set (two bodies).  path: the cloud before and after one move,
    attrs (4, L) = F and dV: an owned set at path[0] migrates to path[1] and is compared with a fresh owned set there."""
    import torch
    from fluca_amd import capi
    from tests.test_gpu_ibm_migrate import _fetch, _migrate, _open, _select_create
    lib = capi.lib
    P, d, s = _open(R, case)
    out = {}
    with torch.cuda.stream(s):
        for name, (X, F, dV, ids) in sets.items():
            L = X[0].size
            Xd, Fd, dVd, bd = [_dev(a) for a in X], _dev(F), _dev(dV), _dev(ids, np.int32)
            mr = C.c_void_p()
            capi.check(lib.fl_ibm_create(P.h, 0, L, *[_ptr(t) for t in Xd], C.byref(mr)), "fl_ibm_create")
            out[name, "replicated"] = _force(lib, mr, Fd, dVd, bd, 2, ABOUT_C5)
            out[name, "replicated, one body"] = _force(lib, mr, Fd, dVd, None, 1, ABOUT_C5[0])
            lib.fl_ibm_destroy(mr)
            mo, rc, sel = _select_create(torch, capi, P, 0, Xd)
            assert rc == 0, rc
            Fl, dVl, bl = Fd.reshape(3, L)[:, sel].contiguous(), dVd[sel].contiguous(), bd[sel].contiguous()
            out[name, "owned"] = _force(lib, mo, Fl, dVl, bl, 2, ABOUT_C5)
            out[name, "owned, one body"] = _force(lib, mo, Fl, dVl, None, 1, ABOUT_C5[0])
            out[name, "count"] = int(sel.numel())
            if name == "face" and R.size > 1:      # the ranks that own markers hand over a bad id / no arrays: everybody's error
                bad = bl.clone()
                if bad.numel():
                    bad[0] = 2
                out["bad id"] = _force(lib, mo, Fl, dVl, bad, 2, ABOUT_C5)
                out["null"] = _force(lib, mo, None, dVl, bl, 2, ABOUT_C5)
            lib.fl_ibm_destroy(mo)
        if path is not None:
            m, rc, gid = _select_create(torch, capi, P, 0, [_dev(a) for a in path[0]])
            assert rc == 0
            attr = _dev(attrs).reshape(4, -1)[:, gid].contiguous().reshape(-1)
            Xl = [_dev(a)[gid].contiguous() for a in path[1]]
            rc, Lnew, moved = _migrate(lib, m, Xl, 4, attr)
            assert rc == 0, rc
            _, gid, attr = _fetch(torch, lib, m, Lnew, 4)
            a4 = attr.reshape(4, Lnew)
            Fm, dVm = a4[:3].contiguous(), a4[3].contiguous()
            out["migrated"] = _force(lib, m, Fm, dVm, None, 1, ABOUT_C5[0])
            out["moved"] = moved
            lib.fl_ibm_destroy(m)
            mf, rc, sel = _select_create(torch, capi, P, 0, [_dev(a) for a in path[1]])
            assert rc == 0
            a4 = _dev(attrs).reshape(4, -1)[:, sel].contiguous()
            Ff, dVf = a4[:3].contiguous(), a4[3].contiguous()
            out["fresh"] = _force(lib, mf, Ff, dVf, None, 1, ABOUT_C5[0])
            lib.fl_ibm_destroy(mf)
        s.synchronize()
    P.close()
    return out


class _C5:
    """the grid of tests/test_gpu_config5.py's "c5_even" (64 x 48 x 32 over 2 x 2 x 2 ranks, z periodic) without its CPU oracle: what _handle / _open read"""

    def __init__(self, ranks):
        from tests.test_gpu_config5 import CASES, _coords
        c = CASES["c5_even"]
        self.n, self.ranks, self.bc, self.box, self.kappa, self.own = c["n"], ranks, c["bc"], c["box"], 1e-3, None
        self.xf = _coords(self.n, self.box, False)


@functools.lru_cache(maxsize=None)
def _run_grid():
    from tests.test_gpu_config5 import _cylinder
    from tests.test_gpu_ibm_owner import _cloud
    case, one = _C5((2, 2, 2)), _C5((1, 1, 1))
    h = 2.0 / 64
    # the cylinder and the face cloud of tests/test_gpu_ibm_owner.py (_markers), the moving cloud of tests/test_gpu_ibm_migrate.py (_moving_cloud)
    markers = {"cylinder": _cylinder(case.box, h), "face": list(_cloud([((1.0, 0.4, 0.25), 100)], h))}
    sets = {}
    for name, X in markers.items():
        X = [np.ascontiguousarray(a) for a in X]
        L = X[0].size
        rng = np.random.default_rng(len(name))
        sets[name] = (X, rng.standard_normal((3, L)), rng.uniform(0.5, 1.5, L) * h ** 3, np.arange(L) % 2)
    X0 = _cloud([((1.0 - 2.2 * h, 0.75 - 2.2 * h, 0.5 - 2.2 * h), 300), ((0.5, 0.4, 2.2 * h), 150)], h, seed=23)
    step = np.zeros_like(X0)
    step[:, :300] = 1.1 * h
    step[2, 300:] = -1.1 * h
    path = [[np.ascontiguousarray(a) for a in X0 + k * step] for k in range(2)]
    Lc = X0.shape[1]
    rng = np.random.default_rng(77)
    attrs = np.concatenate([rng.standard_normal((3, Lc)), rng.uniform(0.5, 1.5, (1, Lc)) * h ** 3])
    res1 = inproc.run_threads(1, _grid_worker, one, sets, path, attrs)[0]
    res8 = inproc.run_threads(8, _grid_worker, case, sets, path, attrs, wire_timeout=30.0)
    return sets, path, attrs, res1, res8


def _same(a, b):
    return a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("name", ["cylinder", "face"])
def test_replicated_owned_and_one_rank_sets_give_the_same_bits_on_all_eight_ranks(name):
    """the cylinder of test_gpu_ibm_owner.py on 64 x 48 x 32 over 2 x 2 x 2 ranks; the face cloud, which six of the eight ranks own no marker of"""
    sets, _, _, res1, res8 = _run_grid()
    X, F, dV, ids = sets[name]
    for nb, tag, body in ((2, "", ids), (1, ", one body", None)):
        ref = fr.reference(np.stack(X), F, dV, ABOUT_C5[:nb], PERIOD_Z, body=body, nbody=nb)
        want = res1[name, "replicated" + tag]
        assert want[0] == 0
        _check(ref, want[1], want[2], f"{name}{tag}, one rank")
        assert _same(res1[name, "owned" + tag], want)
        for rank, r in enumerate(res8):
            assert _same(r[name, "replicated" + tag], want), (rank, "replicated")
            assert _same(r[name, "owned" + tag], want), (rank, "owned")
    counts = [r[name, "count"] for r in res8]
    assert sum(counts) == X[0].size and (min(counts) > 0 if name == "cylinder" else sorted(counts)[:6] == [0] * 6), counts


def test_errors_of_the_ranks_that_own_markers_are_everybodys():
    _, _, _, _, res8 = _run_grid()
    assert [r["bad id"][0] for r in res8] == [-63] * 8 and [r["null"][0] for r in res8] == [-85] * 8
    assert all(np.all(r["bad id"][1] == 7.0) and np.all(r["null"][2] == 7.0) for r in res8)


def test_a_migrated_set_gives_the_bits_of_a_fresh_set():
    """one fl_ibm_migrate of test_gpu_ibm_migrate.py's cloud: owners change across a face, an edge, a corner and the periodic seam"""
    _, path, attrs, res1, res8 = _run_grid()
    moved = np.array([r["moved"] for r in res8])
    assert moved[:, 0].sum() == moved[:, 1].sum() > 0
    ref = fr.reference(np.stack(path[1]), attrs[:3], attrs[3], ABOUT_C5[:1], PERIOD_Z)
    _check(ref, res1["fresh"][1], res1["fresh"][2], "the cloud after the move, one rank")
    assert _same(res1["migrated"], res1["fresh"])
    for rank, r in enumerate(res8):
        assert _same(r["fresh"], res1["fresh"]) and _same(r["migrated"], res1["fresh"]), rank


# ------------------------------------------------------------------------------------------------ 6. non-finite terms

def test_a_non_finite_term_makes_its_group_nan_and_the_call_returns(zbox):
    from fluca_amd import capi
    lib = capi.lib
    L = 130
    X, F, dV = _random_markers(L, 5)
    ids = np.arange(L) % 3
    about = np.tile(X[:, 64], (3, 1))                                                # r of marker 64 (body 1) is zero on every axis
    m = zbox.create(X)
    bd = _dev(ids, np.int32)
    Fn = F.copy()
    Fn[1, 17] = np.nan                                                               # F_y dV, and the torque terms x and z of that marker
    Fd, dVd = _dev(Fn), _dev(dV)
    for body, nb in ((None, 1), (bd, 3)):
        rc, f, t = _force(lib, m, Fd, dVd, body, nb, about)
        assert rc == 0 and np.all(np.isnan(f)) and np.all(np.isnan(t)), (rc, f, t)
    Fi = F.copy()
    Fi[:, 64] = [1e300, -1e300, 1e300]
    dVi = dV.copy()
    dVi[64] = 1e10                                                                   # F dV overflows: an infinite force term; r x F = 0 exactly
    Fd, dVd = _dev(Fi), _dev(dVi)
    with np.errstate(over="ignore"):
        ref = fr.reference(X, Fi, dVi, about, PERIOD_Z, body=ids, nbody=3)
        assert np.isinf(Fi[:, 64] * dVi[64]).all() and np.all(np.isfinite(ref["torque"]))
    rc, f, t = _force(lib, m, Fd, dVd, bd, 3, about)
    assert rc == 0 and np.all(np.isnan(f)) and np.array_equal(t, ref["torque"]), (rc, f, t - ref["torque"])
    assert fr.within(ref, "torque", t) <= 1.0
    lib.fl_ibm_destroy(m)


# ------------------------------------------------------------------------------------------------ 7. through NSStep

N7, D7, RHO7 = 32, 8, 1.25
DT7 = 0.5 / N7


def _step_run(R, distribution, tmpdir):
    """tests/test_gpu_ibm_motion.py's 32^3 channel with the sphere oscillating in y and turning about z.  The initial field is zero, so in step 1
    F = U_target - interp(0) = U_target, the bits of fl_ibm_rigid_pose on every rank grid; step 2 (one rank only) starts from a flow.
    -> the forces and what the test needs to form them again"""
    import torch
    from fluca_amd import capi, hostapi as H
    from tests.flow_parity import sphere_markers
    from tests.test_gpu_ibm_motion import Motion
    P = C.c_void_p
    lib = capi.lib
    n = N7
    rank, size = (0, 1) if R is None else (R.rank, R.size)
    rk = (2, 2, 2) if size > 1 else (1, 1, 1)
    X0, dV = sphere_markers(n, D7)
    L = X0[0].size
    ids = (np.arange(L) % 2).astype(np.int32)
    motion = Motion((0.5, 0.5, 0.5), 1.0 / n, DT7)
    mesh = P()
    assert H.lib.MeshCartCreate3d(0, 0, 1, n, n, n, rk[0], rk[1], rk[2], None, None, None, C.byref(mesh)) == 0
    assert H.lib.MeshSetRank(mesh, rank, size) == 0
    assert H.lib.MeshSetUp(mesh) == 0
    assert H.lib.MeshCartSetUniformCoordinates(mesh, 0., 1., 0., 1., 0., 1.) == 0
    ns = P()
    assert H.lib.NSCreate(C.byref(ns)) == 0 and H.lib.NSSetType(ns, b"cnlinear") == 0 and H.lib.NSSetMesh(ns, mesh) == 0
    assert H.lib.NSSetDensity(ns, RHO7) == 0 and H.lib.NSSetViscosity(ns, 0.01) == 0

    @H.BCFunc
    def inlet(dim, t, x, val, ctx):
        val[0], val[1], val[2] = 4.0 * x[1] * (1.0 - x[1]), 0.0, 0.0
        return 0

    @H.BCFunc
    def zero(dim, t, x, val, ctx):
        val[0] = val[1] = val[2] = 0.0
        return 0

    bcs = [H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=inlet), H.NSBoundaryCondition(type=H.NS_BC_PRESSURE_OUTLET, pressure=zero),
           H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=zero), H.NSBoundaryCondition(type=H.NS_BC_VELOCITY, velocity=zero),
           H.NSBoundaryCondition(type=H.NS_BC_PERIODIC), H.NSBoundaryCondition(type=H.NS_BC_PERIODIC)]
    for b in range(6):
        assert H.lib.NSSetBoundaryCondition(ns, b, bcs[b]) == 0
    path = os.path.join(tmpdir, f"force_{distribution}_{size}.txt")
    argc, av = H.argv("-ns_time_step_size", DT7, "-ns_ksp_rtol", 1e-6, "-ns_abf_schur_ksp_rtol", 1e-8, "-ns_abf_momentum_ksp_rtol", 1e-8,
                      "-ns_ibm_marker_distribution", distribution, "-ns_ibm_force_monitor", path)
    assert H.lib.NSSetFromOptions(ns, argc, av) == 0 and H.lib.NSSetUp(ns) == 0
    hp = P()
    assert H.lib.NSGetPoisson(ns, C.byref(hp)) == 0
    if R is not None:
        R.attach(hp)
    dev = lambda a, dt=np.float64: torch.as_tensor(np.ascontiguousarray(a, dtype=dt).ravel(), device="cuda")
    Xd, dVd, idd = [dev(a) for a in X0], dev(dV), dev(ids, np.int32)
    torch.cuda.synchronize()
    out = dict(path=path)
    f3, t3 = (C.c_double * 6)(*([7.0] * 6)), (C.c_double * 6)(*([7.0] * 6))

    def force(about=None):
        ab = None if about is None else (C.c_double * 6)(*np.asarray(about, dtype=np.float64).ravel())
        f3[:], t3[:] = [7.0] * 6, [7.0] * 6
        rc = H.lib.NSGetImmersedBoundaryForce(ns, ab, f3, t3)
        return rc, np.array(f3).reshape(2, 3), np.array(t3).reshape(2, 3)

    out["no boundary"] = force()[0]
    assert H.lib.NSSetImmersedBoundary(ns, 0, L, *[_ptr(t) for t in Xd], _ptr(dVd), None) == 0
    out["before the first step"] = force()

    def owned():
        m, c5 = P(), (C.c_int64 * 5)()
        assert H.lib.NSGetImmersedBoundary(ns, C.byref(m)) == 0
        return c5[0] if lib.fl_ibm_owned_counts(m, c5) == 0 else -1                           # a replicated set has no such count

    out["owned"] = [owned()]
    fn = motion.callback(H)
    c0 = (C.c_double * 3)(*motion.c0)
    assert H.lib.NSSetImmersedBoundaryMotion(ns, c0, fn, None) == 0
    assert H.lib.NSSetImmersedBoundaryBodies(ns, 2, _ptr(idd)) == 0                           # before the step that migrates markers
    out["step rc"] = [H.lib.NSStep(ns)]
    out["owned"].append(owned())
    assert H.lib.NSMonitor(ns) == 0
    out["two bodies"] = force()
    out["two bodies, about the centre"] = force(np.tile(motion.pose(DT7)[0], (2, 1)))
    out["two bodies, about the origin"] = force(np.zeros((2, 3)))
    one = dev(np.zeros(L), np.int32)
    assert H.lib.NSSetImmersedBoundaryBodies(ns, 1, _ptr(one)) == 0                           # after it: the ids follow the set's own numbers
    out["one body"] = force()
    assert H.lib.NSSetImmersedBoundaryBodies(ns, 2, _ptr(idd)) == 0
    out["two bodies again"] = force()
    if size == 1:
        # the test's own U_target - interp(v0) on the solver's set, step 1 (v0 = 0) and step 2 (v0 = the flow after step 1)
        m = P()
        assert H.lib.NSGetImmersedBoundary(ns, C.byref(m)) == 0
        v, p, Vp = P(), P(), (C.c_void_p * 3)()
        assert H.lib.NSGetSolutionArrays(ns, C.byref(v), Vp, C.byref(p)) == 0
        ncell = n ** 3
        v0 = torch.zeros(3 * ncell, dtype=torch.float64, device="cuda")
        for k in (1, 2):
            if k == 2:
                capi.check(lib.fl_poisson_synchronize(hp))
                host = np.empty(3 * ncell)
                capi.check(lib.fl_memcpy_d2h(0, host.ctypes.data_as(C.c_void_p), v, host.nbytes))
                v0 = dev(host)
                torch.cuda.synchronize()
                out["step rc"].append(H.lib.NSStep(ns))
                assert H.lib.NSMonitor(ns) == 0 and H.lib.NSMonitor(ns) == 0                 # the second call writes nothing
                out["two bodies, step 2"] = force()
            centre, rotvec, vel, om = [(C.c_double * 3)(*a) for a in motion.pose(k * DT7)]
            Ut, U = torch.empty(3 * L, dtype=torch.float64, device="cuda"), torch.empty(3 * L, dtype=torch.float64, device="cuda")
            capi.check(lib.fl_ibm_rigid_pose(hp, L, *[_ptr(t) for t in Xd], c0, centre, rotvec, vel, om, None, None, None, _ptr(Ut)))
            capi.check(lib.fl_ibm_interp(m, 3, _ptr(v0), _ptr(U)))
            capi.check(lib.fl_poisson_synchronize(hp))
            Fh = Ut.cpu().numpy() - U.cpu().numpy()
            Fd = dev(Fh)
            torch.cuda.synchronize()
            rc, f, t = _force(lib, m, Fd, dVd, idd, 2, np.tile(motion.pose(k * DT7)[0], (2, 1)))
            assert rc == 0
            out["own", k] = (f, t, Fh.reshape(3, L), np.abs(U.cpu().numpy()).max())
    capi.check(lib.fl_poisson_synchronize(hp))
    H.lib.NSDestroy(C.byref(ns))
    H.lib.MeshDestroy(C.byref(mesh))
    return out


@functools.lru_cache(maxsize=None)
def _run_steps(distribution, size, tmpdir):
    if size == 1:
        return inproc.run_threads(1, lambda R: _step_run(None, distribution, tmpdir))
    return inproc.run_threads(size, _step_run, distribution, tmpdir, wire_timeout=60.0)


@pytest.fixture(scope="module")
def stepdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("ibm_force"))


def test_nsstep_reports_minus_rho_over_dt_times_the_sums_of_its_own_forcing(stepdir):
    from fluca_amd import hostapi as H
    from tests.flow_parity import sphere_markers
    r = _run_steps("replicated", 1, stepdir)[0]
    assert r["no boundary"] == H.ERR_ARG_WRONGSTATE
    rc, f, t = r["before the first step"]
    assert rc == H.ERR_ARG_WRONGSTATE and np.all(f == 7.0) and np.all(t == 7.0)
    assert r["step rc"] == [0, 0]
    s = -(RHO7 / DT7)
    for k, name in ((1, "two bodies"), (2, "two bodies, step 2")):
        rc, f, t = r[name]
        fo, to, F, umax = r["own", k]
        assert rc == 0 and np.array_equal(f, s * fo) and np.array_equal(t, s * to), (k, f - s * fo, t - s * to)
        assert np.abs(f[:, 1]).min() > 0.0 and np.abs(t[:, 2]).min() > 0.0
        assert (umax == 0.0) if k == 1 else (umax > 1e-3)                                # step 2 interpolates a flow
    # the default point is the motion's centre at the end of the step; the origin gives another torque and the same force
    assert _same(r["two bodies"], r["two bodies, about the centre"]) and _same(r["two bodies"], r["two bodies again"])
    assert np.array_equal(r["two bodies, about the origin"][1], r["two bodies"][1]) and not np.array_equal(r["two bodies, about the origin"][2], r["two bodies"][2])
    # two bodies add up to the one body, to 2 ulp of sum |t| (the exact parts are the same: only the last roundings differ)
    X0, dV = sphere_markers(N7, D7)
    F = r["own", 1][2]
    tf, tt = fr.terms(np.zeros((3, dV.size)), F, dV, np.zeros(3))
    rc1, f1, t1 = r["one body"]
    assert rc1 == 0 and np.all(f1[1] == 7.0)                                             # one body: three numbers written
    f2 = r["two bodies"][1]
    for c in range(3):      # the difference in exact arithmetic: a floating-point sum of the two would add a rounding of its own
        diff = abs(Fraction(float(f2[0, c])) + Fraction(float(f2[1, c])) - Fraction(float(f1[0, c])))
        tol = 2 * Fraction(fr.ulp(abs(s) * math.fsum(np.abs(tf[c]))))
        print(f"component {c}: |f_0 + f_1 - f| = {float(diff):.3e}, 2 ulp(sum |t|) = {float(tol):.3e}")
        assert diff <= tol, (c, float(diff), float(tol))


def test_the_monitor_writes_one_line_per_step_and_body_that_parses_back(stepdir):
    r = _run_steps("replicated", 1, stepdir)[0]
    rows = [line.split() for line in open(r["path"])]
    assert [(int(a[0]), int(a[2])) for a in rows] == [(1, 0), (1, 1), (2, 0), (2, 1)] and all(len(a) == 9 for a in rows)
    assert [float(a[1]) for a in rows] == [DT7, DT7, DT7 + DT7, DT7 + DT7]
    for k, name in ((1, "two bodies"), (2, "two bodies, step 2")):
        for b in range(2):
            got = np.array([float(x) for x in rows[2 * (k - 1) + b][3:]])
            assert np.array_equal(got, np.concatenate([r[name][1][b], r[name][2][b]])), (k, b)


@pytest.mark.parametrize("distribution", ["replicated", "owner"])
def test_eight_ranks_report_the_bits_of_one_rank(stepdir, distribution):
    """step 1 from the zero field: both marker distributions on 2 x 2 x 2 ranks against one rank, bit for bit, on all eight ranks; with owner-rank
    markers the body ids given before the step migrate with the markers, those given after it follow the set's numbers"""
    from tests.flow_parity import sphere_markers
    one = _run_steps("replicated", 1, stepdir)[0]
    res = _run_steps(distribution, 8, stepdir)
    for rank, r in enumerate(res):
        assert r["step rc"] == [0] and r["before the first step"][0] == 73, rank
        for name in ("two bodies", "two bodies, about the centre", "two bodies, about the origin", "two bodies again"):
            assert _same(r[name], one[name]), (rank, name, r[name], one[name])
        assert r["one body"][0] == 0 and np.array_equal(r["one body"][1][0], one["one body"][1][0]) and np.array_equal(r["one body"][2][0], one["one body"][2][0]), rank
    rows = [line.split() for line in open(res[0]["path"])]
    assert [(int(a[0]), int(a[2])) for a in rows] == [(1, 0), (1, 1)]                    # rank 0 alone writes
    counts = np.array([r["owned"] for r in res])
    print(f"{distribution}: markers owned per rank before / after the step {counts[:, 0].tolist()} / {counts[:, 1].tolist()}")
    if distribution == "owner":      # the step has moved markers between ranks: the ids given before it travelled with them
        assert counts[:, 0].sum() == counts[:, 1].sum() == sphere_markers(N7, D7)[0][0].size and np.any(counts[:, 0] != counts[:, 1]), counts
    else:
        assert np.all(counts == -1)
