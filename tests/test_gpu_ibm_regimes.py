"""-m gpu: the immersed-boundary kernels on the marker sets of tests/ibm_regimes.py -- bins of several LDS chunks, tile scans of several rounds,
marker counts that leave wavefronts idle, moved markers, markers on the lattice, beyond walls and beyond the ends of a periodic axis.

Every set, both delta functions: interp / spread against the oracle with the tolerances of tests/test_gpu_ibm.py, against the long-double
reference of tests/ibm_reference.py with the derived bound of tests/test_ibm_regimes.py (a leg that does not depend on the oracle), the
invariants, the bits (spreading twice, a second handle, an update away and back), fl_ibm_update against a handle created at the new positions,
and dense_face on two ranks in one process (owner-rank markers, tests/test_gpu_ibm_owner.py's helpers).

Measured on an MI355X against the long-double reference, over all sets: interp at most 130 u max|u| (dense_shell, Roma; the bound there is
16030), spread at most 0.33 of its bound.

One fl_poisson handle and one oracle grid per (grid, boundary types), one marker handle per (set, boundary types, delta function), for the
whole module."""
import ctypes as C

import numpy as np
import pytest

from oracle import fluca_oracle as fo
from tests import ibm_reference as ref
from tests import ibm_regimes as R
from tests.test_ibm_regimes import data, interp_excess, spread_excess

pytestmark = pytest.mark.gpu

KINDS = [0, 1]
CASES = [(r, bc) for r in R.SINGLE for bc in r.bcs]
IDS = [f"{r.name}-{R.BCNAME[tuple(bc)]}" for r, bc in CASES]


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


class Markers:
    """fl_ibm_create / update / interp / spread on a fluca_amd.Poisson"""

    def __init__(self, P, kind, X):
        from fluca_amd.capi import check, lib
        self.lib, self.check, self.P, self.L = lib, check, P, X[0].size
        self.Xd = [dev(a) for a in X]
        self.h = C.c_void_p()
        P._pre()
        check(lib.fl_ibm_create(P.h, kind, self.L, *[C.c_void_p(t.data_ptr()) for t in self.Xd], C.byref(self.h)), "fl_ibm_create")

    def update(self, X):
        assert X[0].size == self.L
        self.Xd = [dev(a) for a in X]
        self.P._pre()
        self.check(self.lib.fl_ibm_update(self.h, *[C.c_void_p(t.data_ptr()) for t in self.Xd]), "fl_ibm_update")

    def interp(self, u, ncomp):
        import torch
        U = torch.full((ncomp * self.L,), np.nan, dtype=torch.float64, device="cuda")
        self.P._pre()
        self.check(self.lib.fl_ibm_interp(self.h, ncomp, C.c_void_p(u.data_ptr()), C.c_void_p(U.data_ptr())), "fl_ibm_interp")
        self.P._post()
        return host(U).reshape(ncomp, self.L)

    def spread(self, F, dV, f0, ncomp):
        """f0 (3, ncell) on the host -> f (3, ncell): the components beyond ncomp must come back untouched"""
        f = dev(f0)
        Fd, dVd = dev(F[:ncomp]), dev(dV)
        self.P._pre()
        self.check(self.lib.fl_ibm_spread(self.h, ncomp, C.c_void_p(Fd.data_ptr()), C.c_void_p(dVd.data_ptr()), C.c_void_p(f.data_ptr())), "fl_ibm_spread")
        self.P._post()
        return host(f).reshape(f0.shape)

    def close(self):
        if self.h:
            self.lib.fl_ibm_destroy(self.h)
        self.h = None


class Pool:
    def __init__(self):
        self.pairs, self.sets, self.extra = {}, {}, []

    def pair(self, r, bc):
        from fluca_amd.poisson import Poisson
        key = (r.n, tuple(map(bytes, r.xf)), tuple(bc))
        if key not in self.pairs:
            self.pairs[key] = (Poisson(r.n, r.xf, bc, 1e-3), fo.Grid(r.n, r.xf, bc, 1e-3))
        return self.pairs[key]

    def markers(self, r, bc, kind):
        key = (r.name, tuple(bc), kind)
        if key not in self.sets:
            self.sets[key] = Markers(self.pair(r, bc)[0], kind, r.markers())
        return self.sets[key]

    def fresh(self, r, bc, kind, X):
        """a handle of the test's own (closed with the pool)"""
        self.extra.append(Markers(self.pair(r, bc)[0], kind, X))
        return self.extra[-1]

    def close(self):
        for m in self.extra + list(self.sets.values()):
            m.close()
        for P, _ in self.pairs.values():
            P.close()


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    yield p
    p.close()


_ORACLE = {}


def oracle(pool, r, bc, kind, X=None, tag="set"):
    """U (4, L) and f (3, ncell) of the oracle on the set's data (cached per case: the GPU legs share it)"""
    key = (r.name, tuple(bc), kind, tag)
    if key not in _ORACLE:
        g, d = pool.pair(r, bc)[1], data(r)
        X = r.markers() if X is None else X
        u4 = np.concatenate([d["u"], d["f0"][:1]])
        _ORACLE[key] = (g.ibm_interp(kind, X, u4), g.ibm_spread(kind, X, d["dV"], d["F"], d["f0"].copy()))
    return _ORACLE[key]


def close_to_oracle(U, Uo, f, fo_):
    """the tolerances of tests/test_gpu_ibm.py"""
    if U is not None:
        assert np.allclose(U, Uo, rtol=1e-12, atol=1e-13), ("interp", float(np.abs(U - Uo).max()))
    if f is not None:
        assert np.allclose(f, fo_, rtol=1e-12, atol=1e-12 * np.abs(fo_).max()), ("spread", float(np.abs(f - fo_).max()))


# ------------------------------------------------------------------------------------------------ 1. oracle and long-double reference

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("r,bc", CASES, ids=IDS)
def test_interp_and_spread_match_the_oracle_and_the_long_double_reference(r, bc, kind, pool):
    """ncomp = 1, 2, 3 (and 4 for interp) from a random f0; the components beyond ncomp keep f0's bits, and so does every cell no marker reaches"""
    m, d, X = pool.markers(r, bc, kind), data(r), r.markers()
    Uo, fo_ = oracle(pool, r, bc, kind)
    u4 = np.concatenate([d["u"], d["f0"][:1]])
    ud = dev(u4)
    for ncomp in (1, 2, 3, 4):
        U = m.interp(ud, ncomp)
        close_to_oracle(U, Uo[:ncomp], None, None)
        ex, K = interp_excess(r, bc, kind, X, u4[:ncomp], U)
        print(f"{r.name} kind {kind} ncomp {ncomp}: interp {ex:.1f} u max|u| of {K}")
        assert ex <= K, (ncomp, ex, K)
    for ncomp in (1, 2, 3):
        f = m.spread(d["F"], d["dV"], d["f0"], ncomp)
        assert np.array_equal(f[ncomp:], d["f0"][ncomp:])
        close_to_oracle(None, None, f[:ncomp], fo_[:ncomp])
        rel, inB, same = spread_excess(r, bc, kind, X, d["dV"], d["F"][:ncomp], d["f0"][:ncomp], f[:ncomp])
        print(f"{r.name} kind {kind} ncomp {ncomp}: spread {rel:.2e} of its bound")
        assert rel <= 1.0 and same, (ncomp, rel, same)


# ------------------------------------------------------------------------------------------------ 2. invariants

INNER = [(r, bc) for r, bc in CASES if r.interior() is not None]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("r,bc", INNER, ids=[f"{r.name}-{R.BCNAME[tuple(bc)]}" for r, bc in INNER])
def test_invariants_on_the_interior_markers(r, bc, kind, pool):
    """sum of the weights = 1, <interp u, F dV> = sum_i u_i f_i V_i, sum_i f_i V_i = sum F dV, with the thresholds of tests/test_gpu_ibm.py; the markers
    that a wall clips are left out, as there"""
    m, d = pool.markers(r, bc, kind), data(r)
    inner = r.interior()
    ncell = r.n[0] * r.n[1] * r.n[2]
    one = m.interp(dev(np.ones(ncell)), 1)[0]
    assert np.allclose(one[inner], 1.0, rtol=0, atol=1e-13), float(np.abs(one[inner] - 1.0).max())
    vol = np.einsum("k,j,i->kji", *[np.diff(r.xf[a]) for a in (2, 1, 0)]).ravel()
    Fi = np.zeros_like(d["F"])
    Fi[:, inner] = d["F"][:, inner]
    U = m.interp(dev(d["u"]), 3)
    fz = m.spread(Fi, d["dV"], np.zeros((3, ncell)), 3)
    lhs, rhs = (U * Fi * d["dV"]).sum(), (d["u"] * fz * vol).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0), (lhs, rhs)
    assert np.allclose((fz * vol).sum(axis=1), (Fi * d["dV"]).sum(axis=1), rtol=1e-12, atol=1e-15)


# ------------------------------------------------------------------------------------------------ 3. bits

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("r,bc", CASES, ids=IDS)
def test_the_bits_do_not_depend_on_the_run(r, bc, kind, pool):
    """Spreading twice; a second handle from the same markers (the binning atomics hand out other slots: the sort hides it, over several chunks too);
    a handle moved to other positions and back."""
    m, d, X = pool.markers(r, bc, kind), data(r), r.markers()
    ud = dev(d["u"])
    U, f = m.interp(ud, 3), m.spread(d["F"], d["dV"], d["f0"], 3)
    assert np.array_equal(f, m.spread(d["F"], d["dV"], d["f0"], 3))
    m2 = pool.fresh(r, bc, kind, X)
    assert np.array_equal(U, m2.interp(ud, 3)) and np.array_equal(f, m2.spread(d["F"], d["dV"], d["f0"], 3))
    rng = np.random.default_rng(31)
    other = [rng.permutation(a) for a in X]                      # every coordinate shuffled on its own: other bins, other counts
    m2.update(other)
    assert not np.array_equal(f, m2.spread(d["F"], d["dV"], d["f0"], 3)) or r.name == "stray_1"
    m2.update(X)
    assert np.array_equal(U, m2.interp(ud, 3)) and np.array_equal(f, m2.spread(d["F"], d["dV"], d["f0"], 3))
    m2.close()


# ------------------------------------------------------------------------------------------------ 4. moved markers

def _moved(r, X):
    """a rigid motion: rotation by 0.05 rad about the axis (1, 2, 3) through the centre of the box, then a shift by (2.3, -1.7, 9.1) h"""
    h = np.array([(r.xf[d][-1] - r.xf[d][0]) / r.n[d] for d in range(3)])
    c = np.array([0.5 * (r.xf[d][-1] + r.xf[d][0]) for d in range(3)])
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Rm = np.eye(3) + np.sin(0.05) * Kx + (1 - np.cos(0.05)) * Kx @ Kx
    Y = Rm @ (np.stack(X) - c[:, None]) + c[:, None] + (np.array([2.3, -1.7, 9.1]) * h)[:, None]
    return [np.ascontiguousarray(a) for a in Y]


# a box (cell-index units) that neither the set nor its moved image touches, to squeeze all markers into
FAR = {"dense_shell": ((222.0, 258.0), (168.0, 195.0), (6.0, 40.0)), "dense_stretched": ((20.0, 30.0), (34.5, 37.5), (1.0, 4.0))}
MOVES = [(R.DENSE_SHELL, R.WALLS), (R.DENSE_SHELL, R.XZPER), (R.SCAN_RAGGED, R.XZPER), (R.DENSE_STRETCHED, R.ZPER), (R.LATTICE, R.XZPER)]


def _far(r, X):
    lo_hi = FAR[r.name]
    out = []
    for d in range(3):
        t = (X[d] - X[d].min()) / (X[d].max() - X[d].min())
        s = lo_hi[d][0] + t * (lo_hi[d][1] - lo_hi[d][0])
        xc = 0.5 * (r.xf[d][1:] + r.xf[d][:-1])
        out.append(np.interp(s, np.arange(r.n[d]), xc))         # index -> position through the centres (any axis)
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("r,bc", MOVES, ids=[f"{r.name}-{R.BCNAME[tuple(bc)]}" for r, bc in MOVES])
def test_update_to_new_positions_equals_a_fresh_handle(r, bc, kind, pool):
    """fl_ibm_update rebuilds weights, counts, offsets, the active list and the sort: U and f equal those of a handle created at the new positions bit
    for bit, and the oracle's there; then on to positions that leave every tile the set ever touched"""
    d, X0 = data(r), r.markers()
    ud = dev(d["u"])
    per = r.periodic(bc)
    m = pool.fresh(r, bc, kind, X0)
    steps = [("moved", _moved(r, X0))] + ([("far", _far(r, X0))] if r.name in FAR else [])
    occupied = ref.bins(r.n, kind, X0, per, r.xf) > 0
    for tag, X1 in steps:
        now = ref.bins(r.n, kind, X1, per, r.xf) > 0
        assert (now != occupied).any()                          # bins empty and fill
        if tag == "far":
            assert not (now & occupied).any()                   # every old tile is left
        occupied |= now
        m.update(X1)
        U, f = m.interp(ud, 3), m.spread(d["F"], d["dV"], d["f0"], 3)
        mf = pool.fresh(r, bc, kind, X1)
        assert np.array_equal(U, mf.interp(ud, 3)), tag
        assert np.array_equal(f, mf.spread(d["F"], d["dV"], d["f0"], 3)), tag
        mf.close()
        Uo, fo_ = oracle(pool, r, bc, kind, X1, tag)
        close_to_oracle(U, Uo[:3], f, fo_)
        assert not np.array_equal(f, d["f0"])
    m.close()


# ------------------------------------------------------------------------------------------------ 5. stray markers

@pytest.mark.parametrize("kind", KINDS)
def test_markers_beyond_walls_contribute_nothing(kind, pool):
    """supports wholly beyond each of the six walls, by 3 and by 40 cells (and, with walls everywhere, the markers that the periodic case wraps):
    U = 0 exactly, and f keeps f0's bits wherever no other marker reaches"""
    r = R.STRAY
    g = R.stray_groups(r)
    for bc in r.bcs:
        m, d = pool.markers(r, bc, kind), data(r)
        gone = g["beyond_walls"].reshape(3, 4)[[a for a in range(3) if not r.periodic(bc)[a]]].ravel()
        if bc == R.WALLS:
            gone = np.concatenate([gone, g["one_period"], g["two_periods"], g["far"]])
        U = m.interp(dev(d["u"]), 3)
        assert np.all(U[:, gone] == 0.0) and np.all(U[:, g["inside"]] != 0.0)
        f = m.spread(d["F"], d["dV"], d["f0"], 3)
        keep = np.setdiff1d(np.arange(r.markers()[0].size), gone)
        cells = ref.spread(r.n, r.xf, r.periodic(bc), kind, [a[keep] for a in r.markers()], d["dV"][keep], d["F"][:, keep])[0]
        untouched = np.ones(f.shape[1], dtype=bool)
        untouched[cells] = False
        assert np.array_equal(f[:, untouched], d["f0"][:, untouched]) and not np.array_equal(f, d["f0"])
        # the strays alone: a set without a single tile
        ms = pool.fresh(r, bc, kind, [a[gone] for a in r.markers()])
        assert np.all(ms.interp(dev(d["u"]), 3) == 0.0)
        assert np.array_equal(ms.spread(d["F"][:, gone], d["dV"][gone], d["f0"], 3), d["f0"])
        ms.close()


@pytest.mark.parametrize("group", ["one_period", "two_periods", "far"])
@pytest.mark.parametrize("kind", KINDS)
def test_positions_on_a_periodic_axis_are_taken_modulo_the_period(kind, group, pool):
    """Markers 0.37, 1.62 and 5.3 periods beyond either end of the periodic x and z axes: the oracle's U and f (it wraps with a full modulo), and the
    bits of the same markers shifted back into the box by whole periods -- the box lengths are powers of two, h = 1/16 and the positions multiples
    of 2^-20, so the shift and the index arithmetic are exact."""
    r, bc = R.STRAY, R.XZPER
    idx = R.stray_groups(r)[group]
    X = [a[idx] for a in r.markers()]
    back = [a.copy() for a in X]
    for a in (0, 2):
        span = r.xf[a][-1] - r.xf[a][0]
        back[a] = np.mod(X[a] - r.xf[a][0], span) + r.xf[a][0]
        assert np.all((back[a] - X[a]) / span == np.round((back[a] - X[a]) / span))
    assert any(np.any(np.abs(back[a] - X[a]) > 0) for a in (0, 2))
    d, g = data(r), pool.pair(r, bc)[1]
    F, dV = d["F"][:, idx], d["dV"][idx]
    ms, mb = pool.fresh(r, bc, kind, X), pool.fresh(r, bc, kind, back)
    U, f = ms.interp(dev(d["u"]), 3), ms.spread(F, dV, d["f0"], 3)
    Ub, fb = mb.interp(dev(d["u"]), 3), mb.spread(F, dV, d["f0"], 3)
    ms.close(), mb.close()
    close_to_oracle(U, g.ibm_interp(kind, X, d["u"]), f, g.ibm_spread(kind, X, dV, F, d["f0"].copy()))
    assert np.all(U != 0.0) and not np.array_equal(f, d["f0"])
    assert np.array_equal(U, Ub) and np.array_equal(f, fb)


# ------------------------------------------------------------------------------------------------ 6. two ranks: owner-rank markers

def _case(r):
    from tests.test_gpu_config5 import Case
    box = [(float(r.xf[d][0]), float(r.xf[d][-1])) for d in range(3)]
    case = Case(n=r.n, ranks=(1, 1, 2), bc=r.bcs[-1] if r is R.STRAY else r.bcs[0], box=box)
    assert all(np.array_equal(case.xf[d], r.xf[d]) for d in range(3))
    return case


def _owner_worker(Rk, case, kind, X, num, d, with_gid):
    """One rank of an owner-rank set.  X: the caller's list; num: the caller's marker numbers (a permutation of 0 .. L-1, shuffled against the list
    order); the replicated set of the same rank holds marker number g at list index g, which is the order the owner path must reproduce."""
    import torch
    from fluca_amd import capi
    from tests.test_gpu_config5 import _blk, _handle
    from tests.test_gpu_ibm_owner import _ptr
    lib = capi.lib
    P, dec, s = _handle(Rk, case)
    out = {}
    with torch.cuda.stream(s):
        L = X[0].size
        Xd = [dev(a) for a in X]
        idx = torch.zeros(L, dtype=torch.int64, device="cuda")
        cnt = C.c_int64(-1)
        capi.check(lib.fl_ibm_owned_select(P.h, kind, L, *[_ptr(t) for t in Xd], _ptr(idx), C.byref(cnt)), "fl_ibm_owned_select")
        sel = idx[:cnt.value].clone()
        n = int(sel.numel())
        Xl = [t[sel].contiguous() for t in Xd]
        gid = torch.as_tensor(num, device="cuda")[sel].contiguous()
        m = C.c_void_p()
        capi.check(lib.fl_ibm_create_owned(P.h, kind, n, *[_ptr(t) for t in Xl], _ptr(gid) if with_gid else None, C.byref(m)), "fl_ibm_create_owned")
        c5 = (C.c_int64 * 5)()
        capi.check(lib.fl_ibm_owned_counts(m, c5), "fl_ibm_owned_counts")
        blk3 = lambda a: np.stack([_blk(case, dec, a[c]) for c in range(3)])
        ul, f0b = dev(blk3(d["u"])), blk3(d["f0"])
        Fl, dVl = dev(d["F"]).reshape(3, L)[:, sel].contiguous(), dev(d["dV"])[sel].contiguous()
        res = []
        for again in (False, True):
            if again:       # the same positions once more: routed, binned and sorted anew
                capi.check(lib.fl_ibm_update(m, *[_ptr(t) for t in Xl]), "fl_ibm_update (owned)")
            U, fl = torch.full((3 * n,), np.nan, dtype=torch.float64, device="cuda"), dev(f0b)
            capi.check(lib.fl_ibm_interp(m, 3, _ptr(ul), _ptr(U)), "fl_ibm_interp (owned)")
            capi.check(lib.fl_ibm_spread(m, 3, _ptr(Fl), _ptr(dVl), _ptr(fl)), "fl_ibm_spread (owned)")
            s.synchronize()
            res.append((U.cpu().numpy().reshape(3, n), fl.cpu().numpy().reshape(3, -1)))
        out.update(sel=sel.cpu().numpy(), counts=list(c5), U=res[0][0], f=res[0][1], same_after_update=bool(np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])))
        lib.fl_ibm_destroy(m)
        # replicated markers on the same rank grid, in the order of the caller's numbers
        inv = np.argsort(num)
        mr = C.c_void_p()
        Xr = [dev(a[inv]) for a in X]
        capi.check(lib.fl_ibm_create(P.h, kind, L, *[_ptr(t) for t in Xr], C.byref(mr)), "fl_ibm_create")
        fr, Fr, dVr = dev(f0b), dev(d["F"][:, inv]), dev(d["dV"][inv])
        capi.check(lib.fl_ibm_spread(mr, 3, _ptr(Fr), _ptr(dVr), _ptr(fr)), "fl_ibm_spread")
        s.synchronize()
        out["f_rep"] = fr.cpu().numpy().reshape(3, -1)
        lib.fl_ibm_destroy(mr)
    out["f_want"] = lambda fglob: blk3(fglob)
    out["lo_len"] = ([int(dec.lo[a]) for a in range(3)], [int(dec.len[a]) for a in range(3)])
    P.close()
    return out


def _two_ranks(r, kind, with_gid):
    from tests import inproc
    case, X, d = _case(r), r.markers(), data(r)
    num = np.random.default_rng(41).permutation(X[0].size).astype(np.int64)
    res = inproc.run_threads(2, _owner_worker, case, kind, X, num, d, with_gid)
    g = case.g
    Uo, fo_ = g.ibm_interp(kind, X, d["u"]), g.ibm_spread(kind, X, d["dV"], d["F"], d["f0"].copy())
    assert sum(x["sel"].size for x in res) == X[0].size
    for rank, x in enumerate(res):
        close_to_oracle(x["U"], Uo[:, x["sel"]], x["f"], x["f_want"](fo_))
        assert x["same_after_update"], rank
    return case, X, res


@pytest.mark.parametrize("kind", KINDS)
def test_dense_face_owner_rank_markers_on_two_ranks(kind):
    """A (1, 1, 2) split whose face cuts a bin of more than 256 own + ghost markers, caller numbers shuffled against the list order: the single-domain
    oracle, the ghost counts of the numpy geometry, and -- with the numbers -- the replicated path's bits, over several chunks of the bin.  Without
    numbers the contract promises the oracle only."""
    from tests.test_gpu_ibm_owner import _geometry
    r = R.DENSE_FACE
    case, X, res = _two_ranks(r, kind, True)
    owner, copies = _geometry(case, kind, X)
    for rank, x in enumerate(res):
        assert np.array_equal(x["sel"], np.nonzero(owner == rank)[0])
        ghosts, sent = sum(1 for _, to, _ in copies if to == rank), sum(1 for l, _, _ in copies if owner[l] == rank)
        assert x["counts"] == [int((owner == rank).sum()), ghosts, sent, 8 * ghosts, 32 * sent], (rank, x["counts"], ghosts, sent)
        assert x["counts"][0] + x["counts"][1] > 256
        fields = ref.regime_fields(r.n, kind, X, r.periodic(case.bc), r.xf, block=x["lo_len"])
        assert fields["max_bin"] > 256 and x["counts"][1] > 0, (rank, fields["max_bin"])
        assert np.array_equal(x["f"], x["f_rep"]), (rank, float(np.abs(x["f"] - x["f_rep"]).max()))
    _two_ranks(r, kind, False)


@pytest.mark.parametrize("kind", KINDS)
def test_owner_rank_markers_beyond_a_periodic_end_on_two_ranks(kind):
    """the stray set with x and z periodic, z split over two ranks: every marker has an owner (k_ibm_route wraps with a full modulo) and is
    interpolated and spread as the single-domain oracle does, however many periods out it lies"""
    case, X, res = _two_ranks(R.STRAY, kind, True)
    assert all(x["counts"][0] > 0 for x in res)
