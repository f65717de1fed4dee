"""-m gpu, a 2 x 2 x 2 rank grid in one process (tests/inproc.py): fl_ibm_scalar_force / fl_ibm_scalar_rate on replicated and on owner-rank
markers (fl_ibm_owned_select, gid = list index), the grid and the marker set of tests/ibm_scalar_cases.py -- blocks of 12 x 10 x 8 cells; the sphere
sits where the eight blocks meet, the knot of 260 markers straddles the x face.

Each rank's block of phi and its Q bit for bit against the composition fl_ibm_interp(1) -> fl_vec_lincomb -> fl_ibm_spread(1) on the same rank grid and
set; the gathered phi against the long-double reference and the one-rank run within the derived bound of tests/ibm_scalar_reference.py; the rate the
same on all eight ranks and equal to fl_ibm_force's first components; after one fl_ibm_migrate across a face the bits of a fresh set; voted errors.

One run of the ranks per delta function serves all tests (cached)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ibm_scalar_cases as sc
from tests import ibm_scalar_reference as isr
from tests import inproc
from tests.test_gpu_config5 import Case, _blk, _handle
from tests.test_gpu_ibm_migrate import _fetch, _migrate, _select_create
from tests.test_gpu_ibm_owner import _ptr

pytestmark = pytest.mark.gpu

KINDS = [0, 1]
NPASS = 3
RANKS = (2, 2, 2)


def _case():
    case = Case(n=sc.N, ranks=RANKS, bc=sc.BC, box=sc.BOX)
    assert all(np.array_equal(case.xf[d], sc.grid(True)[d]) for d in range(3))
    return case


def _moved(X):
    """the set 1.1 h further along x: markers cross the x face between the blocks (cell 12)"""
    return [X[0] + 1.1 * sc.H, X[1].copy(), X[2].copy()]


def _calls(torch, capi, P, m, L, phi0b, T, dV, body, fused, by_value):
    """npass passes on this rank's block -> phi block, Q (host); fused: fl_ibm_scalar_force, else the three entry points per pass.
    T, dV, body: device arrays of the L markers this rank hands to the set"""
    lib = capi.lib
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
    phi = dev(phi0b)
    if fused:
        Q = torch.full((L,), np.nan, dtype=torch.float64, device="cuda")
        val = (C.c_double * 3)(*sc.VALUES)
        if by_value:
            capi.check(lib.fl_ibm_scalar_force(m, NPASS, None, _ptr(body), 3, val, _ptr(dV), _ptr(phi), _ptr(Q)), "fl_ibm_scalar_force (value)")
        else:
            capi.check(lib.fl_ibm_scalar_force(m, NPASS, _ptr(T), None, 1, None, _ptr(dV), _ptr(phi), _ptr(Q)), "fl_ibm_scalar_force (target)")
    else:
        Tt = torch.as_tensor(sc.VALUES, device="cuda")[body.long()].contiguous() if by_value else T
        Q = None
        for _ in range(NPASS):
            Phi = torch.full((L,), np.nan, dtype=torch.float64, device="cuda")
            q = torch.full((L,), np.nan, dtype=torch.float64, device="cuda")
            capi.check(lib.fl_ibm_interp(m, 1, _ptr(phi), _ptr(Phi)), "fl_ibm_interp")
            capi.check(lib.fl_vec_lincomb(P.h, L, -1.0, _ptr(Phi), 1.0, _ptr(Tt), _ptr(q)), "fl_vec_lincomb")
            capi.check(lib.fl_ibm_spread(m, 1, _ptr(q), _ptr(dV), _ptr(phi)), "fl_ibm_spread")
            Q = q.clone() if Q is None else Q + q
    torch.cuda.current_stream().synchronize()
    return phi.cpu().numpy(), Q.cpu().numpy()


def _rates(torch, capi, m, L, Q, dV, body):
    """fl_ibm_scalar_rate, and fl_ibm_force's first components for F = (Q, 0, 0)"""
    lib = capi.lib
    rate, about, force = (C.c_double * 3)(), (C.c_double * 9)(), (C.c_double * 9)()
    Qd = torch.as_tensor(Q, device="cuda")
    capi.check(lib.fl_ibm_scalar_rate(m, _ptr(Qd), _ptr(dV), _ptr(body), 3, rate), "fl_ibm_scalar_rate")
    F = torch.cat([Qd, torch.zeros(2 * L, dtype=torch.float64, device="cuda")]).contiguous()
    capi.check(lib.fl_ibm_force(m, _ptr(F), _ptr(dV), _ptr(body), 3, about, force, None), "fl_ibm_force")
    return np.array(list(rate)), np.array(list(force)).reshape(3, 3)[:, 0]


def _worker(R, case, kind):
    import torch
    from fluca_amd import capi
    lib = capi.lib
    P, d, s = _handle(R, case)
    X, data = sc.markers(), sc.data()
    L = X[0].size
    out = {}
    with torch.cuda.stream(s):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        phi0b = _blk(case, d, data["phi0"])
        Tg, dVg, bg = dev(data["T"]), dev(data["dV"]), torch.as_tensor(data["body"], device="cuda")
        Xd = [dev(a) for a in X]
        # replicated markers
        mr = C.c_void_p()
        capi.check(lib.fl_ibm_create(P.h, kind, L, *[_ptr(t) for t in Xd], C.byref(mr)), "fl_ibm_create")
        for by_value in (False, True):
            a = _calls(torch, capi, P, mr, L, phi0b, Tg, dVg, bg, True, by_value)
            b = _calls(torch, capi, P, mr, L, phi0b, Tg, dVg, bg, False, by_value)
            out["rep", by_value] = (a, b)
        out["rep_rates"] = _rates(torch, capi, mr, L, out["rep", True][0][1], dVg, bg)
        lib.fl_ibm_destroy(mr)
        # owner-rank markers
        mo, rc, sel = _select_create(torch, capi, P, kind, Xd)
        assert rc == 0, rc
        n = int(sel.numel())
        Tl, dVl, bl = Tg[sel].contiguous(), dVg[sel].contiguous(), bg[sel].contiguous()
        for by_value in (False, True):
            a = _calls(torch, capi, P, mo, n, phi0b, Tl, dVl, bl, True, by_value)
            b = _calls(torch, capi, P, mo, n, phi0b, Tl, dVl, bl, False, by_value)
            out["own", by_value] = (a, b)
        out["own_rates"] = _rates(torch, capi, mo, n, out["own", True][0][1], dVl, bl)
        out["sel"] = sel.cpu().numpy()
        # voted errors: one rank's bad argument is every rank's error, and the set is as good as before
        phi, Q = dev(phi0b), torch.full((max(n, 1),), np.nan, dtype=torch.float64, device="cuda")
        val = (C.c_double * 3)(*sc.VALUES)
        f = lib.fl_ibm_scalar_force
        out["errors"] = [
            f(mo, 0 if R.rank == 0 else NPASS, _ptr(Tl), None, 1, None, _ptr(dVl), _ptr(phi), _ptr(Q)),
            f(mo, NPASS, _ptr(Tl), _ptr(bl), 3, val if R.rank == 1 else None, _ptr(dVl), _ptr(phi), _ptr(Q)),
            f(mo, NPASS, _ptr(Tl), None, 1, None, _ptr(dVl), None if R.rank == 2 else _ptr(phi), _ptr(Q)),
            lib.fl_ibm_scalar_rate(mo, _ptr(Tl), _ptr(dVl), _ptr(bl), 65 if R.rank == 3 else 3, (C.c_double * 3)()),
        ]
        s.synchronize()
        out["phi_after_errors"] = phi.cpu().numpy()
        out["own_again"] = _calls(torch, capi, P, mo, n, phi0b, Tl, dVl, bl, True, True)
        # one migration across the x face, the attributes (T, dV, body id) travel
        X1 = [dev(a) for a in _moved(X)]
        attr = torch.stack([Tl, dVl, bl.double()]).reshape(-1).contiguous()
        rc, Lnew, moved = _migrate(lib, mo, [t[sel].contiguous() for t in X1], 3, attr)
        assert rc == 0, rc
        _, gid, attr = _fetch(torch, lib, mo, Lnew, 3)
        attr = attr.reshape(3, Lnew)
        Tm, dVm, bm = attr[0].contiguous(), attr[1].contiguous(), attr[2].to(torch.int32).contiguous()
        out["migrated"] = _calls(torch, capi, P, mo, Lnew, phi0b, Tm, dVm, bm, True, True)
        out["moved"] = moved
        lib.fl_ibm_destroy(mo)
        mf, rc, self_ = _select_create(torch, capi, P, kind, X1)
        assert rc == 0, rc
        out["same_owners"] = bool(torch.equal(gid, self_))
        out["fresh"] = _calls(torch, capi, P, mf, int(self_.numel()), phi0b, Tg[self_].contiguous(), dVg[self_].contiguous(), bg[self_].contiguous(), True, True)
        lib.fl_ibm_destroy(mf)
    from tests import mp_common as mpc
    out["block"] = mpc.block(d)
    P.close()
    return out


@functools.lru_cache(maxsize=None)
def _run(kind):
    case = _case()
    return case, inproc.run_threads(8, _worker, case, kind)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("kind", KINDS)
def test_every_rank_has_the_bits_of_the_composition(kind):
    _, res = _run(kind)
    assert sum(r["sel"].size for r in res) == sc.markers()[0].size and all(r["sel"].size > 0 for r in res)
    for rank, r in enumerate(res):
        for key in (("rep", False), ("rep", True), ("own", False), ("own", True)):
            (phi, Q), (phi_c, Q_c) = r[key]
            assert same_bits(phi, phi_c) and same_bits(Q, Q_c), (rank, key)
    assert any(not np.array_equal(r["own", True][0][0], r["own", False][0][0]) for r in res)


def _gather(case, res, key):
    out = np.full(case.shp, np.nan)
    for r in res:
        out[r["block"]] = key(r).reshape(out[r["block"]].shape)
    return out.ravel()


@pytest.mark.parametrize("kind", KINDS)
def test_the_gathered_phi_is_the_one_rank_result_within_the_derived_bound(kind):
    from tests.test_gpu_ibm_scalar import Pool, fused
    case, res = _run(kind)
    d, X = sc.data(), sc.markers()
    geo = isr.Geometry(sc.N, sc.grid(True), sc.PERIODIC, kind, X)
    pool = Pool()
    try:
        one_T, _, _ = fused(pool.markers(True, kind), NPASS, d["dV"], d["phi0"], T=d["T"])
        one_v, _, _ = fused(pool.markers(True, kind), NPASS, d["dV"], d["phi0"], body=d["body"], values=sc.VALUES)
    finally:
        pool.close()
    for by_value, T, one in ((False, d["T"], one_T), (True, d["Tbody"], one_v)):
        phi_r, Q_r, qs, phis = isr.force(geo, T, d["dV"], d["phi0"], NPASS)
        bphi, bQ = isr.bounds(geo, T, d["dV"], qs, phis)
        for name in ("rep", "own"):
            phi = _gather(case, res, lambda r: r[name, by_value][0][0])
            e = float(np.abs(phi.astype(isr.LD) - phi_r).max())
            e1 = float(np.abs(phi - one).max())
            print(f"kind {kind} {name} by_value {by_value}: |phi - ref| {e:.2e}, |phi - one rank| {e1:.2e}, bound {bphi:.2e}")
            assert e <= bphi and e1 <= 2 * bphi
            if name == "own":
                Q = np.full(X[0].size, np.nan)
                for r in res:
                    Q[r["sel"]] = r[name, by_value][0][1]
            else:
                Q = res[0][name, by_value][0][1]
                assert all(same_bits(Q, r[name, by_value][0][1]) for r in res)     # behind the all-reduce every rank holds the same Phi
            assert float(np.abs(Q.astype(isr.LD) - Q_r).max()) <= bQ


@pytest.mark.parametrize("kind", KINDS)
def test_the_rate_is_the_same_on_every_rank_and_fl_ibm_force_s(kind):
    _, res = _run(kind)
    d = sc.data()
    for name in ("rep_rates", "own_rates"):
        rate0 = res[0][name][0]
        assert np.all(np.isfinite(rate0)) and np.all(rate0 != 0.0)
        for r in res:
            assert same_bits(r[name][0], rate0) and same_bits(r[name][1], rate0), name
    # the owned set's sum over the ranks is the split sum of the gathered Q, whatever rank holds which marker
    Q = np.full(d["dV"].size, np.nan)
    for r in res:
        Q[r["sel"]] = r["own", True][0][1]
    assert same_bits(res[0]["own_rates"][0], isr.rate(Q, d["dV"], d["body"], 3))
    assert same_bits(res[0]["rep_rates"][0], isr.rate(res[0]["rep", True][0][1], d["dV"], d["body"], 3))


@pytest.mark.parametrize("kind", KINDS)
def test_after_a_migration_the_bits_of_a_fresh_set(kind):
    _, res = _run(kind)
    assert sum(r["moved"][0] for r in res) == sum(r["moved"][1] for r in res) > 0
    for rank, r in enumerate(res):
        assert r["same_owners"], rank
        assert same_bits(r["migrated"][0], r["fresh"][0]) and same_bits(r["migrated"][1], r["fresh"][1]), rank
    assert any(not np.array_equal(r["migrated"][0], r["own", True][0][0]) for r in res)


@pytest.mark.parametrize("kind", KINDS)
def test_errors_on_the_owned_set_are_voted(kind):
    """npass = 0 on rank 0 only, both target and value on rank 1 only, phi = NULL on rank 2 only, nbody = 65 on rank 3 only: every rank returns the
    error, phi is untouched, and the next call gives the bits from before"""
    case, res = _run(kind)
    d = sc.data()
    for rank, r in enumerate(res):
        assert r["errors"] == [-63, -62, -85, -63], (rank, r["errors"])
        assert same_bits(r["phi_after_errors"], np.ascontiguousarray(d["phi0"].reshape(case.shp)[r["block"]]).ravel())
        assert same_bits(r["own_again"][0], r["own", True][0][0]) and same_bits(r["own_again"][1], r["own", True][0][1]), rank

