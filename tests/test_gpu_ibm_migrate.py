"""-m gpu: owner-rank IBM markers that change rank (fl_ibm_migrate / fl_ibm_owned_fetch, include/fluca_hip.h), eight or four host threads over the
in-process wire.

A marker whose owner cell has moved into a neighbouring block travels there with position, number and attributes; afterwards every rank holds its
own markers in ascending number and the set is the one a fresh fl_ibm_owned_select + fl_ibm_create_owned at the new positions makes.  Checked
here: the partition, positions, attributes, moved counts and copy counts after every move against numpy geometry; interp and spread of the
migrated set bit for bit against a fresh set, spread against the replicated path, both against the CPU oracle; the voted errors, after which the
set gives the bits from before the call; the edges of the contract.

One run of the ranks per (scenario, delta function) serves several tests (cached)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import inproc
from tests.test_gpu_config5 import CASES, Case, _blk, _handle
from tests.test_gpu_ibm_owner import _against_oracle, _cloud, _decomps, _geometry, _markers, _ptr, _reference

pytestmark = pytest.mark.gpu

KINDS = [0, 1]
NMOVES = 5
# owner changes per move over 1 / 2 / 3 rank coordinates and the seam crossings among them, from numpy geometry (the owner rule knows no delta function)
TABLE = [([139, 28, 1], 26), ([143, 27, 3], 26), ([145, 18, 3], 29), ([154, 19, 4], 39), ([98, 14, 1], 12)]


# ------------------------------------------------------------------------------------------------ the calls

def _migrate(lib, m, Xl, nattr, attr):
    Lnew, moved = C.c_int64(-1), (C.c_int64 * 2)(-1, -1)
    rc = lib.fl_ibm_migrate(m, *[_ptr(t) for t in Xl], nattr, _ptr(attr) if attr is not None else None, C.byref(Lnew), moved)
    return rc, Lnew.value, list(moved)


def _fetch(torch, lib, m, n, nattr):
    X = [torch.full((n,), np.nan, dtype=torch.float64, device="cuda") for _ in range(3)]
    gid = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    attr = torch.full((nattr * n,), np.nan, dtype=torch.float64, device="cuda")
    rc = lib.fl_ibm_owned_fetch(m, n, *[_ptr(t) for t in X], _ptr(gid), nattr, _ptr(attr))
    assert rc == 0, rc
    return X, gid, attr


def _counts(capi, m):
    c5 = (C.c_int64 * 5)()
    capi.check(capi.lib.fl_ibm_owned_counts(m, c5), "fl_ibm_owned_counts")
    return list(c5)


def _open(R, case):
    """(Poisson, decomposition, stream) of this rank: the wire's handle, or on one rank the whole grid without a communicator"""
    import torch
    from fluca_amd.poisson import Poisson
    if R.size > 1:
        return _handle(R, case)
    P, s = Poisson(case.n, case.xf, case.bc, case.kappa), torch.cuda.Stream()
    P.set_stream(s)
    return P, _decomps(case)[0], s


def _select_create(torch, capi, P, kind, Xd, with_gid=True, order=None):
    """fl_ibm_owned_select on the replicated device arrays Xd, then fl_ibm_create_owned with gid = list index -> (set, rc, sel)"""
    lib = capi.lib
    L = int(Xd[0].numel())
    idx, cnt = torch.zeros(L, dtype=torch.int64, device="cuda"), C.c_int64(-1)
    capi.check(lib.fl_ibm_owned_select(P.h, kind, L, *[_ptr(t) for t in Xd], _ptr(idx), C.byref(cnt)), "fl_ibm_owned_select")
    sel = idx[:cnt.value].clone()
    if order is not None:
        sel = order(sel)
    Xl = [t[sel].contiguous() for t in Xd]
    m = C.c_void_p()
    rc = lib.fl_ibm_create_owned(P.h, kind, int(sel.numel()), *[_ptr(t) for t in Xl], _ptr(sel) if with_gid else None, C.byref(m))
    return m, rc, sel


def _apply(torch, capi, case, d, m, ref, gids, dev):
    """interp of ref's u and spread of ref's F, dV onto ref's f0 with the set m whose own markers are ref's markers `gids`"""
    lib = capi.lib
    L, n = ref["X"][0].size, int(gids.numel())
    blk3 = lambda a: np.stack([_blk(case, d, a[c]) for c in range(3)])
    ul, f0b = dev(blk3(ref["u"])), blk3(ref["f0"])
    U = torch.full((3 * n,), np.nan, dtype=torch.float64, device="cuda")
    Fl, dVl = dev(ref["F"]).reshape(3, L)[:, gids].contiguous(), dev(ref["dV"])[gids].contiguous()
    fl = dev(f0b)
    capi.check(lib.fl_ibm_interp(m, 3, _ptr(ul), _ptr(U)), "fl_ibm_interp")
    capi.check(lib.fl_ibm_spread(m, 3, _ptr(Fl), _ptr(dVl), _ptr(fl)), "fl_ibm_spread")
    torch.cuda.current_stream().synchronize()
    return U.cpu().numpy().reshape(3, n), fl.cpu().numpy().reshape(3, -1), f0b


# ------------------------------------------------------------------------------------------------ 1. faces, edges, corners, the periodic seam

def _moving_cloud():
    case = Case(**CASES["c5_even"])
    h = (case.box[0][1] - case.box[0][0]) / case.n[0]
    X0 = _cloud([((1.0 - 2.2 * h, 0.75 - 2.2 * h, 0.5 - 2.2 * h), 300), ((0.5, 0.4, 2.2 * h), 150)], h, seed=23)
    step = np.zeros_like(X0)
    step[:, :300] = 1.1 * h                   # towards and through the point where the eight blocks meet
    step[2, 300:] = -1.1 * h                  # down through the periodic seam: z becomes negative and is NOT wrapped
    return case, h, [[np.ascontiguousarray(a) for a in X0 + k * step] for k in range(NMOVES + 1)]


def _moves_worker(R, case, path, ref, kind):
    import torch
    from fluca_amd import capi
    lib = capi.lib
    P, d, s = _open(R, case)
    out = dict(moves=[])
    with torch.cuda.stream(s):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        m, rc, gid = _select_create(torch, capi, P, kind, [dev(a) for a in path[0]])
        assert rc == 0, rc
        attr = torch.stack([8.0 * gid.double() + a for a in range(3)]).reshape(-1).contiguous()
        for k in range(1, NMOVES + 1):
            Xd = [dev(a) for a in path[k]]
            Xl = [t[gid].contiguous() for t in Xd]
            rc, Lnew, moved = _migrate(lib, m, Xl, 3, attr)
            assert rc == 0, (k, rc)
            Xf, gid, attr = _fetch(torch, lib, m, Lnew, 3)
            s.synchronize()
            out["moves"].append(dict(gid=gid.cpu().numpy(), X=[t.cpu().numpy() for t in Xf], attr=attr.cpu().numpy().reshape(3, Lnew), moved=moved,
                                     counts=_counts(capi, m)))
        U, f, f0b = _apply(torch, capi, case, d, m, ref, gid, dev)
        out.update(sel=gid.cpu().numpy(), U=U, f=f, f0=f0b, vol=_blk(case, d, ref["vol"]))
        lib.fl_ibm_destroy(m)
        # a set created afresh at the final positions on the same handles, and the replicated one
        Xd = [dev(a) for a in path[NMOVES]]
        mf, rc, self_ = _select_create(torch, capi, P, kind, Xd)
        assert rc == 0, rc
        out["fresh_sel"] = self_.cpu().numpy()
        out["fresh_counts"] = _counts(capi, mf)
        out["U_fresh"], out["f_fresh"], _ = _apply(torch, capi, case, d, mf, ref, self_, dev)
        lib.fl_ibm_destroy(mf)
        L = path[0][0].size
        mr = C.c_void_p()
        capi.check(lib.fl_ibm_create(P.h, kind, L, *[_ptr(t) for t in Xd], C.byref(mr)), "fl_ibm_create")
        Fr, dVr, fr = dev(ref["F"]), dev(ref["dV"]), dev(f0b)
        capi.check(lib.fl_ibm_spread(mr, 3, _ptr(Fr), _ptr(dVr), _ptr(fr)))
        s.synchronize()
        out["f_rep"] = fr.cpu().numpy().reshape(3, -1)
        lib.fl_ibm_destroy(mr)
    P.close()
    return out


@functools.lru_cache(maxsize=None)
def _run_moves(kind):
    case, h, path = _moving_cloud()
    ref = _reference(case, h, path[NMOVES], kind)
    return case, path, ref, inproc.run_threads(8, _moves_worker, case, path, ref, kind)


def _coords(case, rank):
    return np.stack([rank % case.ranks[0], (rank // case.ranks[0]) % case.ranks[1], rank // (case.ranks[0] * case.ranks[1])])


@pytest.mark.parametrize("kind", KINDS)
def test_markers_migrate_across_faces_edges_corners_and_the_periodic_seam(kind):
    """300 markers drift through the point where the eight blocks meet, 150 sink through the periodic seam (z < 0, unwrapped), five moves of 1.1 h.
    After every move: each rank's numbers are the ascending list of the markers it owns by geometry, positions and attributes travelled bit for bit,
    moved[] and fl_ibm_owned_counts are the geometric counts.  Every move changes owners across a face, an edge AND a corner and crosses the seam."""
    case, path, ref, res = _run_moves(kind)
    owner = [_geometry(case, kind, X)[0] for X in path[:1]]
    for k in range(1, NMOVES + 1):
        own, copies = _geometry(case, kind, path[k])
        prev = owner[-1]
        owner.append(own)
        changed = (_coords(case, own) != _coords(case, prev)).sum(axis=0)
        levels = [int((changed == a).sum()) for a in (1, 2, 3)]
        seam = int((own[300:] != prev[300:]).sum())
        print(f"kind {kind} move {k - 1}: owner changes over 1 / 2 / 3 rank coordinates {levels}, seam crossings {seam}")
        assert all(v > 0 for v in levels) and seam > 0, (k, levels, seam)
        assert (levels, seam) == TABLE[k - 1], (k, levels, seam)
        for rank, r in enumerate(res):
            mv = r["moves"][k - 1]
            mine = np.nonzero(own == rank)[0]
            assert np.array_equal(mv["gid"], mine), (k, rank)
            for a in range(3):
                assert np.array_equal(mv["X"][a], path[k][a][mine]), (k, rank, a)
                assert np.array_equal(mv["attr"][a], 8.0 * mine + a), (k, rank, a)
            assert mv["moved"] == [int(((prev == rank) & (own != rank)).sum()), int(((prev != rank) & (own == rank)).sum())], (k, rank, mv["moved"])
            ghosts = sum(1 for _, to, _ in copies if to == rank)
            sent = sum(1 for l, _, _ in copies if own[l] == rank)
            assert mv["counts"] == [mine.size, ghosts, sent, 8 * ghosts, 32 * sent], (k, rank, mv["counts"], ghosts, sent)


@pytest.mark.parametrize("kind", KINDS)
def test_the_migrated_set_gives_the_bits_of_a_fresh_set_and_of_the_replicated_spread(kind):
    """After the five moves interp of a random u and spread onto a random f0 equal, bit for bit, those of a set created afresh on the same handles at
    the final positions; spread equals fl_ibm_create's bits; both agree with the oracle to test_gpu_ibm_owner's tolerances."""
    case, path, ref, res = _run_moves(kind)
    for rank, r in enumerate(res):
        assert np.array_equal(r["sel"], r["fresh_sel"]) and r["moves"][-1]["counts"] == r["fresh_counts"], rank
        assert np.array_equal(r["U"], r["U_fresh"]), (rank, np.abs(r["U"] - r["U_fresh"]).max())
        assert np.array_equal(r["f"], r["f_fresh"]), (rank, np.abs(r["f"] - r["f_fresh"]).max())
        assert np.array_equal(r["f"], r["f_rep"]), (rank, np.abs(r["f"] - r["f_rep"]).max())
    assert any(not np.array_equal(r["f"], r["f0"]) for r in res)
    _against_oracle(case, ref, res)


# ------------------------------------------------------------------------------------------------ 2. out of reach

def _row_case():
    V = 1
    return Case(n=(32, 8, 8), ranks=(4, 1, 1), bc=[V] * 6, box=[(0.0, 4.0), (0.0, 1.0), (0.0, 1.0)])


def _reach_worker(R, case, X, u):
    import torch
    from fluca_amd import capi
    lib = capi.lib
    P, d, s = _open(R, case)
    out = {}
    with torch.cuda.stream(s):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        m, rc, gid = _select_create(torch, capi, P, 0, [dev(a) for a in X])
        assert rc == 0, rc
        n = int(gid.numel())
        ul = dev(np.stack([_blk(case, d, u[c]) for c in range(3)]))

        def interp():
            U = torch.full((3 * n,), np.nan, dtype=torch.float64, device="cuda")
            capi.check(lib.fl_ibm_interp(m, 3, _ptr(ul), _ptr(U)))
            s.synchronize()
            return U.cpu().numpy()

        out["before"] = (_counts(capi, m), interp())
        for name, x0 in (("far", 2.5), ("near", 1.5)):
            Xn = [a.copy() for a in X]
            Xn[0][0] = x0
            Xl = [dev(a)[gid].contiguous() for a in Xn]
            out[name] = _migrate(lib, m, Xl, 0, None)
            if name == "far":
                out["after_far"] = (_counts(capi, m), interp())
        Xf, g2, _ = _fetch(torch, lib, m, out["near"][1], 0)
        out["gid"] = g2.cpu().numpy()
        lib.fl_ibm_destroy(m)
    P.close()
    return out


def test_a_marker_out_of_reach_is_a_voted_error_and_the_set_survives():
    """Four ranks in a row, 40 markers in block 0.  One marker jumps into block 2, which is no neighbour of block 0: FL_ERR_ARG_OUTOFRANGE on all four
    ranks (nobody waits: the wire's time limit would fail the test), counts and interp give the bits from before.  Into block 1 instead: it moves."""
    case = _row_case()
    rng = np.random.default_rng(5)
    X = [np.ascontiguousarray(rng.uniform(lo, hi, 40)) for lo, hi in ((0.3, 0.9), (0.3, 0.7), (0.3, 0.7))]
    u = rng.standard_normal((3, case.g.ncell))
    owner, copies = _geometry(case, 0, X)
    assert np.all(owner == 0) and any(to == 1 for _, to, _ in copies)
    res = inproc.run_threads(4, _reach_worker, case, X, u, wire_timeout=30.0)
    assert [r["far"][0] for r in res] == [-63] * 4
    for rank, r in enumerate(res):
        assert r["after_far"][0] == r["before"][0] and np.array_equal(r["after_far"][1], r["before"][1]), rank
    assert not np.isnan(res[0]["before"][1]).any() and np.abs(res[0]["before"][1]).max() > 0
    assert [r["near"] for r in res] == [(0, 39, [1, 0]), (0, 1, [0, 1]), (0, 0, [0, 0]), (0, 0, [0, 0])]
    assert np.array_equal(res[0]["gid"], np.arange(1, 40)) and np.array_equal(res[1]["gid"], [0])


# ------------------------------------------------------------------------------------------------ 3. edges of the contract

def _twin_worker(R, case, X, Xnew, ref, kind):
    """fl_ibm_migrate on one set, fl_ibm_update on its twin, the same new positions: moved, and the bits of both"""
    import torch
    from fluca_amd import capi
    lib = capi.lib
    P, d, s = _open(R, case)
    out = {}
    with torch.cuda.stream(s):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        Xd = [dev(a) for a in X]
        ma, rc, gid = _select_create(torch, capi, P, kind, Xd)
        mb, rcb, _ = _select_create(torch, capi, P, kind, Xd)
        assert rc == 0 and rcb == 0
        n = int(gid.numel())
        Xl = [dev(a)[gid].contiguous() for a in Xnew]
        out["migrate"] = _migrate(lib, ma, Xl, 0, None)
        out["update_rc"] = lib.fl_ibm_update(mb, *[_ptr(t) for t in Xl])
        out["small_cap_rc"] = lib.fl_ibm_owned_fetch(ma, n - 1, None, None, None, None, 0, None) if n else -60
        out["a"] = _apply(torch, capi, case, d, ma, ref, gid, dev)[:2]
        out["b"] = _apply(torch, capi, case, d, mb, ref, gid, dev)[:2]
        out["counts"] = (_counts(capi, ma), _counts(capi, mb))
        lib.fl_ibm_destroy(ma)
        lib.fl_ibm_destroy(mb)
    P.close()
    return out


def _same_owner_positions(which):
    """a marker set and a shift of it in y by half a cell that changes no owner"""
    case, h, X = _markers("c5_even", which)
    Xnew = [X[0], np.ascontiguousarray(X[1] + 0.5 * h), X[2]]
    return case, h, X, Xnew


@pytest.mark.parametrize("kind", KINDS)
def test_on_one_rank_nothing_moves_and_the_bits_are_those_of_update(kind):
    _, h, X, Xnew = _same_owner_positions("cylinder+cloud")
    case = Case(**dict(CASES["c5_even"], ranks=(1, 1, 1)))
    ref = _reference(case, h, Xnew, kind)
    r = inproc.run_threads(1, _twin_worker, case, X, Xnew, ref, kind)[0]
    L = X[0].size
    assert r["migrate"] == (0, L, [0, 0]) and r["update_rc"] == 0 and r["small_cap_rc"] == -60          # FL_ERR_ARG_SIZ
    assert np.array_equal(r["a"][0], r["b"][0]) and np.array_equal(r["a"][1], r["b"][1])
    assert np.allclose(r["a"][0], ref["U"], rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("kind", KINDS)
def test_a_call_in_which_no_marker_changes_owner_gives_the_bits_of_update(kind):
    """the face cloud, shifted by half a cell along the face it straddles: moved == [0, 0] on all eight ranks, interp and spread as after fl_ibm_update"""
    case, h, X, Xnew = _same_owner_positions("face")
    assert np.array_equal(_geometry(case, kind, X)[0], _geometry(case, kind, Xnew)[0])
    ref = _reference(case, h, Xnew, kind)
    res = inproc.run_threads(8, _twin_worker, case, X, Xnew, ref, kind)
    assert sum(r["migrate"][1] for r in res) == X[0].size
    for rank, r in enumerate(res):
        assert r["migrate"][0] == 0 and r["migrate"][2] == [0, 0] and r["update_rc"] == 0, (rank, r["migrate"])
        assert r["small_cap_rc"] == -60 and r["counts"][0] == r["counts"][1]
        assert np.array_equal(r["a"][0], r["b"][0]) and np.array_equal(r["a"][1], r["b"][1]), rank


def _refusals_worker(R, case, X, Xfar, Xfar2):
    import torch
    from fluca_amd import capi
    lib = capi.lib
    P, d, s = _open(R, case)
    out = {}
    with torch.cuda.stream(s):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        Xd = [dev(a) for a in X]
        # a set without marker numbers
        m, rc, sel = _select_create(torch, capi, P, 0, Xd, with_gid=False)
        assert rc == 0
        Xl = [t[sel].contiguous() for t in Xd]
        out["no_gid"] = _migrate(lib, m, Xl, 0, None)[0]
        lib.fl_ibm_destroy(m)
        # a replicated set (not collective)
        mr = C.c_void_p()
        capi.check(lib.fl_ibm_create(P.h, 0, X[0].size, *[_ptr(t) for t in Xd], C.byref(mr)))
        out["replicated"] = _migrate(lib, mr, Xd, 0, None)[0]
        out["replicated_fetch"] = lib.fl_ibm_owned_fetch(mr, X[0].size, None, None, None, None, 0, None)
        lib.fl_ibm_destroy(mr)
        # descending numbers on ONE rank (the first that owns two markers or more): the error is everybody's
        flip = (lambda t: torch.flip(t, [0])) if R.rank == 1 else None
        m, rc, sel = _select_create(torch, capi, P, 0, Xd, order=flip)
        assert rc == 0 and (R.rank != 1 or sel.numel() >= 2)
        Xl = [t[sel].contiguous() for t in Xd]
        out["descending"] = _migrate(lib, m, Xl, 0, None)[0]
        out["bad_nattr"] = _migrate(lib, m, Xl, 9 if R.rank == 0 else 0, None)[0]
        out["null"] = lib.fl_ibm_migrate(m, None, None, None, 0, None, C.byref(C.c_int64()), (C.c_int64 * 2)())
        lib.fl_ibm_destroy(m)
        # every marker of rank 0 leaves for rank 1; rank 0 then takes part with NULL arrays
        m, rc, gid = _select_create(torch, capi, P, 0, Xd)
        assert rc == 0
        dV = dev(np.arange(X[0].size) + 0.5)[gid].contiguous()
        r1 = _migrate(lib, m, [dev(a)[gid].contiguous() for a in Xfar], 1, dV)
        _, gid, dV = _fetch(torch, lib, m, r1[1], 1)
        r2 = _migrate(lib, m, [dev(a)[gid].contiguous() for a in Xfar2], 1, dV)       # empty tensors go in as NULL
        _, gid, dV = _fetch(torch, lib, m, r2[1], 1)
        s.synchronize()
        out.update(lose=(r1, r2), gid=gid.cpu().numpy(), dV=dV.cpu().numpy())
        lib.fl_ibm_destroy(m)
    P.close()
    return out


@functools.lru_cache(maxsize=None)
def _run_refusals():
    case, h, X = _markers("c5_even", "face")
    Xfar = [np.ascontiguousarray(X[0] + 4.0 * h), X[1], X[2]]
    Xfar2 = [np.ascontiguousarray(X[0] + 4.5 * h), X[1], X[2]]
    owner = [_geometry(case, 0, a)[0] for a in (X, Xfar, Xfar2)]
    return owner, inproc.run_threads(8, _refusals_worker, case, X, Xfar, Xfar2, wire_timeout=30.0)


def test_sets_that_cannot_migrate_say_so_on_every_rank():
    owner, res = _run_refusals()
    assert (owner[0] == 1).sum() >= 2
    assert [r["no_gid"] for r in res] == [-73] * 8                   # FL_ERR_ARG_WRONGSTATE: created with gid = NULL
    assert [r["replicated"] for r in res] == [-73] * 8 and [r["replicated_fetch"] for r in res] == [-73] * 8
    assert [r["descending"] for r in res] == [-73] * 8               # rank 1's numbers descend: voted
    assert [r["bad_nattr"] for r in res] == [-63] * 8                # rank 0 alone asks for nine attributes: voted
    null = [r["null"] for r in res]
    assert null == [-85] * 8, null                                   # the ranks that own markers hand over no arrays: voted


def test_a_rank_that_loses_all_its_markers_goes_on_with_none():
    owner, res = _run_refusals()
    L = owner[0].size
    n0 = int((owner[0] == 0).sum())
    assert n0 > 0 and np.all(owner[1] == 1) and np.all(owner[2] == 1)
    assert res[0]["lose"] == ((0, 0, [n0, 0]), (0, 0, [0, 0]))
    assert res[1]["lose"] == ((0, L, [0, n0]), (0, L, [0, 0]))
    assert all(r["lose"] == ((0, 0, [0, 0]), (0, 0, [0, 0])) for r in res[2:])
    assert np.array_equal(res[1]["gid"], np.arange(L)) and np.array_equal(res[1]["dV"], np.arange(L) + 0.5)      # the attribute travelled
    assert res[0]["gid"].size == 0
