"""-m gpu: owner-rank IBM markers (fl_ibm_owned_select / fl_ibm_create_owned / fl_ibm_owned_counts, include/fluca_hip.h) on the 2 x 2 x 2 rank
grid of tests/test_gpu_config5.py, eight host threads over the in-process wire.

A marker lives on the rank whose block holds the cell nearest to it; where its support reaches into a neighbouring block -- across a face, an
edge or a corner, through the periodic seam too -- that neighbour holds a ghost copy.  Interpolation returns the ghosts' partial sums to the
owners, spreading sends F and dV of the copies out; no field travels and nothing is all-reduced.  Checked here: the results against the
single-domain CPU oracle (the tolerances of the replicated test), spreading bit for bit against the replicated path, the partition and the copy
counts against a numpy recomputation from geometry, the bytes on the wire, the edges of the contract, and whole time steps through the C host
mirror with -ns_ibm_marker_distribution owner.

One run of eight ranks per (case, marker set, delta function) serves several tests (cached): a run costs more than what is asserted on it."""
import contextlib
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import inproc
from tests.test_gpu_config5 import CASES, Case, _blk, _cylinder, _gather, _handle, _mirror_run

pytestmark = pytest.mark.gpu

KINDS = [0, 1]      # FL_DELTA_PESKIN4, FL_DELTA_ROMA3


# ------------------------------------------------------------------------------------------------ marker sets (seeded)

def _cloud(centres_counts, h, seed=23):
    """uniform points in cubes of half-width 3 h, the groups drawn one after the other from one generator"""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(-3 * h, 3 * h, (3, count)) + np.asarray(centre)[:, None] for centre, count in centres_counts]
    return np.concatenate(parts, axis=1)


def _markers(name, which):
    case = Case(**CASES[name])
    h = (case.box[0][1] - case.box[0][0]) / case.n[0]
    if which == "cylinder":
        X = _cylinder(case.box, h)
    elif which == "cylinder+cloud":
        # the cylinder's supports cross faces and edges only; the cloud sits where the eight blocks meet and on the periodic seam below that point
        # (z taken modulo the span), so that corner copies exist
        cl = _cloud([((1.0, 0.75, 0.5), 200), ((1.0, 0.75, 0.0), 100)], h)
        cl[2] %= 1.0
        X = [np.concatenate([a, b]) for a, b in zip(_cylinder(case.box, h), cl)]
    elif which == "face":
        # the middle of the face between the two x ranks of the low-y, low-z blocks, more than six cells from every other rank face
        X = list(_cloud([((1.0, 0.4, 0.25), 100)], h))
    else:
        raise KeyError(which)
    return case, h, [np.ascontiguousarray(a) for a in X]


def _reference(case, h, X, kind, seed=17):
    g = case.g
    L = X[0].size
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((3, g.ncell))
    F = rng.standard_normal((3, L))
    dV = rng.uniform(0.5, 1.5, L) * h ** 3
    f0 = rng.standard_normal((3, g.ncell))
    vol = np.einsum("k,j,i->kji", *[np.diff(case.xf[a]) for a in (2, 1, 0)]).ravel()
    return dict(X=X, u=u, F=F, dV=dV, f0=f0, vol=vol, U=g.ibm_interp(kind, X, u), f=g.ibm_spread(kind, X, dV, F, f0.copy()))


# ------------------------------------------------------------------------------------------------ geometry in numpy: owners and the ranks a support touches

def _decomps(case):
    from fluca_amd import capi
    from tests import mp_common as mpc
    size = case.ranks[0] * case.ranks[1] * case.ranks[2]
    return [mpc.decomp_of(capi, case.n, case.ranks, r, getattr(case, "own", None)) for r in range(size)]


def _index(case, a, x):
    """continuous cell-centre index along axis a: piecewise linear through the centres, beyond the first / last one through its mirror image in the
    wall or the periodic image"""
    xf = np.asarray(case.xf[a])
    n = case.n[a]
    dx = np.diff(xf)
    if np.allclose(dx, dx[0], rtol=1e-10, atol=0):
        return (x - xf[0]) / ((xf[-1] - xf[0]) / n) - 0.5
    xc = 0.5 * (xf[1:] + xf[:-1])
    if case.periodic[a]:
        ext = np.concatenate([[xc[-1] - (xf[-1] - xf[0])], xc, [xc[0] + (xf[-1] - xf[0])]])
    else:
        ext = np.concatenate([[2 * xf[0] - xc[0]], xc, [2 * xf[-1] - xc[-1]]])
    j = np.clip(np.searchsorted(ext, x, side="right") - 1, 0, n)      # ext[j] <= x < ext[j + 1]; ext[j] is centre j - 1
    return (j - 1) + (x - ext[j]) / (ext[j + 1] - ext[j])


def _geometry(case, kind, X):
    """owner rank of every marker (the rule of include/fluca_hip.h) and the (marker, rank, number of axes the rank differs from the owner on) of
    every ghost copy: a rank other than the owner whose block holds at least one cell of the marker's support"""
    S = 4 if kind == 0 else 3
    decs = _decomps(case)
    L = X[0].size
    own_c, touch = [], []
    for a in range(3):
        n, m = case.n[a], case.ranks[a]
        lo = sorted({int(d.lo[a]) for d in decs})
        assert len(lo) == m
        coord_of = lambda cell: np.searchsorted(lo, cell, side="right") - 1
        s = _index(case, a, X[a])
        c = np.floor(s + 0.5).astype(int)
        c = c % n if case.periodic[a] else np.clip(c, 0, n - 1)
        own_c.append(coord_of(c))
        i0 = (np.floor(s).astype(int) if kind == 0 else np.floor(s + 0.5).astype(int)) - 1
        t = np.zeros((L, m), dtype=bool)
        for k in range(S):
            cell = i0 + k
            ok = np.ones(L, dtype=bool)
            if case.periodic[a]:
                cell = cell % n
            else:
                ok = (cell >= 0) & (cell < n)
            t[np.nonzero(ok)[0], coord_of(cell[ok])] = True
        touch.append(t)
    rank_of = lambda cx, cy, cz: (cz * case.ranks[1] + cy) * case.ranks[0] + cx
    owner = rank_of(*own_c)
    copies = []
    for l in range(L):
        for cz, cy, cx in itertools.product(*[np.nonzero(touch[a][l])[0] for a in (2, 1, 0)]):
            r = rank_of(cx, cy, cz)
            if r != owner[l]:
                copies.append((l, int(r), int(cx != own_c[0][l]) + int(cy != own_c[1][l]) + int(cz != own_c[2][l])))
    return owner, copies


# ------------------------------------------------------------------------------------------------ the worker: one rank of an owned set

def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t.numel() else None


def _owner_worker(R, case, ref, kind, replicated, hand_to=None, with_gid=True):
    """hand_to: {rank: indices} overrides what that rank hands to fl_ibm_create_owned (the wrong-rank case)"""
    import torch
    from fluca_amd import capi
    from fluca_amd.poisson import Poisson
    lib = capi.lib
    if R.size > 1:
        P, d, s = _handle(R, case)
    else:       # one rank: the whole grid, no communicator
        P, s = Poisson(case.n, case.xf, case.bc, case.kappa), torch.cuda.Stream()
        P.set_stream(s)
        d = _decomps(case)[0]
    out = {}
    with torch.cuda.stream(s):
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), device="cuda")
        X, L = ref["X"], ref["X"][0].size
        Xd = [dev(a) for a in X]
        idx = torch.zeros(L, dtype=torch.int64, device="cuda")
        cnt = C.c_int64(-1)
        capi.check(lib.fl_ibm_owned_select(P.h, kind, L, *[_ptr(t) for t in Xd], _ptr(idx), C.byref(cnt)), "fl_ibm_owned_select")
        sel = idx[:cnt.value].clone()
        out["sel"] = sel.cpu().numpy()
        if hand_to is not None and R.rank in hand_to:
            sel = torch.as_tensor(np.asarray(hand_to[R.rank], dtype=np.int64), device="cuda")
        n = int(sel.numel())
        Xl = [t[sel].contiguous() for t in Xd]
        m = C.c_void_p()
        out["create_rc"] = lib.fl_ibm_create_owned(P.h, kind, n, *[_ptr(t) for t in Xl], _ptr(sel) if with_gid else None, C.byref(m))
        if out["create_rc"] == 0:
            c5 = (C.c_int64 * 5)()
            capi.check(lib.fl_ibm_owned_counts(m, c5), "fl_ibm_owned_counts")
            out["counts"] = list(c5)
            blk3 = lambda a: np.stack([_blk(case, d, a[c]) for c in range(3)])
            ul, f0b = dev(blk3(ref["u"])), blk3(ref["f0"])
            U = torch.full((3 * n,), np.nan, dtype=torch.float64, device="cuda")
            Fl, dVl = dev(ref["F"]).reshape(3, L)[:, sel].contiguous(), dev(ref["dV"])[sel].contiguous()
            fl = dev(f0b)
            s.synchronize()
            st0 = R.stats()
            capi.check(lib.fl_ibm_interp(m, 3, _ptr(ul), _ptr(U)), "fl_ibm_interp (owned)")
            s.synchronize()
            st1 = R.stats()
            capi.check(lib.fl_ibm_spread(m, 3, _ptr(Fl), _ptr(dVl), _ptr(fl)), "fl_ibm_spread (owned)")
            s.synchronize()
            st2 = R.stats()
            out["interp_wire"] = {k: st1[k] - st0[k] for k in st0}
            out["spread_wire"] = {k: st2[k] - st1[k] for k in st0}
            out.update(U=U.cpu().numpy().reshape(3, n), f=fl.cpu().numpy().reshape(3, -1), f0=f0b, vol=_blk(case, d, ref["vol"]))
            # the same markers once more (fl_ibm_update routes and bins anew): the same bits
            capi.check(lib.fl_ibm_update(m, *[_ptr(t) for t in Xl]), "fl_ibm_update (owned)")
            U2, fl2 = torch.full_like(U, np.nan), dev(f0b)
            capi.check(lib.fl_ibm_interp(m, 3, _ptr(ul), _ptr(U2)))
            capi.check(lib.fl_ibm_spread(m, 3, _ptr(Fl), _ptr(dVl), _ptr(fl2)))
            s.synchronize()
            out["update_same"] = bool(torch.equal(U, U2) and torch.equal(fl, fl2))
            c5b = (C.c_int64 * 5)()
            capi.check(lib.fl_ibm_owned_counts(m, c5b))
            out["update_same"] = out["update_same"] and list(c5b) == out["counts"]
            if replicated:
                mr = C.c_void_p()
                capi.check(lib.fl_ibm_create(P.h, kind, L, *[_ptr(t) for t in Xd], C.byref(mr)), "fl_ibm_create")
                Ur, fr = torch.empty(3 * L, dtype=torch.float64, device="cuda"), dev(f0b)
                s.synchronize()
                st0 = R.stats()
                capi.check(lib.fl_ibm_interp(mr, 3, _ptr(ul), _ptr(Ur)))
                s.synchronize()
                out["rep_interp_wire"] = {k: R.stats()[k] - st0[k] for k in st0}
                Fr, dVr = dev(ref["F"]), dev(ref["dV"])      # named: a temporary would be freed, and its block handed out again, before the call
                capi.check(lib.fl_ibm_spread(mr, 3, _ptr(Fr), _ptr(dVr), _ptr(fr)))
                s.synchronize()
                out.update(U_rep=Ur.cpu().numpy().reshape(3, L), f_rep=fr.cpu().numpy().reshape(3, -1), rep_counts_rc=lib.fl_ibm_owned_counts(mr, c5b))
                lib.fl_ibm_destroy(mr)
            lib.fl_ibm_destroy(m)
    P.close()
    return out


@functools.lru_cache(maxsize=None)
def _run(name, which, kind, replicated=True):
    case, h, X = _markers(name, which)
    ref = _reference(case, h, X, kind)
    res = inproc.run_threads(8, _owner_worker, case, ref, kind, replicated)
    assert all(r["create_rc"] == 0 for r in res), [r["create_rc"] for r in res]
    return case, h, ref, res


def _against_oracle(case, ref, res):
    L = ref["X"][0].size
    tot = np.zeros(3)
    for rank, r in enumerate(res):
        sel = r["sel"]
        assert np.allclose(r["U"], ref["U"][:, sel], rtol=1e-12, atol=1e-13), ("interp", rank, np.abs(r["U"] - ref["U"][:, sel]).max())
        d = _decomps(case)[rank] if len(res) > 1 else None
        want = np.stack([_blk(case, d, ref["f"][c]) for c in range(3)]) if d is not None else ref["f"]
        assert np.allclose(r["f"], want, rtol=1e-12, atol=1e-12 * abs(ref["f"]).max()), ("spread", rank, np.abs(r["f"] - want).max())
        tot += ((r["f"] - r["f0"]) * r["vol"][None, :]).sum(axis=1)
    # conservation over the ranks: sum_x (f - f0) V_cell = sum_l F_l dV_l
    want = (ref["F"] * ref["dV"][None, :]).sum(axis=1)
    assert np.allclose(tot, want, rtol=1e-9, atol=1e-9 * (np.abs(ref["F"]) * ref["dV"][None, :]).sum()), (tot, want)
    assert sum(r["sel"].size for r in res) == L


# ------------------------------------------------------------------------------------------------ 1. against the oracle

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,which", [("c5_even", "cylinder+cloud"), ("c5_uneven_stretched", "cylinder")])
def test_owned_markers_match_the_oracle_on_the_2x2x2_rank_grid(name, which, kind):
    """Every rank selects its markers (fl_ibm_owned_select) and creates an owned set; interp of a random u against Grid.ibm_interp, spread onto a
    random f0 against Grid.ibm_spread, with the replicated test's tolerances (the partial sums of a marker are added per rank and then in offset
    order, where the oracle adds them cell by cell: last bits), and conservation of the spread force over the ranks.  Equal blocks with the cylinder
    and the corner cloud; uneven blocks on a wall-clustered y axis with the cylinder."""
    case, h, ref, res = _run(name, which, kind, name == "c5_even")
    _against_oracle(case, ref, res)
    assert all(r["update_same"] for r in res)


# ------------------------------------------------------------------------------------------------ 2. spreading: the replicated path's bits

@pytest.mark.parametrize("kind", KINDS)
def test_owned_spreading_gives_the_bits_of_the_replicated_path(kind):
    """gid = the global index: a tile's bin holds the same markers in the same order as with fl_ibm_create on the same rank grid, and the weights come
    from the same kernel on the same positions -- f is equal bit for bit.  U agrees to the oracle's tolerance (the replicated path adds the ranks'
    partial sums in rank order inside the all-reduce, the owned one in offset order)."""
    case, h, ref, res = _run("c5_even", "cylinder+cloud", kind)
    for rank, r in enumerate(res):
        assert np.array_equal(r["f"], r["f_rep"]), (rank, np.abs(r["f"] - r["f_rep"]).max())
        assert np.allclose(r["U"], r["U_rep"][:, r["sel"]], rtol=1e-12, atol=1e-13), rank
    assert any(not np.array_equal(r["f"], r["f0"]) for r in res)


# ------------------------------------------------------------------------------------------------ 3. partition and counts

@pytest.mark.parametrize("kind", KINDS)
def test_selections_partition_the_markers_and_the_counts_are_the_geometric_ones(kind):
    case, h, ref, res = _run("c5_even", "cylinder+cloud", kind)
    L = ref["X"][0].size
    owner, copies = _geometry(case, kind, ref["X"])
    allsel = np.concatenate([r["sel"] for r in res])
    assert allsel.size == L and np.array_equal(np.sort(allsel), np.arange(L))            # disjoint, and they cover the list
    by_level = {1: 0, 2: 0, 3: 0}
    for _, _, level in copies:
        by_level[level] += 1
    print(f"kind {kind}: L = {L}, copies = {len(copies)} (face {by_level[1]}, edge {by_level[2]}, corner {by_level[3]}), owned per rank "
          f"{[int((owner == r).sum()) for r in range(8)]}")
    for rank, r in enumerate(res):
        assert np.array_equal(r["sel"], np.nonzero(owner == rank)[0]), rank              # ascending global indices of the rank's own markers
        ghosts = sum(1 for _, to, _ in copies if to == rank)
        sent = sum(1 for l, _, _ in copies if owner[l] == rank)
        assert r["counts"] == [int((owner == rank).sum()), ghosts, sent, 8 * ghosts, 32 * sent], (rank, r["counts"], ghosts, sent)
    # the path across faces, edges AND corners is exercised (what the corner cloud is for)
    assert by_level[1] > 0 and by_level[2] > 0 and by_level[3] > 0, by_level


# ------------------------------------------------------------------------------------------------ 4. the wire

@pytest.mark.parametrize("kind", KINDS)
def test_no_allreduce_and_the_bytes_on_the_wire_are_the_counted_ones(kind):
    case, h, ref, res = _run("c5_even", "cylinder+cloud", kind)
    copies = sum(r["counts"][2] for r in res)
    assert copies == sum(r["counts"][1] for r in res) > 0
    for r in res:
        assert r["interp_wire"]["allreduces"] == 0 and r["spread_wire"]["allreduces"] == 0
        assert r["rep_interp_wire"]["allreduces"] == 1
        assert r["interp_wire"]["bytes"] == 3 * r["counts"][3] and r["spread_wire"]["bytes"] == r["counts"][4]
        assert r["interp_wire"]["exchanges"] <= 1 and r["spread_wire"]["exchanges"] <= 1
    assert sum(r["interp_wire"]["bytes"] for r in res) == 24 * copies
    assert sum(r["spread_wire"]["bytes"] for r in res) == sum(r["counts"][4] for r in res) == 32 * copies


# ------------------------------------------------------------------------------------------------ 5. edges of the contract

@pytest.mark.parametrize("kind", KINDS)
def test_one_rank_gives_the_bits_of_the_replicated_set(kind):
    case, h, X = _markers("c5_even", "cylinder+cloud")
    case = Case(**dict(CASES["c5_even"], ranks=(1, 1, 1)))
    ref = _reference(case, h, X, kind)
    r = inproc.run_threads(1, _owner_worker, case, ref, kind, True)[0]
    L = X[0].size
    assert r["create_rc"] == 0 and r["counts"] == [L, 0, 0, 0, 0] and np.array_equal(r["sel"], np.arange(L))
    assert np.array_equal(r["U"], r["U_rep"]) and np.array_equal(r["f"], r["f_rep"])
    assert r["rep_counts_rc"] == -73                                                    # FL_ERR_ARG_WRONGSTATE on a replicated set
    assert r["interp_wire"]["exchanges"] == 0 and r["spread_wire"]["exchanges"] == 0
    _against_oracle(case, ref, [r])


@pytest.mark.parametrize("kind", KINDS)
def test_ranks_without_markers_take_part_and_their_field_stays(kind):
    """100 markers around the middle of one face between two x ranks: six ranks own nothing and hold no ghost; they pass L_local = 0 with NULL
    arrays, every call succeeds, their f is untouched.  Without marker numbers (gid = NULL: own markers, then ghosts) on top."""
    case, h, ref, res = _run("c5_even", "face", kind, False)
    empty = [rank for rank, r in enumerate(res) if r["counts"][:3] == [0, 0, 0]]
    assert len(empty) == 6, [r["counts"] for r in res]
    for rank in empty:
        assert res[rank]["sel"].size == 0 and np.array_equal(res[rank]["f"], res[rank]["f0"]) and res[rank]["interp_wire"]["exchanges"] == 0
    assert sum(r["counts"][2] for r in res) > 0                                         # the two others do exchange copies
    _against_oracle(case, ref, res)
    res = inproc.run_threads(8, functools.partial(_owner_worker, with_gid=False), case, ref, kind, False)
    assert all(r["create_rc"] == 0 for r in res)
    _against_oracle(case, ref, res)


def test_a_marker_on_the_wrong_rank_is_an_error_on_every_rank_and_nobody_hangs():
    """Rank 0 hands over one marker of rank 7's next to its own: FL_ERR_ARG_OUTOFRANGE, voted, on all eight ranks -- the seven others do not wait in an
    exchange rank 0 never enters (the wire's time limit would fail the test)."""
    case, h, X = _markers("c5_even", "cylinder+cloud")
    ref = _reference(case, h, X, 0)
    owner, _ = _geometry(case, 0, X)
    mine, foreign = np.nonzero(owner == 0)[0], np.nonzero(owner == 7)[0]
    assert mine.size and foreign.size
    hand = {0: np.concatenate([mine, foreign[:1]])}
    res = inproc.run_threads(8, functools.partial(_owner_worker, hand_to=hand), case, ref, 0, False, wire_timeout=30.0)
    assert [r["create_rc"] for r in res] == [-63] * 8


def test_owned_counts_refuse_a_replicated_set():
    case, h, ref, res = _run("c5_even", "cylinder+cloud", 0)
    assert all(r["rep_counts_rc"] == -73 for r in res)                                  # FL_ERR_ARG_WRONGSTATE


# ------------------------------------------------------------------------------------------------ 6. whole time steps through the C host mirror

@contextlib.contextmanager
def _extra_options(*opts):
    """_mirror_run builds its option list with hostapi.argv: append to it for the duration of a run (set before the rank threads start)"""
    from fluca_amd import hostapi as H
    plain = H.argv
    H.argv = lambda *a: plain(*a, *opts)
    try:
        yield
    finally:
        H.argv = plain


def test_nsstep_with_owner_rank_markers_on_the_2x2x2_rank_grid():
    """The channel with the cylinder of markers held at rest by direct forcing (test_gpu_config5's), -ns_ibm_marker_distribution owner on eight ranks
    against the undecomposed run: v and V to 1e-8, p to 1e-7, as the replicated markers are held to."""
    from fluca_amd import hostapi as H
    n, ranks, nsteps = (32, 24, 16), (2, 2, 2), 3
    with _extra_options("-ns_ibm_marker_distribution", "owner"):
        parts = inproc.run_threads(8, _mirror_run, n, ranks, nsteps, True)
    v, V, p = _gather(parts, n)
    one = inproc.run_threads(1, lambda R: _mirror_run(None, n, ranks, nsteps, True))
    v1, V1, p1 = _gather(one, n)
    free = inproc.run_threads(1, lambda R: _mirror_run(None, n, ranks, nsteps, False))
    vf, _, _ = _gather(free, n)
    assert np.linalg.norm(v1 - vf) >= 1e-3 * np.linalg.norm(vf)           # the forcing does something
    assert np.linalg.norm(v - v1) <= 1e-8 * np.linalg.norm(v1)
    for d in range(3):
        assert np.linalg.norm(V[d] - V1[d]) <= 1e-8 * max(np.linalg.norm(V1[d]), 1e-12), d
    assert np.linalg.norm(p - p1) <= 1e-7 * np.linalg.norm(p1)
    ns = C.c_void_p()
    assert H.lib.NSCreate(C.byref(ns)) == 0
    argc, av = H.argv("-ns_ibm_marker_distribution", "scattered")
    assert H.lib.NSSetFromOptions(ns, argc, av) == H.ERR_ARG_UNKNOWN_TYPE
    H.lib.NSDestroy(C.byref(ns))
