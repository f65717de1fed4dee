"""CPU: the conditions on the table of tests/interior_ranks.py that keep a case of tests/test_gpu_interior_ranks.py from passing by accident --
every rank grid has a rank with two different neighbours on an axis and fl_halo_plan gives it the two messages of the general branch, the plans
of all ranks pair up, the blocks tile the grid within the library's own limits, the stretched grids tell their cells apart, the marker sets
straddle both faces of the middle block -- and that the first of them fails on the two-rank counterpart of every case.  Host arithmetic only:
fl_decomp_default, fl_decomp_neighbor, fl_decomp_neighbor_offset, fl_halo_plan, and numpy geometry for the markers."""
import ctypes as C

import numpy as np
import pytest

from tests import interior_ranks as ir
from tests.launch_regimes import CHEB2_MIN_CELLS, RANK_BY_NAME, TOY_RANK_BLOCKS, mg_levels


def _rank_grids():
    """every rank grid of the interior-rank GPU tests as an InteriorCase: the table, the vote, the Schur cases, ranks_std_z3"""
    out = list(ir.CASES) + [ir.VOTE]
    for k, (n, ranks, own, bc) in enumerate(ir.SCHUR):
        out.append(ir.InteriorCase(f"schur{k}", n, ranks, own, bc, [(0.0, 1.0), (0.0, 1.0), (0.0, 0.5)], (0, 1, 2), "k_schur_var_ring"))
    reg = RANK_BY_NAME["ranks_std_z3"]
    for bc in reg.bcs:
        out.append(ir.InteriorCase(f"{reg.name}-{'channel' if bc == ir.CHANNEL else 'cavity'}", reg.n, reg.ranks, reg.own, bc,
                                   [(0.0, 1.0), (0.0, 1.0), (0.0, 0.5)], (), reg.reaches))
    return out


GRIDS = _rank_grids()
IDS = [c.name for c in GRIDS]


def two_rank_counterpart(case):
    """the same grid with two ranks on every split axis, default ownership: what the several-rank tests had before"""
    return case.on_ranks(tuple(min(r, 2) for r in case.ranks))


def check_interior_rank(case):
    """At least one rank has lo >= 0, hi >= 0 and lo != hi on an axis, and fl_halo_plan gives every such rank and axis the two messages of its
    general branch: (hi: send my high face under tag 2 ax + 1, receive my high ghost under 2 ax), (lo: send my low face under 2 ax, receive my low
    ghost under 2 ax + 1).  -> the (rank, axis) pairs found"""
    found = []
    for rank in range(case.size):
        nb = ir.neighbours(case, rank)
        plan = ir.halo_plan(case, rank)
        for ax in ir.interior_axes(case, rank):
            lo, hi = nb[ax]
            mine = [m for m in plan if m[1] // 2 == ax]
            assert mine == [(hi, 2 * ax + 1, 2 * ax + 1, 2 * ax + 1, 2 * ax), (lo, 2 * ax, 2 * ax, 2 * ax, 2 * ax + 1)], (case.name, rank, ax, mine)
            found.append((rank, ax))
    assert found, f"{case!r}: no rank has two different neighbours on an axis"
    return found


@pytest.mark.parametrize("case", GRIDS, ids=IDS)
def test_an_interior_rank_exists_and_takes_the_general_branch_of_the_plan(case):
    found = check_interior_rank(case)
    # the offsets -1 and +1 of such an axis lead to the same two ranks (what fl_ibm_plan.h routes ghost copies by)
    from fluca_amd import capi
    per = (C.c_int * 3)(*[int(p) for p in case.periodic])
    for rank, ax in found:
        d = case.decomp(rank)
        got = []
        for o in (-1, 1):
            off = [0, 0, 0]
            off[ax] = o
            got.append(capi.lib.fl_decomp_neighbor_offset(C.byref(d), per, (C.c_int * 3)(*off)))
        assert tuple(got) == ir.neighbours(case, rank)[ax] and got[0] != got[1]
    # a rank in the middle of a non-periodic axis touches no boundary of it
    for rank, ax in found:
        d = case.decomp(rank)
        if not case.periodic[ax]:
            assert 0 < d.lo[ax] and d.lo[ax] + d.len[ax] < case.n[ax]


@pytest.mark.parametrize("case", GRIDS, ids=IDS)
def test_the_table_is_sensitive_the_two_rank_counterpart_has_no_interior_rank(case):
    """the negative example: with two ranks per split axis the check above fails -- every rank touches a boundary or has the same peer twice"""
    two = two_rank_counterpart(case)
    assert two.size >= 2 and two.size < case.size
    with pytest.raises(AssertionError, match="no rank has two different neighbours"):
        check_interior_rank(two)


@pytest.mark.parametrize("case", GRIDS, ids=IDS)
def test_the_plans_of_all_ranks_pair_up(case):
    """every send has the one matching receive: the peer holds exactly one message from me whose receive tag is my send tag, and it fills the
    ghost layer opposite the face I sent"""
    plans = [ir.halo_plan(case, r) for r in range(case.size)]
    nsend = nrecv = 0
    for me, plan in enumerate(plans):
        assert len(plan) == len(set(plan))
        for peer, sb, rb, stag, rtag in plan:
            assert 0 <= peer < case.size and peer != me
            match = [m for m in plans[peer] if m[0] == me and m[4] == stag]
            assert len(match) == 1, (case.name, me, peer, stag, match)
            assert match[0][2] == sb ^ 1, (case.name, me, peer, sb, match)
            nsend += 1
            nrecv += sum(1 for m in plans[peer] if m[0] == me and m[2] >= 0 and m[4] == stag)
    assert nsend == nrecv == sum(len(p) for p in plans)


def _library_ratio(case):
    """the coarsening ratio of the first multigrid level as mg_build_levels (fl_mg.hip) decides it on several ranks: an axis is halved when
    n % (2 ranks) == 0, n / ranks >= 8 and every rank's range starts even and is even"""
    decs = [case.decomp(r) for r in range(case.size)]
    out = []
    for a in range(3):
        n, m = case.n[a], case.ranks[a]
        ok = n % (2 * m) == 0 and n // m >= ir.MG_MIN_EVEN and all(d.lo[a] % 2 == 0 and d.len[a] % 2 == 0 for d in decs)
        out.append(2 if ok else 1)
    return tuple(out)


@pytest.mark.parametrize("case", GRIDS, ids=IDS)
def test_the_blocks_tile_the_grid_within_the_library_s_limits(case):
    decs = [case.decomp(r) for r in range(case.size)]
    blocks = case.blocks()
    # tiling: per axis the ranges of the rank coordinates are consecutive and add up; every rank of a coordinate has the same range
    for a in range(3):
        ranges = {}
        for d in decs:
            ranges.setdefault(int(d.coord[a]), set()).add((int(d.lo[a]), int(d.len[a])))
        assert sorted(ranges) == list(range(case.ranks[a])) and all(len(v) == 1 for v in ranges.values())
        at = 0
        for c in range(case.ranks[a]):
            lo, ln = next(iter(ranges[c]))
            assert lo == at and ln >= 1
            at += ln
        assert at == case.n[a]
    assert sum(b[0] * b[1] * b[2] for b in blocks) == case.n[0] * case.n[1] * case.n[2]
    # the fused smoother: at least 2 cells per axis on every block
    assert all(min(b) >= ir.CHEB2_MIN for b in blocks), blocks
    # owner-rank markers: at least 4 cells along every split axis
    if case.name in ir.IBM:
        assert all(b[a] >= ir.IBM_OWNER_MIN for b in blocks for a in range(3) if case.ranks[a] > 1), blocks
    # where the case is meant to coarsen: every block coarsens by itself (even ranges of at least 8 cells, tests/launch_regimes.py::mg_levels),
    # all blocks by the same ratio, and that is the library's collective decision and the oracle's on the undecomposed grid
    if case.coarsens:
        ratios = set()
        for b in blocks:
            lv = mg_levels(b)
            assert len(lv) >= 2, (case.name, b)
            ratios.add(tuple(p // q for p, q in zip(lv[0], lv[1])))
        assert len(ratios) == 1, ratios
        glob = mg_levels(case.n)
        assert ratios == {_library_ratio(case)} == {tuple(p // q for p, q in zip(glob[0], glob[1]))}, (ratios, _library_ratio(case), glob[:2])
        for a in range(3):
            if _library_ratio(case)[a] == 2:
                assert all(b[a] % 2 == 0 and b[a] >= ir.MG_MIN_EVEN for b in blocks)


def test_the_three_blocks_of_the_vote_straddle_the_fuse_threshold_and_disagree_about_z():
    """exactly the middle block is below fl_cheb2_agree's 32768 cells, so the collective answer is "not fused" although two of three ranks would;
    on their own the outer blocks would halve z and the middle one would not (31 planes): the library's collective rule and MgOracle both leave z
    alone, so there is one hierarchy"""
    case = ir.VOTE
    cells = [b[0] * b[1] * b[2] for b in case.blocks()]
    assert [c >= CHEB2_MIN_CELLS for c in cells] == [True, False, True], cells
    own = [tuple(p // q for p, q in zip(*mg_levels(b)[:2])) for b in case.blocks()]
    assert own == [(2, 2, 2), (2, 2, 1), (2, 2, 2)]
    glob = mg_levels(case.n)
    assert _library_ratio(case) == (2, 2, 1) == tuple(p // q for p, q in zip(glob[0], glob[1]))
    # the issue's own example grid, 32 x 32 x (32 + 30 + 32), straddles too -- but MgOracle would halve its 94 planes and the library would not
    ex = ir.InteriorCase("ex", (32, 32, 94), (1, 1, 3), ([32], [32], [32, 30, 32]), case.bc, case.box, (), "")
    assert [b[0] * b[1] * b[2] >= CHEB2_MIN_CELLS for b in ex.blocks()] == [True, False, True]
    assert _library_ratio(ex)[2] == 1 and mg_levels(ex.n)[1][2] == 47


def _rows(g, d, c):
    """[cell][offset -2..2] of the viscous rows and [cell][offset -2..1] of the B rows of the cells' low faces along axis d, component c"""
    lap, b = np.zeros((g.n[d], 5)), np.zeros((g.n[d], 4))
    for i in range(g.n[d]):
        for off, v in g.lap_row(d, i, c):
            lap[i, off + 2] += v
        for col, v in g.B_row(d, i, c):
            off = col - i
            if g.periodic[d]:          # a column through the seam
                off = off - g.n[d] if off > 2 else off + g.n[d] if off < -2 else off
            b[i, off + 2] += v
    return lap, b


@pytest.mark.parametrize("case", [c for c in ir.CASES if c.stretched], ids=[c.name for c in ir.CASES if c.stretched])
def test_stretched_cases_tell_every_two_cells_of_an_axis_apart(case):
    """On a stretched axis no two cells share their 1-D table rows (the viscous row and the B rows of the low face): a rank that reads the rows
    of another cell -- an offset by its lo, by a block length, by the neighbour's -- reads other numbers, by far more than the parity tolerance
    of 2e-13.  On the uniform axes of the same case two inner cells do share them, which is why the case is stretched."""
    g = case.g
    for d in range(3):
        for c in range(3):
            lap, b = _rows(g, d, c)
            n = case.n[d]
            # per pair of cells: how far apart their numbers are, relative to the largest of their kind (the larger of the two kinds)
            apart = np.max([np.abs(r[:, None, :] - r[None, :, :]).max(axis=2) / np.abs(r).max() for r in (lap, b)], axis=0)
            off = apart[~np.eye(n, dtype=bool)]
            if d in case.stretched:
                assert off.min() >= 1e-7, (case.name, d, c, off.min())
            elif n >= 6:
                assert off.min() <= 1e-14, (case.name, d, c, off.min())


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", ir.IBM)
def test_the_body_straddles_both_faces_of_the_middle_block(name, kind):
    """numpy geometry (tests/test_gpu_ibm_owner.py::_geometry, the owner rule and the supports of include/fluca_hip.h): the middle rank owns markers,
    holds ghost copies of markers of its low AND of its high neighbour and sends copies of its own to both; on z4_periodic copies also cross the
    seam between rank 3 and rank 0"""
    from tests.test_gpu_ibm_owner import _geometry
    case = ir.BY_NAME[name]
    X = ir.markers(name)
    owner, copies = _geometry(case, kind, X)
    counts = [int((owner == r).sum()) for r in range(case.size)]
    assert counts[1] > 0 and counts[0] > 0 and counts[2] > 0, counts
    into = {(int(owner[l]), to) for l, to, _ in copies}
    print(f"{name} kind {kind}: owned per rank {counts}, copies {len(copies)}, (owner, holder) pairs {sorted(into)}")
    assert {(0, 1), (2, 1), (1, 0), (1, 2)} <= into, into
    if name == "z4_periodic":
        assert {(3, 0), (0, 3)} <= into, into


@pytest.mark.parametrize("name", ir.IBM)
def test_the_migration_path_leaves_the_middle_block_both_ways_and_one_marker_runs_through_it(name):
    from tests.test_gpu_ibm_owner import _geometry
    case = ir.BY_NAME[name]
    path, runner = ir.migration_path(name)
    own = [_geometry(case, 0, X)[0] for X in path]
    a, b = own[0], own[1]
    moves = {(int(p), int(q)) for p, q in zip(a, b) if p != q}
    assert {(1, 0), (1, 2), (0, 1), (2, 1)} <= moves, moves          # call 1: leavers in both directions, arrivals from both sides
    assert [int(o[runner]) for o in own] == [0, 1, 2]                # the runner: 0 -> 1 in call 1, 1 -> 2 in call 2
    for p, q in zip(own[:-1], own[1:]):                              # nobody jumps further than to a neighbour (FL_ERR_ARG_OUTOFRANGE otherwise)
        step = np.abs(p - q)
        assert np.all((step <= 1) | (case.periodic[int(np.argmax(case.ranks))] & (step == case.size - 1))), (name, step.max())
    assert int((own[1] != own[2]).sum()) == 1                        # call 2 moves the runner alone


def test_the_toy_block_list_has_the_new_blocks():
    """tests/launch_regimes.py::TOY_RANK_BLOCKS (checked there to take no 8-wave plan) gains the blocks of the table, the vote and the Schur cases"""
    for case in GRIDS:
        if case.name.startswith("ranks_std_z3"):      # no toy block: it is there for its 8-wave plan
            continue
        for b in case.blocks():
            assert b in TOY_RANK_BLOCKS, (case.name, b)
